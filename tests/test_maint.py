"""kad_table_maintenance on the GPU: the scan of Dht::bucketMaintenance over the device's bucket times and directory,
record for record and total for total against the host twin (kad_maint_scan_host) and against the yardstick of
tests/maint_ref.py (the reference's loop one bucket at a time). Every comparison is exact."""
import numpy as np
import pytest
import torch

import maint_ref as R
import sweep_ref
import tables as TB
from opendht_amd import DeviceTable, maint_scan_host
from opendht_amd import _lib
from opendht_amd import synth as S
from opendht_amd._lib import lib, ptr

NOW = 10**15
_CACHE = {}


def _open(t, gpu, **kw):
    return DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0, **kw)


def _rec_bytes(r):
    return r.cpu().numpy().tobytes() if torch.is_tensor(r) else r.tobytes()


def _same(got, want, what=""):
    assert got["totals"] == want["totals"], (what, got["totals"], want["totals"])
    assert _rec_bytes(got["records"]) == want["records"].tobytes(), what


def _all_three(T, t, tm, want, what="", **kw):
    """device form, host form and the twin against `want`."""
    _same(T.maintenance(NOW, **kw), want, (what, "device"))
    _same(T.maintenance_host(NOW, **kw), want, (what, "host"))
    _same(maint_scan_host(t["off"], t["first"], tm, NOW, **kw), want, (what, "twin"))


def cut(t, B):
    """The first B buckets of table t as a table (the last one then reaches to the end of the ID space)."""
    n = int(t["off"][B])
    return TB.table(t["ids"][:n], t["status"][:n], t["first"][:B], t["off"][:B + 1], name=f"{t['name']}_B{B}")


def shapes():
    if not _CACHE:
        _CACHE["uniform"] = TB.uniform_config(10_000, 11)
        _CACHE["split"] = TB.split_config(10_000)
        assert _CACHE["uniform"]["first"].shape[0] == 2048 and _CACHE["split"]["first"].shape[0] >= 1025
    return _CACHE


@pytest.mark.gpu
def test_every_small_table(gpu):
    """The 30 width patterns of B <= 4 as device tables, the 340 time patterns through set_bucket_times."""
    seen = 0
    for w in R.width_patterns():
        ids, first, off = R.table_of_widths(w)
        t = TB.table(ids, np.ones(ids.shape[0], np.uint8), first, off)
        with _open(t, gpu) as T:
            for tm in [c[1] for c in R.small_cases(NOW) if c[0] == w]:
                tm = np.array(tm, np.int64)
                T.set_bucket_times(tm)
                np.testing.assert_array_equal(T.bucket_times(), tm)
                _all_three(T, t, tm, R.scan(off, first, tm, NOW), (w, tm))
                seen += 1
    assert seen == 340


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["uniform", "split"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_bucket_counts(gpu, shape, B):
    t = cut(shapes()[shape], B)
    tm = R.draw_times(B, NOW, 0x3A + B)
    want = R.scan(t["off"], t["first"], tm, NOW)
    if B >= 63:
        assert 0 < want["totals"]["candidates"] < B
    with _open(t, gpu) as T:
        T.set_bucket_times(tm)
        _all_three(T, t, tm, want, t["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sparse_good", "S10000"])
def test_named_tables(gpu, name):
    t = TB.sparse_good_table() if name == "sparse_good" else TB.split_config(10_000)
    B = t["first"].shape[0]
    if name == "sparse_good":
        assert int((np.diff(t["off"].astype(np.int64)) == 0).sum()) == 282
    tm = R.draw_times(B, NOW, 0x77)
    want = R.scan(t["off"], t["first"], tm, NOW)
    tot = want["totals"]
    assert tot["sure"] > 0 and tot["stale"] > 0 and (name != "sparse_good" or (tot["empty"] >= 282 and tot["maybe"] > 0))
    with _open(t, gpu) as T:
        T.set_bucket_times(tm)
        _all_three(T, t, tm, want, name)


@pytest.mark.gpu
def test_more_buckets_than_one_scan_round(gpu):
    """2^20 buckets are 4096 tiles; the one-workgroup scan takes 2048 per round, so the second half's bases come through
    the carry. The whole list against the twin; the yardstick (plain Python) on the slices where it matters: the start,
    the round boundary and the end."""
    big = sweep_ref.big_table()
    first, off = S.uniform_buckets(big["ids"], 20)
    t = TB.table(big["ids"], big["status"], first, off, name="U20_1200000")
    B = first.shape[0]
    assert B > 524_288
    tm = R.draw_times(B, NOW, 0x20)
    twin = maint_scan_host(off, first, tm, NOW)
    assert twin["totals"]["candidates"] > 600_000
    assert (twin["records"]["bucket"] > 524_288).sum() > 300_000
    bk = twin["records"]["bucket"]
    for fb in (0, 524_288 - 1500, B - 3000):
        ref = R.scan(off, first, tm, NOW, first_bucket=fb, stop=fb + 3000)
        assert ref["totals"]["candidates"] > 1500
        assert ref["records"].tobytes() == twin["records"][(bk >= fb) & (bk < fb + 3000)].tobytes()
    with _open(t, gpu) as T:
        T.set_bucket_times(tm)
        _same(T.maintenance(NOW), twin, "device")
        _same(T.maintenance_host(NOW), twin, "host")
        fb = 524_288 - 700
        want = maint_scan_host(off, first, tm, NOW, first_bucket=fb, cap=1000)
        _same(T.maintenance(NOW, first_bucket=fb, cap=1000), want, "resume across the round boundary")


def _s10000(gpu):
    t = shapes()["split"]
    tm = R.draw_times(t["first"].shape[0], NOW, 0x51)
    if "s_want" not in _CACHE:
        _CACHE["s_want"] = R.scan(t["off"], t["first"], tm, NOW)
    return t, tm, _CACHE["s_want"]


@pytest.mark.gpu
def test_caps_and_canary(gpu):
    t, tm, full = _s10000(gpu)
    count = full["totals"]["candidates"]
    assert count > 300
    with _open(t, gpu) as T:
        T.set_bucket_times(tm)
        for cap in (0, 1, count - 1, count, count + 1):
            buf = torch.full((count + 8, 2), -0x55555556, dtype=torch.int32, device=gpu)
            got = T.maintenance(NOW, cap=cap, out=buf)
            assert got["totals"] == full["totals"]
            m = min(cap, count)
            raw = buf.cpu().numpy()
            assert raw[:m].tobytes() == full["records"][:m].tobytes()
            assert (raw[m:].view(np.uint32) == 0xAAAAAAAA).all()
            h = T.maintenance_host(NOW, cap=cap)
            assert h["totals"] == full["totals"] and h["records"].tobytes() == full["records"][:m].tobytes()


@pytest.mark.gpu
def test_first_bucket_and_resume(gpu):
    t, tm, full = _s10000(gpu)
    B = t["first"].shape[0]
    rec = full["records"]
    with _open(t, gpu) as T:
        T.set_bucket_times(tm)
        for fb in (0, 1, 255, 256, 257, B - 1, B):
            want = R.scan(t["off"], t["first"], tm, NOW, first_bucket=fb)
            assert want["records"].tobytes() == rec[rec["bucket"] >= fb].tobytes()
            _all_three(T, t, tm, want, fb, first_bucket=fb)
        got, fb, calls = [], 0, 0
        while True:
            r = T.maintenance(NOW, first_bucket=fb, cap=100)
            part = r["records"].cpu().numpy().view(np.uint32)
            got.append(part)
            calls += 1
            if r["totals"]["candidates"] <= 100:
                break
            fb = int(part[-1, 0]) + 1
        assert calls == (rec.shape[0] + 99) // 100
        assert np.concatenate(got).tobytes() == rec.tobytes()


@pytest.mark.gpu
def test_never_set_equals_all_min(gpu):
    t = shapes()["split"]
    B = t["first"].shape[0]
    want = R.scan(t["off"], t["first"], None, NOW)
    assert want["totals"]["candidates"] == B == want["totals"]["stale"]
    with _open(t, gpu) as T:
        assert (T.bucket_times() == R.INT64_MIN).all()
        _all_three(T, t, None, want, "never set")
        a = T.maintenance(NOW)
        T.set_bucket_times(None)  # still no array: the same path
        _same(T.maintenance(NOW), want, "NULL on a table without times")
        T.set_bucket_times(np.full(B, R.INT64_MIN, np.int64))
        b = T.maintenance(NOW)
        _same(b, want, "all INT64_MIN")
        assert torch.equal(a["records"], b["records"])
        T.set_bucket_times(np.full(B, NOW, np.int64))
        assert T.maintenance(NOW)["totals"]["stale"] == 0
        T.set_bucket_times(None)
        assert (T.bucket_times() == R.INT64_MIN).all()
        _same(T.maintenance(NOW), want, "reset")


@pytest.mark.gpu
def test_two_streams(gpu):
    t, tm, full = _s10000(gpu)
    B = t["first"].shape[0]
    with _open(t, gpu) as T:
        T.set_bucket_times(tm)
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        outs = [(torch.empty(8, dtype=torch.int32, device=gpu), torch.zeros((B, 2), dtype=torch.int32, device=gpu))
                for _ in range(2)]
        torch.cuda.synchronize()
        L = lib()
        for _ in range(3):
            for s, (tot, rec) in zip((s1, s2), outs):
                rc = L.kad_table_maintenance(T.handle, NOW, 0, ptr(tot), ptr(rec), B, s.cuda_stream)
                assert rc == 0, L.kad_last_error()
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        for tot, rec in outs:
            assert [int(x) for x in tot.cpu().numpy().view(np.uint32)] == list(full["totals"].values())
            assert rec.cpu().numpy()[:full["records"].shape[0]].tobytes() == full["records"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["uniform", "split"])
def test_table_unchanged_by_bucket_time_calls(gpu, shape):
    """export, export_lines and a count-8 query give the same bytes before and after touch, set, patch, maintenance."""
    t = shapes()[shape]
    B = t["first"].shape[0]
    targets = TB.adversarial_targets(t, extra=512)
    tg = torch.from_numpy(targets).to(gpu)

    def state(T):
        idx, cnt = T.rt_closest(tg, 8)
        torch.cuda.synchronize()
        parts = [a.tobytes() for a in T.export()] + [idx.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes()]
        for which in range(13):
            x = T.export_lines(which)
            parts.append(b"" if x is None else x.tobytes())
        return parts, T.info()["device_bytes"]

    with _open(t, gpu) as T:
        before, bytes0 = state(T)
        T.touch_buckets(tg, NOW)
        T.set_bucket_times(R.draw_times(B, NOW, 5))
        T.patch_bucket_times([0, B - 1, 0], [1, 2, 3])
        T.touch_buckets(targets[:10], NOW + 1)
        T.maintenance(NOW)
        T.maintenance_host(NOW)
        after, bytes1 = state(T)
        assert before == after
        assert bytes1 >= bytes0 + 8 * B  # the times are counted in the table's device bytes
