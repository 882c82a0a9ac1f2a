"""Timing of the bucket-time calls on the bench shard (one 1/8 shard of the 100M-node U(24) table) and
on a split-policy table of 1M nodes, one process per table, medians of 5 after a warm-up as tools/sweep_bench.py.

  scan     kad_table_maintenance at three staleness settings (0 %, 1 % and 100 % of the buckets stale; empty buckets
           are candidates at every setting), the totals alone (cap 0) and the totals with the list (cap B), each
           launch timed by its own pair of events. Beside it, taken in the same run:
             host_route   what a caller without the scan does: the offsets from kad_table_export, a host array of
                          times, the test of dht.cpp:2833 in numpy (wall clock)
             floor        a torch sum over 16 bytes per bucket (the bytes the count pass reads when nothing is a candidate)
  touch    kad_table_touch_buckets of 1M IDs, against kad_rt_find_bucket_batch alone on the same IDs, and against
           find_bucket + read-back + a numpy scatter into a host array of times (wall clock)
  host     what a table that uses bucket times pays on the host side: kad_table_apply of the same batch (one split, 64
           inserts) on twin tables with and without bucket times, and kad_table_set_bucket_times of B entries beside
           the kad_table_create of the same snapshot

    python tools/maint_bench.py [--out profiles/r19/maint/maint_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOW = 10**15
TEN_MIN = 600 * 10**9
REPS = 5


def med(v):
    return float(np.median(v))


def run_table(which, split_nodes):
    import torch

    from opendht_amd import DeviceTable
    from opendht_amd import synth as S
    from opendht_amd._lib import KAD_OP_INSERT, KAD_OP_SPLIT, lib, ptr
    from opendht_amd.sharded import build_shard, config3_spec

    dev = torch.device("cuda:0")
    if which == "shard":
        sh = build_shard(config3_spec(), 0)
        ids, st, first, off, base, srt = sh.ids, sh.status, sh.first, sh.off, sh.index_base, True
    else:
        ids = S.random_ids(split_nodes, 0x7A1A5)
        perm, first, off = S.split_table(ids)
        ids = np.ascontiguousarray(ids[perm])
        st, base, srt = S.random_status(ids.shape[0], 0x7A1A6, 80, 10), 0, False

    def make():
        return DeviceTable(ids, st, first, off, device=0, index_base=base, sorted=srt)

    t0 = time.perf_counter()
    T = make()
    create_ms = (time.perf_counter() - t0) * 1e3
    n, B = T.n, T.B
    L = lib()
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(0x3A17)
    res = {"nodes": int(n), "buckets": int(B), "create_ms": create_ms, "scan": {}}

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        return med(out)

    tot = torch.empty(8, dtype=torch.int32, device=dev)
    rec = torch.empty((B, 2), dtype=torch.int32, device=dev)
    floor = torch.ones(2 * B, dtype=torch.int64, device=dev)

    def scan(cap):
        rc = L.kad_table_maintenance(T.handle, NOW, 0, ptr(tot), ptr(rec) if cap else None, cap, stream.cuda_stream)
        assert rc == 0, L.kad_last_error()

    for name, frac in (("0%", 0.0), ("1%", 0.01), ("100%", 1.0)):
        tm = np.where(rng.random(B) < frac, NOW - TEN_MIN - 1, NOW).astype(np.int64)
        t0 = time.perf_counter()
        T.set_bucket_times(tm)
        set_ms = (time.perf_counter() - t0) * 1e3
        r = {"totals_us": timed(lambda: scan(0)), "totals_and_list_us": timed(lambda: scan(B)),
             "floor_sum_16B_per_bucket_us": timed(lambda: floor.sum()), "set_bucket_times_ms": set_ms}
        scan(B)
        torch.cuda.synchronize()
        v = tot.cpu().numpy().view(np.uint32)
        r["candidates"], r["stale"], r["empty"] = int(v[0]), int(v[1]), int(v[2])
        wall = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            o = np.zeros(B + 1, np.uint32)
            assert L.kad_table_export(T.handle, None, None, None, ptr(o)) == 0
            cand = np.flatnonzero((tm < NOW - TEN_MIN) | (np.diff(o.astype(np.int64)) == 0))
            wall.append((time.perf_counter() - t0) * 1e6)
        assert cand.shape[0] == r["candidates"]
        assert np.array_equal(rec[:cand.shape[0], 0].cpu().numpy().view(np.uint32), cand.astype(np.uint32))
        r["host_route_export_numpy_us"] = med(wall)
        r["bytes_model"] = 16 * B + 40 * r["candidates"] + 8 * r["candidates"]
        res["scan"][name] = r

    # touch
    q = 1 << 20
    tg = torch.from_numpy(S.random_ids(q, 0x70C4)).to(dev)
    out = torch.empty(q, dtype=torch.int32, device=dev)

    def touch(with_out):
        rc = L.kad_table_touch_buckets(T.handle, ptr(tg), q, NOW, ptr(out) if with_out else None, stream.cuda_stream)
        assert rc == 0, L.kad_last_error()

    def find():
        rc = L.kad_rt_find_bucket_batch(T.handle, ptr(tg), q, ptr(out), stream.cuda_stream)
        assert rc == 0, L.kad_last_error()

    res["touch"] = {"ids": q, "touch_us": timed(lambda: touch(False)), "touch_with_buckets_us": timed(lambda: touch(True)),
                    "find_bucket_us": timed(find)}
    host_tm = np.zeros(B, np.int64)
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        find()
        host_tm[out.cpu().numpy().view(np.uint32)] = NOW
        wall.append((time.perf_counter() - t0) * 1e6)
    res["touch"]["find_readback_scatter_us"] = med(wall)
    want = np.full(B, NOW, np.int64)
    T.set_bucket_times(want - 1)
    touch(True)
    torch.cuda.synchronize()
    got = T.bucket_times()
    assert np.array_equal(got == NOW, host_tm == NOW)
    T.close()

    # host-side costs: the same apply on twins with and without bucket times
    new_ids = S.random_ids(64, 0xA991)
    ops = np.zeros((65, 3), np.uint32)
    ops[0] = (KAD_OP_SPLIT, B // 2, 0)
    ops[1:, 0], ops[1:, 1] = KAD_OP_INSERT, np.arange(64)
    arms = {"with_times": [], "without_times": []}
    for rep in range(3):
        for arm in (("with_times", "without_times") if rep % 2 == 0 else ("without_times", "with_times")):
            X = make()
            if arm == "with_times":
                X.set_bucket_times(np.full(B, NOW, np.int64))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            X.apply(ops, new_ids, np.ones(64, np.uint8))
            arms[arm].append((time.perf_counter() - t0) * 1e3)
            assert X.B == B + 1
            X.close()
    res["host"] = {"apply_split_64_inserts_ms": {k: med(v) for k, v in arms.items()}, "apply_samples_ms": arms}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None, help="internal: run one table in this process")
    ap.add_argument("--split-nodes", type=int, default=1_000_000)
    ap.add_argument("--tables", default="shard,split")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.table:
        print("RESULT " + json.dumps(run_table(args.table, args.split_nodes)))
        return
    res = {}
    for which in args.tables.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--table", which, "--split-nodes",
                            str(args.split_nodes)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{which}: exit {r.returncode}")
        line = next(x for x in r.stdout.splitlines() if x.startswith("RESULT "))
        res["bench_shard" if which == "shard" else "split_table"] = json.loads(line[7:])
        text = json.dumps(res, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
