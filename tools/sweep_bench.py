"""Timing of the whole-table sweep (kad_table_sweep) and of kad_table_expire, on the bench shard
(one 1/8 shard of the 100M-node U(24) table) and on a split-policy table of 1M nodes.

Sweep arms, each against a streaming floor taken in the same run (a plain torch sum over an int64 tensor of the byte
count the arm reads; never the code under test):

    totals    the counts alone                 reads n status bytes + 8 (B + 1) directory bytes
    lists     the counts and both lists        the same, plus the bit maps once more ((n + B) / 8 bytes)
    incoming  the counts with KAD_SWEEP_INCOMING  the same as totals, plus time and reply_time (16 n bytes)

Arms and floors are interleaved launch by launch within a round, every launch timed by its own pair of events; the
figure is the median over all launches of an arm, with the quartiles. `stats_today` is what a caller pays for the same
totals without the sweep: export_status() (one byte per node over PCIe) and a numpy count, wall clock.

kad_table_expire against today's route (kad_table_apply with the same REMOVE ops, then set_times and set_addrs from host
arrays already gathered for the survivors, outside the timing; DeviceTable.expire()'s own n + B words of host output
arrays are inside it), wall clock, alternating which goes first, at 0.01 %, 1 % and 10 % of the nodes expired. Every
repetition builds fresh twin tables with times and wire records and gives each twin one untimed warm-up round of the
same fraction by its own route (a periodic job on a live table: pool and pinned read-back buffer have their size), so
every sample of a fraction is taken at one table size, (1 - fraction) of the full one; the timed round marks the same
random nodes expired on both.

    python tools/sweep_bench.py [--rounds 20] [--reps 6] [--out profiles/r10/sweep/sweep_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opendht_amd import DeviceTable  # noqa: E402
from opendht_amd import synth as S  # noqa: E402
from opendht_amd._lib import KAD_OP_REMOVE, KAD_SWEEP_INCOMING, lib, ptr  # noqa: E402
from opendht_amd.sharded import build_shard, config3_spec  # noqa: E402

NOW = 10**13


def draw_times(n, seed):
    rng = np.random.default_rng(seed)
    t = NOW - rng.integers(1, 5 * 60 * 10**9, size=n)
    r = np.where(rng.random(n) < 0.5, t - rng.integers(1, 10**9, size=n), t + 1).astype(np.int64)
    return t.astype(np.int64), r, np.zeros(n, np.uint8)


def stats(v):
    return {"per_launch_us_median": float(np.median(v)), "per_launch_us_q25": float(np.percentile(v, 25)),
            "per_launch_us_q75": float(np.percentile(v, 75))}


def sweep_arms(T, args, dev):
    L = lib()
    n, B = T.n, T.B
    stream = torch.cuda.current_stream(dev)
    tot = torch.empty(8, dtype=torch.int32, device=dev)
    nodes = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    buckets = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
    read = {"totals": n + 8 * (B + 1), "lists": n + 8 * (B + 1) + (n + B) // 8, "incoming": n + 8 * (B + 1) + 16 * n}
    floors = {a: torch.ones((b + 7) // 8, dtype=torch.int64, device=dev) for a, b in read.items()}

    def sweep(flags, lists):
        rc = L.kad_table_sweep(T.handle, flags, ptr(tot), ptr(nodes) if lists else None, n if lists else 0,
                               ptr(buckets) if lists else None, B if lists else 0, stream.cuda_stream)
        assert rc == 0, L.kad_last_error()

    arms = {"totals": lambda: sweep(0, False), "floor_totals": lambda: floors["totals"].sum(),
            "lists": lambda: sweep(0, True), "floor_lists": lambda: floors["lists"].sum(),
            "incoming": lambda: sweep(KAD_SWEEP_INCOMING, False), "floor_incoming": lambda: floors["incoming"].sum()}
    for _ in range(3):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    per = {a: [] for a in arms}
    for _ in range(args.rounds):
        evs = []
        for _ in range(args.reps):
            for a, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                evs.append((a, e0, e1))
        torch.cuda.synchronize()
        for a, e0, e1 in evs:
            per[a].append(e0.elapsed_time(e1) * 1e3)
    res = {"bytes_read": read, "launches_per_arm": args.rounds * args.reps, "arms": {a: stats(per[a]) for a in arms}}
    for a in read:
        res["arms"][a]["over_floor"] = res["arms"][a]["per_launch_us_median"] / res["arms"]["floor_" + a]["per_launch_us_median"]
    sweep(KAD_SWEEP_INCOMING, True)
    torch.cuda.synchronize()
    res["totals"] = dict(zip(("good", "dubious", "expired", "incoming", "changed_buckets", "empty_buckets"),
                             (int(x) for x in tot.cpu().numpy().view(np.uint32)[:6])))
    # today's route to the same totals: the status bytes over PCIe, counted on the host
    wall = []
    for _ in range(5):
        t0 = time.perf_counter()
        st = T.export_status()
        good = int(np.count_nonzero(st & 1))
        expired = int(np.count_nonzero(st & 2))
        dubious = int(np.count_nonzero((st & 3) == 0))
        wall.append((time.perf_counter() - t0) * 1e6)
    assert (good, dubious, expired) == (res["totals"]["good"], res["totals"]["dubious"], res["totals"]["expired"])
    res["stats_today_export_numpy_us_median"] = float(np.median(wall))
    return res


def expire_arms(make, times, addrs, args):
    """make(): a fresh table. Every repetition builds fresh twins A (kad_table_expire) and B (apply + set_times +
    set_addrs), so all samples of a fraction are taken at one table size. Each twin first takes a warm-up round of the
    same fraction by its own route, untimed (the state of a periodic job on a live table: the engine's pool and the
    table's pinned read-back buffer have their size); the timed round then marks the same random nodes expired on both,
    on the table the warm-up left ((1 - fraction) of the full size)."""
    rng = np.random.default_rng(0xE791)
    out = {}

    def mark(tables, n, gone):
        two = np.full(gone.shape[0], 2, np.uint8)
        old = np.flatnonzero(tables[0].export_status() & 2).astype(np.uint32)  # what the table's own statuses hold
        for X in tables:
            if old.shape[0]:
                X.patch_status(old, np.zeros(old.shape[0], np.uint8))
            X.patch_status(gone, two)
        keep = np.ones(n, bool)
        keep[gone] = False
        ops = np.zeros((gone.shape[0], 3), np.uint32)
        ops[:, 0], ops[:, 1] = KAD_OP_REMOVE, gone
        return keep, ops

    for name, frac in (("0.01%", 1e-4), ("1%", 1e-2), ("10%", 1e-1)):
        wa, wb = [], []
        for rep in range(args.expire_reps):
            A, Bt = make(), make()
            t, r, e = times
            ad = addrs
            for X in (A, Bt):
                X.set_times(t, r, e)
                X.set_addrs(ad)
            for timed in (False, True):
                n = A.n
                m = max(1, int(n * frac))
                gone = np.sort(rng.choice(n, size=m, replace=False)).astype(np.uint32)
                keep, ops = mark((A, Bt), n, gone)
                t, r, e, ad = (np.ascontiguousarray(x[keep]) for x in (t, r, e, ad))
                torch.cuda.synchronize()

                def run_a():
                    t0 = time.perf_counter()
                    removed, _ = A.expire()
                    dt = (time.perf_counter() - t0) * 1e3
                    if timed:
                        wa.append(dt)
                    if os.environ.get("KAD_DEBUG"):
                        print(f"expire() wall {dt:.3f} ms ({name}, timed={timed})", file=sys.stderr, flush=True)
                    assert np.array_equal(removed - np.uint32(A.index_base), gone)

                def run_b():
                    t0 = time.perf_counter()
                    Bt.apply(ops)
                    Bt.set_times(t, r, e)
                    Bt.set_addrs(ad)
                    dt = (time.perf_counter() - t0) * 1e3
                    if timed:
                        wb.append(dt)
                    if os.environ.get("KAD_DEBUG"):
                        print(f"today's route wall {dt:.3f} ms ({name}, timed={timed})", file=sys.stderr, flush=True)

                for fn in ((run_a, run_b) if rep % 2 == 0 else (run_b, run_a)):
                    fn()
                assert A.n == Bt.n == int(keep.sum())
            same = all(np.array_equal(a, b) for a, b in zip(A.export(), Bt.export()))
            assert same, "twins differ"
            A.close()
            Bt.close()
        out[name] = {"nodes": int(n), "removed": int(gone.shape[0]),
                     "expire_ms": wa, "apply_set_times_set_addrs_ms": wb,
                     "expire_faster_in_rounds": int(sum(a < b for a, b in zip(wa, wb))),
                     "expire_ms_median": float(np.median(wa)), "today_ms_median": float(np.median(wb))}
    out["twins_equal_at_end"] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--expire-reps", type=int, default=3)
    ap.add_argument("--split-nodes", type=int, default=1_000_000)
    ap.add_argument("--tables", default="shard,split")
    ap.add_argument("--skip-expire", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for which in args.tables.split(","):
        if which == "shard":
            sh = build_shard(config3_spec(), 0)
            ids, st, first, off, base, srt = sh.ids, sh.status, sh.first, sh.off, sh.index_base, True
        else:
            ids = S.random_ids(args.split_nodes, 0x7A1A5)
            perm, first, off = S.split_table(ids)
            ids = np.ascontiguousarray(ids[perm])
            st, base, srt = S.random_status(ids.shape[0], 0x7A1A6, 80, 10), 0, False

        def make():
            return DeviceTable(ids, st, first, off, device=0, index_base=base, sorted=srt)

        T = make()
        times = draw_times(T.n, 0x71AE)
        T.set_times(*times)
        r = {"nodes": int(T.n), "buckets": int(T.B), "sweep": sweep_arms(T, args, dev)}
        T.close()
        if not args.skip_expire:
            addrs = np.random.default_rng(0xADD5).integers(0, 256, size=(len(times[0]), 6), dtype=np.uint8)
            r["expire"] = expire_arms(make, times, addrs, args)
        res["bench_shard" if which == "shard" else "split_table"] = r
        text = json.dumps(res, indent=1)
        if args.out:  # after every table, so a run cut short leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
