"""Timing of the onNewNode triage verdicts (kad_rt_triage_batch) against two kernels this work does
not touch, on the same candidate IDs:

    find_bucket      kad_rt_find_bucket_batch: the locate alone, the floor of any per-candidate table question
    rows8_a, rows8_b kad_rt_closest_batch at count 8, twice (the gap between the two is the spread of one arm)
    triage           the verdict call (verdict + node)
    triage_bucket    the same, also writing the bucket index (what opendht_amd.ingest asks for)
    triage_deferred  the form that loads the status bytes after the key compare instead of together with the keys
                     (KAD_TRIAGE_KERNEL=deferred in the tools build; same results, one line less for known IDs,
                     one dependent step more for new ones)

Tables: the bench shard (one 1/8 shard of the 100M-node U(24) table, statuses as the bench has them) and a
split-policy table of 1M nodes in steady state (90 % good, none expired). Candidate mixes, 1M each, a different
batch for every launch of every arm: `realistic` (80 % IDs of the table's own nodes, 20 % new ones) and `all_new`. Arms are
interleaved launch by launch within a round, every launch timed by its own pair of events; the figure is the median
over all launches of an arm, with the quartiles. The kinds each mix produces are counted on batch 0.

    python tools/triage_bench.py [--rounds 20] [--reps 8] [--out profiles/r08/triage/triage_bench.json]

--pmc MIX: no timing; the bench shard, that mix, 10 launches of find_bucket, rows8 and triage each, for a counter
run of its own (rocprofv3 --pmc <counters> --kernel-trace -- python tools/triage_bench.py --pmc realistic); the
kernels are told apart by name in the trace.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opendht_amd._lib as _kl  # noqa: E402

_kl.use_ablation_build()  # the deferred variant lives only in the tools build
from opendht_amd import KAD_NN_KIND_MASK, KAD_NN_MYBUCKET, DeviceTable  # noqa: E402
from opendht_amd import synth as S  # noqa: E402
from opendht_amd.sharded import build_shard, config3_spec  # noqa: E402

KINDS = ("none", "known", "replace", "insert", "split", "full")


def measure(T, ids_host, new_batches, self_id, args, dev):
    """Both mixes on one table. new_batches: host arrays of new candidate IDs (one per batch)."""
    rng = np.random.default_rng(0x7B1A)
    n = ids_host.shape[0]
    mixes = {"realistic": [], "all_new": []}
    for nb in new_batches:
        q = nb.shape[0]
        m = nb.copy()
        known = rng.random(q) < 0.8
        m[known] = ids_host[rng.integers(0, n, size=int(known.sum()))]
        mixes["realistic"].append(torch.from_numpy(m).to(dev))
        mixes["all_new"].append(torch.from_numpy(nb).to(dev))
    q = args.queries
    stream = torch.cuda.current_stream(dev)
    idx = torch.empty((q, 8), dtype=torch.int32, device=dev)
    cnt = torch.empty((q,), dtype=torch.uint8, device=dev)
    fb = torch.empty((q,), dtype=torch.int32, device=dev)
    out = (torch.empty((q,), dtype=torch.uint8, device=dev), torch.empty((q,), dtype=torch.int32, device=dev), None)
    outb = (out[0], out[1], torch.empty((q,), dtype=torch.int32, device=dev))
    oute = (torch.empty((q,), dtype=torch.uint8, device=dev), torch.empty((q,), dtype=torch.int32, device=dev), None)

    def deferred(tg):
        os.environ["KAD_TRIAGE_KERNEL"] = "deferred"
        T.rt_triage(tg, self_id, True, out=oute, stream=stream.cuda_stream)
        del os.environ["KAD_TRIAGE_KERNEL"]

    res = {}
    for mix, tgs in mixes.items():
        if args.pmc and mix != args.pmc:
            continue
        arms = {
            "find_bucket": lambda j: T.find_bucket(tgs[j], out=fb, stream=stream.cuda_stream),
            "rows8_a": lambda j: T.rt_closest(tgs[j], 8, idx, cnt, stream=stream.cuda_stream),
            "triage": lambda j: T.rt_triage(tgs[j], self_id, True, out=out, stream=stream.cuda_stream),
            "rows8_b": lambda j: T.rt_closest(tgs[j], 8, idx, cnt, stream=stream.cuda_stream),
            "triage_bucket": lambda j: T.rt_triage(tgs[j], self_id, True, out=outb, stream=stream.cuda_stream),
            "triage_deferred": lambda j: deferred(tgs[j]),
        }
        for j in range(len(tgs)):  # every batch once through every arm
            for fn in arms.values():
                fn(j)
        torch.cuda.synchronize()
        if args.pmc:
            for a in ("find_bucket", "rows8_a", "triage"):
                for r in range(10):
                    arms[a](r % len(tgs))
                torch.cuda.synchronize()
            return {}
        arms["find_bucket"](0)
        arms["triage_bucket"](0)
        arms["triage_deferred"](0)
        torch.cuda.synchronize()
        v = outb[0].cpu().numpy()
        same_bucket = bool(np.array_equal(outb[2].cpu().numpy(), fb.cpu().numpy()))
        same_deferred = bool(np.array_equal(oute[0].cpu().numpy(), v) and np.array_equal(oute[1].cpu().numpy(), outb[1].cpu().numpy()))
        hist = {k: int(((v & KAD_NN_KIND_MASK) == i).sum()) for i, k in enumerate(KINDS)}
        per = {a: [] for a in arms}
        launch = 0
        for rd in range(args.rounds):
            evs = []
            for r in range(args.reps):  # interleaved launch by launch, each with its own events
                for a, fn in arms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    # the next batch for every launch: an arm never runs on the IDs the arm before it just pulled
                    # through the caches (with one batch per repetition the last arm measured 10-15 us low)
                    fn(launch % len(tgs))
                    launch += 1
                    e1.record(stream)
                    evs.append((a, e0, e1))
            torch.cuda.synchronize()
            for a, e0, e1 in evs:
                per[a].append(e0.elapsed_time(e1) * 1e3)
        r = {"kinds_batch0": hist, "mybucket_batch0": int(((v & KAD_NN_MYBUCKET) != 0).sum()),
             "bucket_equals_find_bucket": same_bucket, "deferred_equals_default": same_deferred,
             "launches_per_arm": args.rounds * args.reps,
             "arms": {a: {"per_launch_us_median": float(np.median(per[a])),
                          "per_launch_us_q25": float(np.percentile(per[a], 25)),
                          "per_launch_us_q75": float(np.percentile(per[a], 75))} for a in arms}}
        m = {a: r["arms"][a]["per_launch_us_median"] for a in arms}
        r["rows8_spread_us"] = abs(m["rows8_a"] - m["rows8_b"])
        r["triage_minus_rows8_us"] = m["triage"] - 0.5 * (m["rows8_a"] + m["rows8_b"])
        r["triage_minus_find_bucket_us"] = m["triage"] - m["find_bucket"]
        res[mix] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--batches", type=int, default=7,
                    help="distinct candidate batches, one per launch in turn (coprime to the number of arms)")
    ap.add_argument("--split-nodes", type=int, default=1_000_000)
    ap.add_argument("--tables", default="shard,split")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pmc", default=None, choices=("realistic", "all_new"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    self_id = np.random.default_rng(0x5E1F).integers(0, 256, size=20, dtype=np.uint8)
    res = {"queries": args.queries, "bytes_per_candidate": {
        "streamed": "20 in, 1 + 4 out (+ 4 with the bucket index)",
        "table": "16 (dir[b], dir[b+1].x) + 8 per node of the bucket (keys); a key match: + 12 (that node's tail); no "
                 "equal ID: + 1 per node (status bytes). Each of the three is its own random 64-byte line or two"}}
    which = ["shard"] if args.pmc else args.tables.split(",")
    if "shard" in which:
        spec = config3_spec()
        sh = build_shard(spec, 0)
        new = [spec.targets_for(0, args.queries, seed=0x7A1A0001 + j) for j in range(args.batches)]
        T = DeviceTable(sh.ids, sh.status, sh.first, sh.off, device=0, index_base=sh.index_base, sorted=True)
        res["bench_shard"] = {"nodes": int(T.n), "buckets": int(T.B),
                              **measure(T, np.asarray(sh.ids).reshape(-1, 20), new, self_id, args, dev)}
        T.close()
        del sh
    if "split" in which:
        ids = S.random_ids(args.split_nodes, 0x7A1A5)
        perm, first, off = S.split_table(ids)
        ids = np.ascontiguousarray(ids[perm])
        st = S.random_status(ids.shape[0], 0x7A1A6, 90, 0)
        new = [S.random_ids(args.queries, 0x7A1A7 + j) for j in range(args.batches)]
        T = DeviceTable(ids, st, first, off, device=0)
        res["split_table"] = {"nodes": int(T.n), "buckets": int(T.B), **measure(T, ids, new, self_id, args, dev)}
        T.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
