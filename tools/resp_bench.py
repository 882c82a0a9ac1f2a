"""Timing of the storage-responsibility verdicts (kad_rt_responsible_batch) against the rows they
replace, on the bench workload: one 1/8 shard of the 100M-node table, U(d), 1M targets, a different batch per
launch. Arms, interleaved launch by launch within a round:

    rows_a, rows_b   rt_closest at count 8, twice (the gap between the two is the spread of one arm)
    resp             the verdict call, random self_id (nearly every query decided by its line)
    resp_loads       the same with the line-decided verdicts compiled out (KAD_RESP_KERNEL=noshortcut in the
                     tools build): every query loads key[last]

Every launch is timed by its own pair of events; the figure is the median over all launches of an arm, with the
quartiles; the mean of back-to-back groups is given beside it. The verdicts of both forms are checked against
the rows plus a host xor compare, and the share of queries the line decides is read from the statistics build
(KAD_RESP_KERNEL=stats).

    python tools/resp_bench.py [--rounds 20] [--reps 8] [--out profiles/r07/resp/resp_bench.json]
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

_kl.use_ablation_build()  # the noshortcut / stats variants live only in the tools build
from opendht_amd import DeviceTable  # noqa: E402
from opendht_amd.sharded import build_shard, config3_spec  # noqa: E402


def host_verdicts(ids, base, targets, rows, cnt, self_id):
    """far = cnt >= 1 and (id(row[cnt-1]) ^ h) < (self_id ^ h), bytewise big-endian."""
    q = targets.shape[0]
    has = cnt >= 1
    last = np.where(has, rows[np.arange(q), np.maximum(cnt.astype(np.int64), 1) - 1] - np.uint32(base), 0)
    da = ids[last] ^ targets
    ds = self_id[None, :] ^ targets
    ne = da != ds
    f = ne.argmax(1)
    r = np.arange(q)
    return (has & ne.any(1) & (da[r, f] < ds[r, f])).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--batches", type=int, default=8, help="distinct target batches, one per launch in turn")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = config3_spec()
    sh = build_shard(spec, 0)
    host_tg = [spec.targets_for(0, args.queries, seed=0x0D470002 + j) for j in range(args.batches)]
    tgs = [torch.from_numpy(t).to(dev) for t in host_tg]
    T = DeviceTable(sh.ids, sh.status, sh.first, sh.off, device=0, index_base=sh.index_base, sorted=True)
    self_id = np.random.default_rng(0x5E1F).integers(0, 256, size=20, dtype=np.uint8)
    stream = torch.cuda.current_stream(dev)
    idx = torch.empty((args.queries, 8), dtype=torch.int32, device=dev)
    cnt = torch.empty((args.queries,), dtype=torch.uint8, device=dev)
    far = torch.empty((args.queries,), dtype=torch.uint8, device=dev)

    def rows(j):
        T.rt_closest(tgs[j], 8, idx, cnt, stream=stream.cuda_stream)

    def resp(j):
        T.rt_responsible(tgs[j], self_id, 8, 1, out=far, stream=stream.cuda_stream)

    def resp_loads(j):
        os.environ["KAD_RESP_KERNEL"] = "noshortcut"
        resp(j)
        del os.environ["KAD_RESP_KERNEL"]

    arms = {"rows_a": rows, "resp": resp, "rows_b": rows, "resp_loads": resp_loads}
    # correctness on batch 0 (also the warm-up of every arm), and the line-decided share
    rows(0)
    torch.cuda.synchronize()
    want = host_verdicts(np.asarray(sh.ids).reshape(-1, 20), sh.index_base, host_tg[0],
                         idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy(), self_id)
    check = {}
    for name in ("resp", "resp_loads"):
        arms[name](0)
        torch.cuda.synchronize()
        check[name] = bool(np.array_equal(far.cpu().numpy(), want))
    os.environ["KAD_RESP_KERNEL"] = "stats"
    resp(0)
    torch.cuda.synchronize()
    del os.environ["KAD_RESP_KERNEL"]
    st = far.cpu().numpy()
    check["stats"] = bool(np.array_equal(st & 1, want))
    decided = float((st >> 7).mean())
    for j in range(args.batches):  # every batch once through every arm
        for fn in arms.values():
            fn(j)
    torch.cuda.synchronize()

    per = {a: [] for a in arms}
    grp = {a: [] for a in arms}
    for rd in range(args.rounds):
        evs = []
        for r in range(args.reps):  # interleaved launch by launch, each with its own events
            for a, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn((rd * args.reps + r) % args.batches)
                e1.record(stream)
                evs.append((a, e0, e1))
        torch.cuda.synchronize()
        for a, e0, e1 in evs:
            per[a].append(e0.elapsed_time(e1) * 1e3)
        for a, fn in arms.items():  # back-to-back groups
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for r in range(args.reps):
                fn(r % args.batches)
            e1.record(stream)
            torch.cuda.synchronize()
            grp[a].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    res = {"queries": args.queries, "count": 8, "min_nodes": 1, "nodes": int(T.n), "launches_per_arm": args.rounds * args.reps,
           "far_share": float(want.mean()), "line_decided_share": decided, "verdicts_equal_rows_plus_compare": check,
           "arms": {a: {"per_launch_us_median": float(np.median(per[a])),
                        "per_launch_us_q25": float(np.percentile(per[a], 25)),
                        "per_launch_us_q75": float(np.percentile(per[a], 75)),
                        "group_us_median": float(np.median(grp[a])), "group_us_min": float(np.min(grp[a]))}
                    for a in arms}}
    m = {a: res["arms"][a]["per_launch_us_median"] for a in arms}
    res["rows_spread_us"] = abs(m["rows_a"] - m["rows_b"])
    res["resp_minus_rows_us"] = m["resp"] - 0.5 * (m["rows_a"] + m["rows_b"])
    res["resp_loads_minus_resp_us"] = m["resp_loads"] - m["resp"]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: res[k] for k in ("rows_spread_us", "resp_minus_rows_us", "resp_loads_minus_resp_us",
                                          "line_decided_share")}))
    T.close()
    if not all(check.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
