"""Timing of the device refill (kad_sr_refill) over a NodeCache table of 1M nodes (10 % expired) and
sets of S live searches with slabs of 32 entries, for S = 1k, 64k and 1M, once with every search listed and once with
one search in 16. A search holds 0..14 nodes that share a prefix with its ID (closer than the cache's nodes, as what a
lookup has already found), so a refill inserts up to 14 cached nodes behind them and pops what exceeds 14 good nodes.

Timed in the same run, medians after a warm-up, the set put back to its first state (kad_searches_patch, not timed)
before every repetition:

    a  refill        kad_sr_refill end to end on host arrays (wall clock: upload of `which`, gather of the search IDs,
                     the count-14 NodeCache batch, the refill kernel, one copy back), and its refill kernel alone
                     (between HIP events, kad_sr_refill_kernel_ms)
    b  old path      what a caller did before for the same searches: upload of the search IDs, kad_nc_closest_batch at
                     count 14, the rows and counts copied to the host, then kad_searches_patch of the same `which`
                     with the final lists, which are precomputed. The host's own insertNode time is left out, so b is a
                     lower bound of the old path
    c  nc floor      the count-14 NodeCache batch alone (between events), device targets

    python tools/refill_bench.py [--sizes 1000,65536,1048576] [--reps 5] [--out profiles/r11/refill/refill_bench.json]
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

from opendht_amd import DeviceSearches, DeviceTable  # noqa: E402

K, CAP = 14, 32


def sorted_ids(n, seed):
    rng = np.random.default_rng(seed)
    ids = np.frombuffer(rng.bytes(20 * n), np.uint8).reshape(n, 20)
    ids = ids[np.lexsort(ids.T[::-1])]
    return np.ascontiguousarray(ids[np.concatenate(([True], (ids[1:] != ids[:-1]).any(axis=1)))])


def make_set(S, seed):
    """ids (S, 20) ascending; CSR lists of 0..14 nodes sharing 4 bytes with their search ID, ascending in distance."""
    rng = np.random.default_rng(seed)
    ids = sorted_ids(S, seed)
    S = ids.shape[0]
    n = rng.integers(0, K + 1, size=S)
    off = np.frombuffer(rng.bytes(20 * K * S), np.uint8).reshape(S, K, 20).copy()
    off[:, :, :4] = 0
    key = off[:, :, 4:12].copy().view(">u8").reshape(S, K)
    off = np.take_along_axis(off, np.argsort(key, axis=1)[:, :, None], axis=1)
    nodes = off ^ ids[:, None, :]
    keep = np.arange(K)[None, :] < n[:, None]
    offs = np.zeros(S + 1, np.uint32)
    offs[1:] = np.cumsum(n)
    return ids, offs, np.ascontiguousarray(nodes[keep])


def csr_of(exp, which):
    """The lists of the searches `which` of an export as CSR arrays for kad_searches_patch."""
    n = exp["n"][which].astype(np.int64)
    keep = np.arange(exp["node_ids"].shape[1])[None, :] < n[:, None]
    off = np.zeros(which.shape[0] + 1, np.uint32)
    off[1:] = np.cumsum(n)
    return (exp["flags"][which].copy(), off, np.ascontiguousarray(exp["node_ids"][which][keep]),
            np.ascontiguousarray(exp["node_flags"][which][keep]))


def med(v):
    return {"median_us": float(np.median(v)), "q25_us": float(np.percentile(v, 25)), "q75_us": float(np.percentile(v, 75)),
            "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    nid = sorted_ids(args.nodes, 0x11A0)
    status = np.where(np.random.default_rng(0x11A1).random(nid.shape[0]) < 0.1, 2, 1).astype(np.uint8)
    NC = DeviceTable(nid, status, device=0, sorted=True)
    res = {"nodecache_nodes": int(nid.shape[0]), "cap": CAP, "sets": {}}
    for S in (int(v) for v in args.sizes.split(",")):
        ids, offs, nodes = make_set(S, 0x11B0 + S)
        S = ids.shape[0]
        flags0, nfl0 = np.zeros(S, np.uint8), np.zeros(nodes.shape[0], np.uint8)
        DS = DeviceSearches(ids, flags0, offs, nodes, nfl0, cap=CAP, device=0)
        everything = np.arange(S, dtype=np.uint32)
        entry = {"S": S}
        for name, which in (("all", everything), ("one_in_16", everything[::16].copy())):
            m = which.shape[0]
            restore = lambda: DS.patch(everything, flags0, offs, nodes, nfl0)  # noqa: E731
            a_wall, a_kernel, b_wall, c_nc = [], [], [], []
            final = None
            tg_host = np.ascontiguousarray(ids[which])
            for rep in range(args.reps + 1):
                restore()
                t0 = time.perf_counter()
                rows, cnt, ins, st = DS.refill(NC, which)
                t1 = time.perf_counter()
                if rep:
                    a_wall.append((t1 - t0) * 1e6)
                    a_kernel.append(DS.refill_kernel_ms * 1e3)
                if final is None:
                    final = csr_of(DS.export(), which)
                    dirty = int(((ins != 0) | (st != 0)).sum())
                    entry_stats = {"m": m, "inserts": int(sum(bin(int(v)).count("1") for v in ins)),
                                   "searches_with_inserts": int((ins != 0).sum()), "overflowed": int(st.sum()),
                                   "rows_short": int((cnt < K).sum()), "changed_or_overflowed": dirty}
                restore()
                t0 = time.perf_counter()
                tg = torch.from_numpy(tg_host).to(dev)
                idx, c = NC.nc_closest(tg, K)
                idx.cpu(), c.cpu()
                DS.patch(which, *final)
                t1 = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                NC.nc_closest(tg, K, out_idx=idx, out_cnt=c)
                e1.record(stream)
                torch.cuda.synchronize()
                if rep:
                    b_wall.append((t1 - t0) * 1e6)
                    c_nc.append(e0.elapsed_time(e1) * 1e3)
            a, b = med(a_wall), med(b_wall)
            entry[name] = dict(entry_stats, a_refill_end_to_end=a, a_refill_kernel=med(a_kernel), b_old_path_lower_bound=b,
                               c_nc_batch_count14=med(c_nc), a_beats_b=bool(a["median_us"] < b["median_us"]),
                               b_over_a=b["median_us"] / a["median_us"])
        # the refill kernel's traffic per listed search: record and slab read, the 14 gathered IDs and the row, and for
        # a search that changed the slab and record written back
        entry["kernel_bytes_per_search"] = {"read": 64 + CAP * 21 + K * 20 + K * 4 + 4 + 1, "written_if_changed": 64 + CAP * 21,
                                            "outputs": 3}
        res["sets"][str(S)] = entry
        DS.close()
    NC.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
