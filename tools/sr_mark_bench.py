"""Timing of the device node-status marking (kad_sr_mark_nodes) over sets of S live, full searches
(14 good nodes each plus one far node that every group of 16 consecutive searches shares, slabs of 32 entries) for
S = 1k, 64k and 1M, with q = 1, 1024 and 65536 changed nodes that one search holds each, and one run per set with nodes
that 16 searches hold each. The op sets KAD_SN_BAD, which takes a full search below 14 good nodes.

Timed in the same run, medians of --reps after a warm-up, the set put back to its first state (a mark that clears the
bit again, not timed) before every repetition of a:

    a  mark          kad_sr_mark_nodes end to end on host arrays (wall clock around the synchronous call: the sort, one
                     upload, three kernels, one copy back, the sort of the changed list), and its scan and fix kernels
                     alone (between HIP events, kad_sr_mark_kernel_ms)
    b  old path      what a caller did before for the same change: kad_searches_patch of exactly the changed searches
                     with their final lists, which are precomputed. A lower bound: the host's search for the holders is
                     not in it. That search is reported apart, as a numpy scan (np.isin over the keys) of the exported
                     member IDs
    c  floor         a torch sum over S x cap x 8 bytes, the bytes of the member keys the scan kernel streams

    python tools/sr_mark_bench.py [--sizes 1000,65536,1048576] [--reps 5] [--out profiles/r14/sr_mark/mark_bench.json]
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

from opendht_amd import KAD_SN_BAD, DeviceSearches  # noqa: E402

K, CAP, GROUP = 14, 32, 16


def sorted_ids(n, seed):
    rng = np.random.default_rng(seed)
    ids = np.frombuffer(rng.bytes(20 * n), np.uint8).reshape(n, 20)
    ids = ids[np.lexsort(ids.T[::-1])]
    return np.ascontiguousarray(ids[np.concatenate(([True], (ids[1:] != ids[:-1]).any(axis=1)))])


def make_set(S, seed):
    """ids (S, 20) ascending; every search holds 14 nodes sharing 4 bytes with its ID, ascending in distance, and as its
    15th and farthest entry the node its group of 16 consecutive searches shares. Returns ids, off, nodes (S, 15, 20),
    shared (groups, 20)."""
    rng = np.random.default_rng(seed)
    ids = sorted_ids(S, seed)
    S = ids.shape[0]
    d = np.frombuffer(rng.bytes(20 * K * S), np.uint8).reshape(S, K, 20).copy()
    d[:, :, :4] = 0
    key = d[:, :, 4:12].copy().view(">u8").reshape(S, K)
    d = np.take_along_axis(d, np.argsort(key, axis=1)[:, :, None], axis=1)
    groups = (S + GROUP - 1) // GROUP
    shared = np.frombuffer(rng.bytes(20 * groups), np.uint8).reshape(groups, 20).copy()
    shared[:, 0] = ids[::GROUP, 0] ^ 0x80  # differs from every search of the group in the first bit: the farthest entry
    nodes = np.concatenate([d ^ ids[:, None, :], shared[np.arange(S) // GROUP][:, None, :]], axis=1)
    return ids, np.arange(S + 1, dtype=np.uint32) * (K + 1), np.ascontiguousarray(nodes), shared


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


def floor_sum(S, reps):
    """c: a torch sum over the bytes of the member keys, between events."""
    x = torch.randint(0, 1 << 40, (S * CAP,), dtype=torch.int64, device="cuda")
    out = []
    for rep in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        x.sum()
        b.record()
        torch.cuda.synchronize()
        if rep >= 2:
            out.append(a.elapsed_time(b) * 1e3)
    return med(out)


def holder_scan(exp, batch, reps):
    """The host's search for the holders on the parent commit's path: which searches hold a node whose key is in the
    batch (a key match is then confirmed on the 12-byte tail, which is not timed)."""
    keys = np.ascontiguousarray(exp["node_ids"][:, :, :8]).view(">u8").reshape(exp["node_ids"].shape[:2]).astype(np.uint64)
    bkeys = np.ascontiguousarray(batch[:, :8]).view(">u8").reshape(-1).astype(np.uint64)
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        hit = np.isin(keys, bkeys).any(axis=1)
        out.append((time.perf_counter() - t0) * 1e6)
    return med(out), int(hit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sr_mark_bench needs a GPU")
    res = {"cap": CAP, "sets": {}}
    for S in (int(v) for v in args.sizes.split(",")):
        ids, offs, nodes, shared = make_set(S, 0x14B0 + S)
        S = ids.shape[0]
        DS = DeviceSearches(ids, np.zeros(S, np.uint8), offs, nodes.reshape(-1, 20), np.zeros(S * (K + 1), np.uint8),
                            cap=CAP, device=0)
        rng = np.random.default_rng(0x14C0 + S)
        entry = {"S": S, "c_torch_sum_of_key_bytes": floor_sum(S, args.reps), "key_bytes": S * CAP * 8}
        # (q asked for, held by 16); the run is named by the q it ends up with
        for q, many in [(q, False) for q in (1, 1024, 65536)] + [(65536, True)]:
            if many:
                q = min(q, shared.shape[0])
                batch = np.ascontiguousarray(shared[rng.choice(shared.shape[0], size=q, replace=False)])
            else:  # members of distinct entries; a set too small for q distinct searches gives several per search
                q = min(q, S * K)
                e = rng.choice(S * K, size=q, replace=False)
                batch = np.ascontiguousarray(nodes[e // K, e % K])
            name = f"q{q}_held_by_{GROUP if many else 1}"
            setb = np.full(q, KAD_SN_BAD, np.uint8)
            a_wall, a_scan, a_fix, b_wall = [], [], [], []
            final = stats = None
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                r = DS.mark_nodes(batch, None, setb)
                t1 = time.perf_counter()
                if rep:
                    a_wall.append((t1 - t0) * 1e6)
                    scan_ms, fix_ms = DS.mark_kernel_ms()
                    a_scan.append(scan_ms * 1e3)
                    a_fix.append(fix_ms * 1e3)
                if final is None:
                    exp = DS.export()
                    final = csr_of(exp, r["changed"])
                    scan, holders = holder_scan(exp, batch, 3)
                    stats = {"q": int(q), "hits": int(r["hits"].sum()), "changed": int(r["changed"].shape[0]),
                             "lds_batch": bool(q <= 4096), "b_host_holder_scan_numpy": scan, "holders_by_key": holders}
                    del exp
                t0 = time.perf_counter()
                DS.patch(r["changed"], *final)  # writes the same final lists whatever the set holds
                t1 = time.perf_counter()
                if rep:
                    b_wall.append((t1 - t0) * 1e6)
                back = DS.mark_nodes(batch, setb, None)  # the first state again, not timed
                assert back["changed"].shape[0] == r["changed"].shape[0]
            a, b, sc = med(a_wall), med(b_wall), med(a_scan)
            entry[name] = dict(stats, a_mark_end_to_end=a, a_scan_kernel=sc, a_fix_kernel=med(a_fix),
                               b_patch_lower_bound=b, b_over_a=b["median_us"] / a["median_us"],
                               scan_over_c=sc["median_us"] / entry["c_torch_sum_of_key_bytes"]["median_us"])
        res["sets"][str(S)] = entry
        DS.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
