"""Timing of the device insertNode (kad_sr_insert) over sets of S live, full searches (14 good nodes
each, slabs of 32 entries) for S = 1k, 64k and 1M, once with every search listed and once with one search in 16, with 1
and 8 accepted candidates per listed search. A candidate shares one byte more with its search's ID than the members do,
so it enters the list and the last entry is popped.

Timed in the same run, medians after a warm-up, the set put back to its first state (kad_searches_patch, not timed)
before every repetition of a:

    a  insert        kad_sr_insert end to end on host arrays (wall clock around the synchronous call: one upload of
                     which, off, IDs and flags, the insert kernel, one copy back), and its insert kernel alone (between
                     HIP events, kad_sr_insert_kernel_ms)
    b  old path      what a caller did before for the same searches: kad_searches_patch of the same `which` with the
                     final lists, which are precomputed. The host's own insertNode time is left out, so b is a lower
                     bound of the old path

and one tick of the steady shape of tests/test_search_ingest.py (200 searches, 5000 candidates) through
try_search_insert and through try_search_insert_device, host double included: both are bound by Python.

    python tools/sr_insert_bench.py [--sizes 1000,65536,1048576] [--reps 5] [--out profiles/r13/sr_insert/insert_bench.json]
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

from opendht_amd import DeviceSearches, try_search_insert, try_search_insert_device  # noqa: E402

K, CAP = 14, 32


def sorted_ids(n, seed):
    rng = np.random.default_rng(seed)
    ids = np.frombuffer(rng.bytes(20 * n), np.uint8).reshape(n, 20)
    ids = ids[np.lexsort(ids.T[::-1])]
    return np.ascontiguousarray(ids[np.concatenate(([True], (ids[1:] != ids[:-1]).any(axis=1)))])


def make_set(S, seed):
    """ids (S, 20) ascending; every search holds 14 nodes sharing 4 bytes with its ID, ascending in distance."""
    rng = np.random.default_rng(seed)
    ids = sorted_ids(S, seed)
    S = ids.shape[0]
    d = np.frombuffer(rng.bytes(20 * K * S), np.uint8).reshape(S, K, 20).copy()
    d[:, :, :4] = 0
    d[:, :, 4] |= 1  # never as close as a candidate
    key = d[:, :, 4:12].copy().view(">u8").reshape(S, K)
    d = np.take_along_axis(d, np.argsort(key, axis=1)[:, :, None], axis=1)
    return ids, np.arange(S + 1, dtype=np.uint32) * K, np.ascontiguousarray((d ^ ids[:, None, :]).reshape(S * K, 20))


def make_cands(ids, which, k, seed):
    """k candidates per listed search sharing 5 bytes with its ID: closer than every member."""
    rng = np.random.default_rng(seed)
    m = which.shape[0]
    d = np.frombuffer(rng.bytes(20 * k * m), np.uint8).reshape(m, k, 20).copy()
    d[:, :, :5] = 0
    return np.arange(m + 1, dtype=np.uint32) * k, np.ascontiguousarray((d ^ ids[which][:, None, :]).reshape(m * k, 20))


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


def tick(reps):
    """One steady tick through both schemes, fresh searches and a fresh device set each time."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import insert_ref as I
    import refill_ref as F
    import searches_ref as R
    import test_search_ingest as T

    out = {"searches": 200, "candidates": 5000}
    for name in ("try_search_insert", "try_search_insert_device"):
        wall, counts = [], None
        for rep in range(reps + 1):
            searches, cands = T.steady()
            ids = R.id_bytes([c.id for c in cands])
            with DeviceSearches(*F.snapshot(searches, T.NOW), cap=CAP, device=0) as DS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "try_search_insert":
                    counts = try_search_insert(DS, R.HostSearches(searches, cands, T.NOW), ids)
                else:
                    counts = try_search_insert_device(DS, I.HostInsert(searches, cands, T.NOW), ids, T.NOW)
                torch.cuda.synchronize()
                if rep:
                    wall.append((time.perf_counter() - t0) * 1e6)
        out[name] = dict(med(wall), counts={k: int(v) for k, v in counts.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sr_insert_bench needs a GPU")
    res = {"cap": CAP, "sets": {}}
    for S in (int(v) for v in args.sizes.split(",")):
        ids, offs, nodes = make_set(S, 0x13B0 + S)
        S = ids.shape[0]
        flags0, nfl0 = np.zeros(S, np.uint8), np.zeros(nodes.shape[0], np.uint8)
        DS = DeviceSearches(ids, flags0, offs, nodes, nfl0, cap=CAP, device=0)
        everything = np.arange(S, dtype=np.uint32)
        entry = {"S": S}
        for name, which in (("all", everything), ("one_in_16", everything[::16].copy())):
            for k in (1, 8):
                coff, cids = make_cands(ids, which, k, 0x13C0 + k)
                a_wall, a_kernel, b_wall = [], [], []
                final = stats = None
                for rep in range(args.reps + 1):
                    DS.patch(everything, flags0, offs, nodes, nfl0)  # the first state again, not timed
                    t0 = time.perf_counter()
                    ins, st = DS.insert(which, coff, cids)
                    t1 = time.perf_counter()
                    if rep:
                        a_wall.append((t1 - t0) * 1e6)
                        a_kernel.append(DS.insert_kernel_ms() * 1e3)
                    if final is None:
                        final = csr_of(DS.export(), which)
                        stats = {"m": int(which.shape[0]), "candidates": int(cids.shape[0]), "accepted": int(ins.sum()),
                                 "overflowed": int(st.sum())}
                    t0 = time.perf_counter()
                    DS.patch(which, *final)  # writes the same final lists whatever the set holds
                    t1 = time.perf_counter()
                    if rep:
                        b_wall.append((t1 - t0) * 1e6)
                a, b = med(a_wall), med(b_wall)
                entry[f"{name}_k{k}"] = dict(stats, a_insert_end_to_end=a, a_insert_kernel=med(a_kernel),
                                             b_patch_lower_bound=b, a_beats_b=bool(a["median_us"] < b["median_us"]),
                                             b_over_a=b["median_us"] / a["median_us"])
        # the insert kernel's traffic per listed search with k candidates: record and slab read, which, two offsets, the
        # candidates; the slab and record written back where the list changed; k result bytes and one status
        entry["kernel_bytes_per_search"] = {"read": 64 + CAP * 21 + 12, "read_per_candidate": 21,
                                            "written_if_changed": 64 + CAP * 21, "written_per_candidate": 1, "status": 1}
        res["sets"][str(S)] = entry
        DS.close()
    res["steady_tick"] = tick(3)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
