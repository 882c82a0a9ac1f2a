"""Timing of the trySearchInsert verdicts (kad_sr_try_insert_batch): 1M candidates per launch over
sets of S synced searches (live, full, each holding 14 good nodes that share a prefix with its ID, as the 14 closest
of a large network do), for S = 1k, 64k and 1M. The prefix is 3 bytes, 4 for S > 64k: at least 8 bits longer than what
a random candidate shares with its nearest search ID, so that a random candidate is refused (a network with as few
nodes per live search as a shorter prefix stands for would accept most candidates somewhere).

    steady     random candidates: both neighbours refuse nearly every one as too far
    accept10   10 % of the candidates lie next to a search ID and are accepted by that search

Beside it, on the same machine:

    find_bucket  kad_rt_find_bucket_batch on 1M random targets over a split-policy table of 1M nodes: one locate per
                 candidate, the nearest existing kernel
    host16       the refusing part of the walk on the host over the same set and candidates, 16 threads: numpy lower
                 bound and threshold compare of both neighbours on the 64-bit keys per chunk. Probes that pass the
                 threshold are counted, their member scan and the walk beyond are not run: a lower bound of the
                 host's cost, and not the reference's C++ loop

Every launch has its own pair of events and its own candidate batch; the figure is the median over the launches of an
arm, with the quartiles.

    python tools/searches_bench.py [--sizes 1000,65536,1048576] [--launches 40] [--out profiles/r09/searches/searches_bench.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opendht_amd import DeviceSearches, DeviceTable  # noqa: E402
from opendht_amd import synth as SY  # noqa: E402

K = 14


def share_bytes(S):
    return 3 if S <= 65536 else 4


def make_set(S, seed):
    """ids (S, 20) ascending, node_ids (S * 14, 20) ascending in distance per search, as uint8 arrays."""
    rng = np.random.default_rng(seed)
    ids = np.frombuffer(rng.bytes(20 * S), np.uint8).reshape(S, 20)
    ids = ids[np.lexsort(ids.T[::-1])]
    ids = ids[np.concatenate(([True], (ids[1:] != ids[:-1]).any(axis=1)))]
    S = ids.shape[0]
    off = np.frombuffer(rng.bytes(20 * K * S), np.uint8).reshape(S, K, 20).copy()
    sh = share_bytes(S)
    off[:, :, :sh] = 0
    key = off[:, :, sh:sh + 8].copy().view(">u8").reshape(S, K)  # the offset is the distance: order by its leading bytes
    off = np.take_along_axis(off, np.argsort(key, axis=1)[:, :, None], axis=1)
    nodes = (off ^ ids[:, None, :]).reshape(-1, 20)
    return ids, np.ascontiguousarray(nodes)


def batches(ids, q, n, seed, near):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = np.frombuffer(rng.bytes(20 * q), np.uint8).reshape(q, 20).copy()
        if near:
            pick = np.flatnonzero(rng.random(q) < near)
            sh = share_bytes(ids.shape[0]) + 2  # two bytes more than the members share: inside the threshold
            c[pick, :sh] = ids[rng.integers(0, ids.shape[0], size=pick.size), :sh]
        out.append(c)
    return out


def key64(a):
    return np.ascontiguousarray(a[:, :8]).view(">u8").reshape(-1).astype(np.uint64)


def host16(ids, nodes, cand):
    """(seconds, accepted) of the host restatement on 16 threads."""
    skey, thr = key64(ids), key64(nodes.reshape(ids.shape[0], K, 20)[:, K - 1])
    S = ids.shape[0]

    def chunk(c):
        x = key64(c)
        lb = np.searchsorted(skey, x, side="left")
        acc = 0
        for s in (np.minimum(lb, S - 1), np.maximum(lb, 1) - 1):
            acc += int(((x ^ skey[s]) < (thr[s] ^ skey[s])).sum())  # closer than entry[13] on the key: the slow path
        return acc

    parts = np.array_split(cand, 64)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        acc = sum(ex.map(chunk, parts))
    return time.perf_counter() - t0, acc


def timed(fn, n, stream):
    evs = []
    for j in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn(j)
        e1.record(stream)
        evs.append((e0, e1))
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in evs]
    return {"per_launch_us_median": float(np.median(us)), "per_launch_us_q25": float(np.percentile(us, 25)),
            "per_launch_us_q75": float(np.percentile(us, 75)), "launches": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    q = args.queries
    res = {"queries": q, "sets": {}}

    tid = SY.random_ids(1_000_000, 0x5EA1)
    perm, first, off = SY.split_table(tid)
    tid = np.ascontiguousarray(tid[perm])
    T = DeviceTable(tid, SY.random_status(tid.shape[0], 0x5EA2, 90, 0), first, off, device=0)
    tg = [torch.from_numpy(SY.random_ids(q, 0x5EA3 + j)).to(dev) for j in range(args.batches)]
    fb = torch.empty((q,), dtype=torch.int32, device=dev)
    arm = lambda j: T.find_bucket(tg[j % len(tg)], out=fb, stream=stream.cuda_stream)  # noqa: E731
    timed(arm, len(tg), stream)
    res["find_bucket_1M_node_split_table"] = timed(arm, args.launches, stream)
    T.close()
    del tg

    for S in (int(v) for v in args.sizes.split(",")):
        ids, nodes = make_set(S, 0x5EB0 + S)
        S = ids.shape[0]
        offs = (np.arange(S + 1, dtype=np.uint32) * K).astype(np.uint32)
        DS = DeviceSearches(ids, np.zeros(S, np.uint8), offs, nodes, np.zeros(nodes.shape[0], np.uint8), cap=K, device=0)
        entry = {"S": S, "cap": K, "share_bits": 8 * share_bytes(S), "device_bytes": DS.device_bytes,
                 "lds_keys": S <= 4096}
        out = tuple(torch.empty((q,), dtype=torch.int32, device=dev) for _ in range(3)) + (
            torch.empty((q,), dtype=torch.uint8, device=dev),)
        for mix, near in (("steady", 0.0), ("accept10", 0.1)):
            hb = batches(ids, q, args.batches, 0x5EC0 + S, near)
            db = [torch.from_numpy(b).to(dev) for b in hb]
            arm = lambda j: DS.try_insert(db[j % len(db)], out=out, stream=stream.cuda_stream)  # noqa: E731
            timed(arm, len(db), stream)
            r = timed(arm, args.launches, stream)
            arm(0)
            torch.cuda.synchronize()
            fwd, back, stop = out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy()
            r["batch0"] = {"accepted_candidates": int(((fwd + back) > 0).sum()), "inserts": int(fwd.sum() + back.sum()),
                           "stop_hist_fwd": np.bincount(stop & 15, minlength=4).tolist(),
                           "stop_hist_back": np.bincount(stop >> 4, minlength=4).tolist()}
            if not args.no_host:
                sec, acc = host16(ids, nodes, hb[0])
                r["host16_us"] = sec * 1e6
                r["host16_slow_path_probes"] = acc
            entry[mix] = r
            del db
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
