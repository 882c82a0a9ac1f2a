"""Timing of a whole trySearchInsert tick in one call (kad_sr_try_insert_tick) against the same tick
driven from the host with the calls that existed before it, on the same sets and candidates, slabs of 32 entries.

Sets: S live, full searches, each holding what the 14 closest of 300 x S random nodes look like (the steady recipe of
tests/test_search_ingest.py at any S: the k-th member's distance is the k-th order statistic of that population).
Candidates: `steady`, 5000 and 100000 new random IDs, of which a handful is accepted; `adversarial`, 20000 candidates
aimed at 8192 searches (closer than every member, so each is accepted by its search and refused by the neighbours,
several per search and one in ten a repeat of an earlier one): candidates of one search meet, so the tick takes as many
rounds as the busiest search has candidates.

Timed in the same run, medians after a warm-up, the touched searches put back (kad_searches_patch, not timed) before
every repetition:

    a  tick          kad_sr_try_insert_tick end to end on host arrays (wall clock around the synchronous call), with the
                     device time of its verdict kernels and of its gather and insert kernels (kad_sr_tick_stats)
    b  parent path   per round kad_sr_try_insert_batch_host on the remaining candidates, kad_searches_export without the
                     slabs (the records of all S searches, to derive the trim bits), kad_sr_plan_round, and kad_sr_insert
                     of the ready pairs with their IDs uploaded again. The plan is the engine's in both, so the difference
                     is the data path

Neither includes the host's replay on its own lists, which is the same for both. The bytes that cross the bus per round
are worked out from the counts: a: 4 r up (from round 2) and 16 r down for r remaining candidates, 8 p up and 2 p down for
p pairs, and 21 q up once; b: 20 r up and 13 r down, 64 S down, 29 p up and 2 p down.

    python tools/sr_tick_bench.py [--sizes 1000,65536,1048576] [--reps 5] [--out profiles/r15/sr_tick/tick_bench.json]

--out adds its sets to a file that exists, so the sizes can run one per process."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opendht_amd import KAD_SR_TICK_APPLIED, DeviceSearches, plan_round  # noqa: E402

K, CAP = 14, 32
ADVERSARIAL = (65536, 20000, 8192)  # set size, candidates, searches aimed at


def sorted_ids(n, seed):
    rng = np.random.default_rng(seed)
    ids = np.frombuffer(rng.bytes(20 * n), np.uint8).reshape(n, 20)
    ids = ids[np.lexsort(ids.T[::-1])]
    return np.ascontiguousarray(ids[np.concatenate(([True], (ids[1:] != ids[:-1]).any(axis=1)))])


def make_set(S, seed):
    """ids (S, 20) ascending; every search holds 14 nodes at the distances of the 14 closest of 300 S random nodes."""
    rng = np.random.default_rng(seed)
    ids = sorted_ids(S, seed)
    S = ids.shape[0]
    frac = np.cumsum(rng.exponential(size=(S, K)), axis=1) / (300.0 * S)  # ascending fractions of the ID space
    top = np.minimum(frac * 2.0 ** 64, 2.0 ** 63).astype(np.uint64) + np.uint64(1 << 20)
    top += np.arange(K, dtype=np.uint64)[None, :]  # strictly ascending whatever the rounding did
    d = np.frombuffer(rng.bytes(20 * K * S), np.uint8).reshape(S, K, 20).copy()
    d[:, :, :8] = top.astype(">u8").view(np.uint8).reshape(S, K, 8)
    return ids, np.arange(S + 1, dtype=np.uint32) * K, np.ascontiguousarray((d ^ ids[:, None, :]).reshape(S * K, 20))


def adversarial_cands(ids, q, aimed, seed):
    """q candidates for `aimed` of the searches: the search ID with its last 6 bytes random (closer than every member,
    whose distance is at least 2^116), one in ten a repeat."""
    rng = np.random.default_rng(seed)
    at = rng.choice(ids.shape[0], size=aimed, replace=False)[rng.integers(0, aimed, size=q)]
    c = ids[at].copy()
    c[:, 14:] = np.frombuffer(rng.bytes(6 * q), np.uint8).reshape(q, 6)
    rep = np.flatnonzero(rng.random(q) < 0.1)
    rep = rep[rep > 0]
    c[rep] = c[(rng.random(rep.shape[0]) * rep).astype(np.int64)]
    return np.ascontiguousarray(c)


def med(v):
    return {"median_us": float(np.median(v)), "q25_us": float(np.percentile(v, 25)), "q75_us": float(np.percentile(v, 75)),
            "reps": len(v)}


def reset(DS, touched, offs, nodes):
    """The searches `touched` back to their 14 first nodes."""
    w = np.unique(np.asarray(touched, np.uint32))
    if w.shape[0] == 0:
        return
    rows = (w[:, None].astype(np.int64) * K + np.arange(K)[None, :]).reshape(-1)
    DS.patch(w, np.zeros(w.shape[0], np.uint8), np.arange(w.shape[0] + 1, dtype=np.uint32) * K, nodes[rows],
             np.zeros(rows.shape[0], np.uint8))


def run_tick(DS, cand):
    t0 = time.perf_counter()
    r = DS.try_insert_tick(cand)
    wall = (time.perf_counter() - t0) * 1e6
    ap = np.flatnonzero(r["kind"] == KAD_SR_TICK_APPLIED)
    lo = r["lb"][ap].astype(np.int64) - r["back"][ap] - 1
    hi = r["lb"][ap].astype(np.int64) + r["fwd"][ap]
    touched = np.concatenate([np.arange(max(a, 0), min(b, DS.S - 1) + 1) for a, b in zip(lo, hi)]) if ap.shape[0] else []
    q = cand.shape[0]
    rounds = []
    for k in range(1, r["stats"]["rounds"] + 1):
        rem = int(((r["round"] >= k) | (r["kind"] == 0)).sum())
        rounds.append({"remaining": rem, "up": (4 * rem if k > 1 else 0), "down": 16 * rem})
    return wall, r["stats"], touched, {"once_up": 21 * q, "rounds": rounds, "pairs_up": 8 * r["stats"]["pairs"],
                                       "pairs_down": 2 * r["stats"]["pairs"]}


def run_parent(DS, cand):
    """The same tick from the host: verdicts, the export for the trim bits, the engine's plan, kad_sr_insert."""
    S = DS.S
    t0 = time.perf_counter()
    rem = np.arange(cand.shape[0])
    rounds, touched, pairs, applied, skipped = [], [], 0, 0, 0
    while rem.shape[0]:
        ids = cand[rem]
        lb, fwd, back, stop = DS.try_insert_host(ids)
        st = DS.export(nodes=False)
        trims = (st["full"] != 0) & (st["t"] < st["n"])
        fs, bs = stop & 15, stop >> 4
        l, f, b = lb.astype(np.int64), fwd.astype(np.int64), back.astype(np.int64)
        trim = ((fs >= 2) & trims[np.minimum(l + f, S - 1)]).astype(np.uint8) | \
               (((bs >= 2) & trims[np.maximum(l - b - 1, 0)]).astype(np.uint8) << 1)
        kind, pw, pc, want = plan_round(S, lb, fwd, back, stop, trim)
        if pw.shape[0]:
            ins, status = DS.insert(pw, np.arange(pw.shape[0] + 1, dtype=np.uint32), ids[pc])
            if status.any() or not np.array_equal(ins, want):
                raise RuntimeError("parent path: a result byte against the plan")
            touched.append(pw)
        rounds.append({"remaining": int(rem.shape[0]), "up": 20 * int(rem.shape[0]) + 29 * int(pw.shape[0]),
                       "down": 13 * int(rem.shape[0]) + 64 * S + 2 * int(pw.shape[0])})
        pairs += int(pw.shape[0])
        applied += int((kind == 1).sum())
        skipped += int((kind == 0).sum())
        rem = rem[kind == 2]
    wall = (time.perf_counter() - t0) * 1e6
    return wall, {"rounds": len(rounds), "pairs": pairs, "applied": applied, "skipped": skipped}, \
        (np.concatenate(touched) if touched else []), rounds


def bench(DS, cand, offs, nodes, reps):
    a_wall, a_ver, a_ins, b_wall = [], [], [], []
    a_stats = a_bytes = b_stats = b_rounds = None
    for rep in range(reps + 1):
        wall, a_stats, touched, a_bytes = run_tick(DS, cand)
        reset(DS, touched, offs, nodes)
        if rep:
            a_wall.append(wall)
            a_ver.append(a_stats["verdict_ms"] * 1e3)
            a_ins.append(a_stats["insert_ms"] * 1e3)
        wall, b_stats, touched, b_rounds = run_parent(DS, cand)
        reset(DS, touched, offs, nodes)
        if rep:
            b_wall.append(wall)
    same = all(a_stats[k] == b_stats[k] for k in ("rounds", "pairs", "applied", "skipped"))
    a, b = med(a_wall), med(b_wall)
    a_total = a_bytes["once_up"] + a_bytes["pairs_up"] + a_bytes["pairs_down"] + sum(r["up"] + r["down"] for r in a_bytes["rounds"])
    b_total = sum(r["up"] + r["down"] for r in b_rounds)
    return {"candidates": int(cand.shape[0]), "rounds": a_stats["rounds"], "pairs": a_stats["pairs"],
            "applied": a_stats["applied"], "skipped": a_stats["skipped"], "same_counts_both_paths": bool(same),
            "a_tick_end_to_end": a, "a_verdict_kernels": med(a_ver), "a_insert_kernels": med(a_ins),
            "b_parent_path": b, "a_beats_b": bool(a["median_us"] < b["median_us"]), "b_over_a": b["median_us"] / a["median_us"],
            "a_bus_bytes": a_total, "b_bus_bytes": b_total,
            "a_round_bytes": [r["up"] + r["down"] for r in a_bytes["rounds"]][:12],
            "b_round_bytes": [r["up"] + r["down"] for r in b_rounds][:12]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sr_tick_bench needs a GPU")
    res = {"cap": CAP, "sets": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    for S0 in (int(v) for v in args.sizes.split(",")):
        ids, offs, nodes = make_set(S0, 0x15B0 + S0)
        S = ids.shape[0]
        DS = DeviceSearches(ids, np.zeros(S, np.uint8), offs, nodes, np.zeros(nodes.shape[0], np.uint8), cap=CAP, device=0)
        entry = {"S": S}
        for q in (5000, 100000):
            rng = np.random.default_rng(0x15C0 + q)
            cand = np.frombuffer(rng.bytes(20 * q), np.uint8).reshape(q, 20).copy()
            entry[f"steady_q{q}"] = bench(DS, cand, offs, nodes, args.reps)
        if S0 == ADVERSARIAL[0]:
            entry[f"adversarial_q{ADVERSARIAL[1]}"] = bench(DS, adversarial_cands(ids, ADVERSARIAL[1], ADVERSARIAL[2], 0x15D0),
                                                            offs, nodes, args.reps)
        res["sets"][str(S0)] = entry
        DS.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
