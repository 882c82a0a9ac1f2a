"""Timing of Dht::searchStep's decision over a device set of live searches (kad_sr_step) against the path
that gave the same answer before it existed, on the same sets, slabs of 32 entries.

Sets: the steady lists of tools/sr_tick_bench.py (S live searches of 14 nodes each) with step bits drawn per entry: 40 %
synced and answered (SYNCED | NOGET), 20 % with a request in flight (PENDING | NOGET), 10 % answered long ago (NOGET), 30 %
never asked; one search in 100 has only bad nodes and expires.

Timed, medians after a warm-up, one process per size:

    all_verdict   DS.step() over every search, nothing written
    all_apply     DS.step(None, KAD_STEP_APPLY): sends and expiries written in place; the set is created again (not timed)
                  before every repetition
    listed        one search in 16, listed in `which`, verdict mode

each end to end (wall clock around the synchronous call on host arrays) and as the kernel time between the call's two
events (kad_sr_step_stats). The parent path, for the same answer: kad_searches_export of the search flags, n and the flag
bytes; the closed form in numpy over the (S, cap) flag matrix; for all_apply also kad_searches_patch of every search that
changed, lists and node IDs uploaded again. Its answer is compared with the device's once per run. Beside the kernel: a
torch sum over a device tensor of as many bytes as the flag bytes and records it reads, between two events.

    python tools/sr_step_bench.py [--sizes 1000,65536,1048576] [--reps 5] [--out profiles/r16/sr_step/step_bench.json]

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from opendht_amd import (KAD_SN_BAD, KAD_SN_CANDIDATE, KAD_SN_NOGET, KAD_SN_PENDING, KAD_SN_SYNCED, KAD_STEP_APPLY,  # noqa: E402
                         KAD_STEP_EXHAUSTED, KAD_STEP_EXPIRE, KAD_STEP_SHORT, KAD_STEP_SYNCED, DeviceSearches)
from opendht_amd._lib import check, lib, ptr  # noqa: E402
from sr_tick_bench import CAP, K, make_set, med  # noqa: E402


def make_flags(S, seed):
    rng = np.random.default_rng(seed)
    kinds = np.array([0, KAD_SN_SYNCED | KAD_SN_NOGET, KAD_SN_PENDING | KAD_SN_NOGET, KAD_SN_NOGET], np.uint8)
    fl = kinds[rng.choice(4, size=(S, K), p=[.3, .4, .2, .1])]
    fl[rng.random(S) < 0.01] = KAD_SN_BAD
    return np.ascontiguousarray(fl.reshape(-1))


def export_flags(DS):
    S, cap = DS.S, DS.cap
    sf, n, fl = np.zeros(S, np.uint8), np.zeros(S, np.uint32), np.zeros((S, cap), np.uint8)
    check(lib().kad_searches_export(DS._h, None, ptr(sf), ptr(n), None, ptr(fl), None, None), "kad_searches_export")
    return sf, n, fl


def numpy_step(sf, n, fl):
    """The closed form of kad_step.h over the (m, cap) flag matrix: picks as a boolean matrix, solicited, bits."""
    m, cap = fl.shape
    valid = np.arange(cap)[None, :] < n[:, None]
    badb = (fl & KAD_SN_BAD) != 0
    bad, good = badb & valid, ~badb & valid
    pend, sync, noget, cand = ((fl & b) != 0 for b in (KAD_SN_PENDING, KAD_SN_SYNCED, KAD_SN_NOGET, KAD_SN_CANDIDATE))
    n_bad, lead = bad.sum(1), np.cumprod(bad, axis=1).sum(1)
    sol = (good & pend).sum(1)
    live = (sf & 1) == 0
    first8 = good & (np.cumsum(good, axis=1) <= 8)
    synced = live & good.any(1) & ~(first8 & ~sync).any(1)
    gettable = ~noget & (~badb | cand) & valid
    gg = gettable & good & ~pend
    room = 4 - sol
    before = np.cumsum(gg, axis=1) - gg
    sending = live & (sol < 4)
    exhausted = sending & (gg.sum(1) < room)
    picks = gettable & sending[:, None] & (exhausted[:, None] | (before < room[:, None]))
    sol = sol + (picks & gg).sum(1)
    expire = live & (lead >= np.minimum(n, 25))
    bits = np.where(live, 0, 1) | np.where(live & (n - n_bad < 14), KAD_STEP_SHORT, 0) | np.where(synced, KAD_STEP_SYNCED, 0) | \
        np.where(exhausted, KAD_STEP_EXHAUSTED, 0) | np.where(expire, KAD_STEP_EXPIRE, 0)
    return picks, sol, bits.astype(np.uint32)


def mask_of(picks):
    return (picks.astype(np.uint64) << np.arange(picks.shape[1], dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)


def parent(DS, nodes, which, apply):
    """Export, the closed form, and (apply) the patch of every search that changed. Returns (picks mask, bits)."""
    sf, n, fl = export_flags(DS)
    if which is not None:
        sf, n, fl = sf[which], n[which], fl[which]
    picks, _, bits = numpy_step(sf, n, fl)
    if apply:
        gone = (bits & KAD_STEP_EXPIRE) != 0
        w = np.flatnonzero(gone | picks.any(1)).astype(np.uint32)
        new = np.where(picks[w], fl[w] | KAD_SN_PENDING | KAD_SN_NOGET, fl[w])
        keep = (np.arange(fl.shape[1])[None, :] < n[w][:, None]) & ~gone[w][:, None]
        off = np.zeros(w.shape[0] + 1, np.uint32)
        off[1:] = np.cumsum(keep.sum(1))
        ids = nodes.reshape(-1, K, 20)[w][keep[:, :K]]
        DS.patch(w, gone[w].astype(np.uint8), off, np.ascontiguousarray(ids), np.ascontiguousarray(new[keep]))
    return mask_of(picks), bits


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e6, r


def torch_sum_us(nbytes, reps):
    t = torch.ones(nbytes, dtype=torch.uint8, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for rep in range(reps + 1):
        a.record()
        t.sum()
        b.record()
        torch.cuda.synchronize()
        if rep:
            out.append(a.elapsed_time(b) * 1e3)
    return med(out)


def bench_set(S0, reps):
    ids, offs, nodes = make_set(S0, 0x15B0 + S0)
    S = ids.shape[0]
    flags = make_flags(S, 0x16A0 + S0)

    def create():
        return DeviceSearches(ids, np.zeros(S, np.uint8), offs, nodes, flags, cap=CAP, device=0)

    entry = {"S": S}
    which = np.arange(0, S, 16, dtype=np.uint32)
    DS = create()
    for name, w in (("all_verdict", None), ("listed", which)):
        wall, kern, pwall = [], [], []
        for rep in range(reps + 1):
            us, r = timed(lambda: DS.step(w))
            pus, (pm, pb) = timed(lambda: parent(DS, nodes, w, False))
            if rep == 0:
                assert np.array_equal(r["picks"], pm) and np.array_equal(r["bits"], pb), name
            else:
                wall.append(us)
                kern.append(r["stats"]["kernel_ms"] * 1e3)
                pwall.append(pus)
        a, b = med(wall), med(pwall)
        entry[name] = {"searches": int(S if w is None else w.shape[0]), "picks": int(r["stats"]["picks"]),
                       "synced": int(r["stats"]["synced"]), "expire": int(r["stats"]["expired"]),
                       "step_end_to_end": a, "step_kernel": med(kern), "parent_path": b,
                       "step_beats_parent": bool(a["median_us"] < b["median_us"]), "parent_over_step": b["median_us"] / a["median_us"]}
    DS.close()
    wall, kern, pwall = [], [], []
    for rep in range(reps + 1):
        DS = create()
        us, r = timed(lambda: DS.step(None, KAD_STEP_APPLY))
        after = DS.export() if rep == 0 else None
        DS.close()
        DS = create()
        pus, (pm, pb) = timed(lambda: parent(DS, nodes, None, True))
        if rep == 0:
            assert np.array_equal(r["picks"], pm) and np.array_equal(r["bits"], pb), "all_apply"
            twin = DS.export()
            assert all(np.array_equal(after[k], twin[k]) for k in after), "all_apply: the two paths leave different sets"
        else:
            wall.append(us)
            kern.append(r["stats"]["kernel_ms"] * 1e3)
            pwall.append(pus)
        DS.close()
    a, b = med(wall), med(pwall)
    entry["all_apply"] = {"searches": S, "picks": int(r["stats"]["picks"]), "expire": int(r["stats"]["expired"]),
                          "changed_searches": int(((pm != 0) | ((pb & KAD_STEP_EXPIRE) != 0)).sum()),
                          "step_end_to_end": a, "step_kernel": med(kern), "parent_path": b,
                          "step_beats_parent": bool(a["median_us"] < b["median_us"]), "parent_over_step": b["median_us"] / a["median_us"]}
    entry["torch_sum_bytes"] = S * (CAP + 64)  # every flag byte and record of the set
    entry["torch_sum_same_bytes"] = torch_sum_us(S * (CAP + 64), reps)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sr_step_bench needs a GPU")
    res = {"cap": CAP, "sets": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    for S0 in (int(v) for v in args.sizes.split(",")):
        res["sets"][str(S0)] = bench_set(S0, args.reps)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
