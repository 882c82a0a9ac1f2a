"""Timing of the whole Dht::searchStep over a device set of live searches (kad_sr_step_full): the listen
requests and announce probes beside the get requests, against the only exact path the parent commit has for searches that
carry a listen() or a put(), on the same sets, slabs of 32 entries.

Sets: the steady sets of tools/sr_step_bench.py (S live searches of 14 nodes each, its step bits per entry, one search in
100 with only bad nodes) with KAD_SN_LISTEN_DUE and KAD_SN_ANNOUNCE_DUE each drawn on about one synced entry in four.
Modes: 60 % of the searches KAD_STEP_LISTEN, 30 % KAD_STEP_ANNOUNCE (half of them with KAD_STEP_PROBE_BLOCKS), 10 % neither.

Timed, medians after a warm-up, one process per size:

    all_verdict   DS.step_full(None, modes) over every search, nothing written
    all_apply     the same with KAD_STEP_APPLY: the three kinds of sends and the expiries written in place; the set is
                  created again (not timed) before every repetition
    listed        one search in 16, listed in `which`, verdict mode

each end to end (wall clock around the synchronous call on host arrays) and as the kernel time between the call's two
events (kad_sr_step_full_stats). The parent path, for the same answer: kad_searches_export of the search flags, n and the
flag bytes; the closed form of kad_step.h's decide_full in numpy over the (S, cap) flag matrix; for all_apply also
kad_searches_patch of every search that changed. Its answer is compared with the device's once per run. Beside them
step_kernel's time on the same set through kad_sr_step with the get-only part of the same modes (the kernel this change
leaves as it is), and the ratio of the two kernel times.

    python tools/sr_stepfull_bench.py [--sizes 1000,65536,1048576] [--reps 5]
                                      [--out profiles/r17/sr_step_full/stepfull_bench.json]

--out adds its sets to a file that exists, so the sizes can run one per process."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from opendht_amd import (KAD_SN_ANNOUNCE_DUE, KAD_SN_BAD, KAD_SN_CANDIDATE, KAD_SN_LISTEN_DUE, KAD_SN_NOGET,  # noqa: E402
                         KAD_SN_PENDING, KAD_SN_SYNCED, KAD_STEP_ANNOUNCE, KAD_STEP_APPLY, KAD_STEP_EXPIRE, KAD_STEP_LISTEN,
                         KAD_STEP_PROBE_BLOCKS, DeviceSearches)
from sr_step_bench import export_flags, make_flags, mask_of, numpy_step, timed  # noqa: E402
from sr_tick_bench import CAP, K, make_set, med  # noqa: E402


def make_full_flags(S, seed):
    rng = np.random.default_rng(seed)
    fl = make_flags(S, seed).reshape(S, K)
    # a search sends listens and probes only when it is synced: in six searches of ten the first eight nodes have replied
    head = rng.random(S) < 0.6
    fl[head, :8] |= np.where((fl[head, :8] & KAD_SN_BAD) == 0, KAD_SN_SYNCED, 0).astype(np.uint8)
    synced = (fl & KAD_SN_SYNCED) != 0
    fl[synced & (rng.random((S, K)) < 0.25)] |= KAD_SN_LISTEN_DUE
    fl[synced & (rng.random((S, K)) < 0.25)] |= KAD_SN_ANNOUNCE_DUE
    return np.ascontiguousarray(fl.reshape(-1))


def make_modes(S, seed):
    kind = np.random.default_rng(seed).random(S)
    return np.where(kind < 0.6, KAD_STEP_LISTEN, np.where(kind < 0.75, KAD_STEP_ANNOUNCE, np.where(
        kind < 0.9, KAD_STEP_ANNOUNCE | KAD_STEP_PROBE_BLOCKS, 0))).astype(np.uint8)


def numpy_step_full(sf, n, fl, mode):
    """decide_full's closed form over the (m, cap) flag matrix: picks, listen, announce as boolean matrices, solicited,
    bits."""
    m, cap = fl.shape
    valid = np.arange(cap)[None, :] < n[:, None]
    good = ((fl & KAD_SN_BAD) == 0) & valid
    sync, cand, ldue, adue = ((fl & b) != 0 for b in (KAD_SN_SYNCED, KAD_SN_CANDIDATE, KAD_SN_LISTEN_DUE, KAD_SN_ANNOUNCE_DUE))
    live = (sf & 1) == 0
    first8 = good & (np.cumsum(good, axis=1) <= 8)
    synced = live & good.any(1) & ~(first8 & ~sync).any(1)
    se = sync & valid
    nc = se & ~cand
    listen = se & ldue & ((np.cumsum(nc, axis=1) - nc) < 4) & (synced & ((mode & KAD_STEP_LISTEN) != 0))[:, None]
    A = se & adue
    c = A & ~cand
    announce = A & ((np.cumsum(c, axis=1) - c) < 8) & (synced & ((mode & KAD_STEP_ANNOUNCE) != 0))[:, None]
    blocks = ((mode & KAD_STEP_PROBE_BLOCKS) != 0)[:, None]
    probed = fl | np.where(announce, KAD_SN_PENDING, 0).astype(np.uint8) | np.where(announce & blocks, KAD_SN_NOGET, 0).astype(np.uint8)
    picks, sol, bits = numpy_step(sf, n, probed)
    return picks, listen, announce, sol, bits, blocks


def parent(DS, nodes, which, modes, apply):
    """Export, the closed form, and (apply) the patch of every search that changed. Returns (picks, listen, announce
    masks, bits)."""
    sf, n, fl = export_flags(DS)
    if which is not None:
        sf, n, fl = sf[which], n[which], fl[which]
    picks, listen, announce, _, bits, blocks = numpy_step_full(sf, n, fl, modes)
    if apply:
        gone = (bits & KAD_STEP_EXPIRE) != 0
        w = np.flatnonzero(gone | picks.any(1) | listen.any(1) | announce.any(1)).astype(np.uint32)
        new = fl[w] | np.where(picks[w] | announce[w], KAD_SN_PENDING, 0).astype(np.uint8) | \
            np.where(picks[w] | (announce[w] & blocks[w]), KAD_SN_NOGET, 0).astype(np.uint8)
        new &= ~(np.where(listen[w], KAD_SN_LISTEN_DUE, 0) | np.where(announce[w], KAD_SN_ANNOUNCE_DUE, 0)).astype(np.uint8)
        keep = (np.arange(fl.shape[1])[None, :] < n[w][:, None]) & ~gone[w][:, None]
        off = np.zeros(w.shape[0] + 1, np.uint32)
        off[1:] = np.cumsum(keep.sum(1))
        ids = nodes.reshape(-1, K, 20)[w][keep[:, :K]]
        DS.patch(w, gone[w].astype(np.uint8), off, np.ascontiguousarray(ids), np.ascontiguousarray(new[keep]))
    return mask_of(picks), mask_of(listen), mask_of(announce), bits


def same(r, p):
    return all(np.array_equal(r[k], v) for k, v in zip(("picks", "listen", "announce", "bits"), p))


def summary(wall, kern, pwall, old_kern, r):
    a, b, kf, ko = med(wall), med(pwall), med(kern), med(old_kern)
    st = r["stats"]
    return {"picks": int(st["picks"]), "listens": int(st["listens"]), "announces": int(st["announces"]),
            "synced": int(st["synced"]), "expire": int(st["expired"]),
            "step_full_end_to_end": a, "step_full_kernel": kf, "parent_path": b, "parent_answers_equal": True,
            "step_full_beats_parent": bool(a["median_us"] < b["median_us"]), "parent_over_step_full": b["median_us"] / a["median_us"],
            "step_kernel_same_set": ko, "step_full_kernel_over_step_kernel": kf["median_us"] / ko["median_us"]}


def bench_set(S0, reps):
    ids, offs, nodes = make_set(S0, 0x15B0 + S0)
    S = ids.shape[0]
    flags = make_full_flags(S, 0x16A0 + S0)
    modes = make_modes(S, 0x17C0 + S0)

    def create():
        return DeviceSearches(ids, np.zeros(S, np.uint8), offs, nodes, flags, cap=CAP, device=0)

    entry = {"S": S, "modes": {"listen": int((modes == KAD_STEP_LISTEN).sum()), "announce": int(((modes & KAD_STEP_ANNOUNCE) != 0).sum()),
                               "neither": int((modes == 0).sum())}}
    which = np.arange(0, S, 16, dtype=np.uint32)
    DS = create()
    for name, w in (("all_verdict", None), ("listed", which)):
        md = modes if w is None else modes[w]
        wall, kern, pwall, old_kern = [], [], [], []
        for rep in range(reps + 1):
            us, r = timed(lambda: DS.step_full(w, md))
            pus, p = timed(lambda: parent(DS, nodes, w, md, False))
            old = DS.step(w, 0)
            if rep == 0:
                assert same(r, p), name
            else:
                wall.append(us)
                kern.append(r["stats"]["kernel_ms"] * 1e3)
                pwall.append(pus)
                old_kern.append(old["stats"]["kernel_ms"] * 1e3)
        entry[name] = dict(summary(wall, kern, pwall, old_kern, r), searches=int(S if w is None else w.shape[0]))
    DS.close()
    wall, kern, pwall, old_kern = [], [], [], []
    am = modes | KAD_STEP_APPLY
    for rep in range(reps + 1):
        DS = create()
        us, r = timed(lambda: DS.step_full(None, am))
        after = DS.export() if rep == 0 else None
        DS.close()
        DS = create()
        pus, p = timed(lambda: parent(DS, nodes, None, am, True))
        if rep == 0:
            assert same(r, p), "all_apply"
            twin = DS.export()
            assert all(np.array_equal(after[k], twin[k]) for k in after), "all_apply: the two paths leave different sets"
        DS.close()
        DS = create()
        old = DS.step(None, KAD_STEP_APPLY)
        DS.close()
        if rep:
            wall.append(us)
            kern.append(r["stats"]["kernel_ms"] * 1e3)
            pwall.append(pus)
            old_kern.append(old["stats"]["kernel_ms"] * 1e3)
    entry["all_apply"] = dict(summary(wall, kern, pwall, old_kern, r), searches=S, parent_sets_equal=True,
                              changed_searches=int(((p[0] | p[1] | p[2]) != 0).sum() + (((p[3] & KAD_STEP_EXPIRE) != 0) & ((p[0] | p[1] | p[2]) == 0)).sum()))
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sr_stepfull_bench needs a GPU")
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
