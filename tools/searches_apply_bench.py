"""Timing of device-side add/erase of live searches (kad_searches_apply) on sets of S searches with
slabs of 32 entries in the states of tools/refill_bench.py (0..14 nodes per search), for S = 1k, 64k and 1M. Three
changes per size: one inserted search; 1 % of the searches erased and as many inserted, scattered; the slabs grown from
32 to 64 entries with the membership unchanged.

Timed in the same run, medians after a warm-up, every repetition starting from a set created anew in the first state
(not timed):

    a  apply       kad_searches_apply end to end on host arrays (wall clock: the host plan, the allocations, the upload of
                   one word per search and the new IDs, the relayout and directory kernels, the frees)
    b  old path    what a caller did before: kad_searches_create of the final state from CSR arrays prepared beforehand
                   and not timed, plus the destroy of the old set. Building the CSR is left out, so b is a lower bound
    c  copy floor  one device-to-device copy of as many bytes as the relayout writes (records and slabs of the new set),
                   between events: the floor of the relayout kernel

The device time of the kernels comes from a profiler run of their own, which repeats only the applies:

    python tools/searches_apply_bench.py --out profiles/r12/searches_apply/apply_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/searches_apply_bench.py --applies-only
    python tools/searches_apply_bench.py --kernel-trace DIR --out profiles/r12/searches_apply/apply_bench.json

The last call reads the trace (the relayout dispatches in launch order are the sizes times the changes times reps + 1)
and adds the kernel medians and kernel / c to the JSON.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from refill_bench import make_set, med, sorted_ids  # noqa: E402

CAP = 32
CHANGES = ("one_insert", "one_percent", "cap_32_to_64")


def new_ids(count, seed):
    """count random IDs in random order (160 bits: none is in the set)."""
    ids = sorted_ids(count, seed)
    return np.ascontiguousarray(ids[np.random.default_rng(seed).permutation(ids.shape[0])])


def change_of(name, ids, offs, nodes, seed):
    """(erase, ins_ids, new cap or None) and the CSR arrays of the final state."""
    S = ids.shape[0]
    rng = np.random.default_rng(seed)
    if name == "cap_32_to_64":
        return np.zeros(0, np.uint32), np.zeros((0, 20), np.uint8), 2 * CAP, (ids, offs, nodes, 2 * CAP)
    m = 1 if name == "one_insert" else max(S // 100, 1)
    erase = np.zeros(0, np.uint32) if name == "one_insert" else np.sort(rng.choice(S, m, replace=False)).astype(np.uint32)
    ins = new_ids(m, seed + 1)
    n = np.diff(offs.astype(np.int64))
    keep = np.ones(S, bool)
    keep[erase] = False
    all_ids = np.concatenate([ids[keep], ins])
    order = np.lexsort(all_ids.T[::-1])  # the inserted lists are empty: the kept lists stay in their order
    n_f = np.concatenate([n[keep], np.zeros(ins.shape[0], np.int64)])[order]
    offs_f = np.zeros(n_f.shape[0] + 1, np.uint32)
    offs_f[1:] = np.cumsum(n_f)
    return erase, ins, None, (np.ascontiguousarray(all_ids[order]), offs_f,
                              np.ascontiguousarray(nodes[np.repeat(keep, n)]), CAP)


def create(csr):
    from opendht_amd import DeviceSearches

    ids, offs, nodes, cap = csr
    return DeviceSearches(ids, np.zeros(ids.shape[0], np.uint8), offs, nodes, np.zeros(nodes.shape[0], np.uint8),
                          cap=cap, device=0)


def run(args):
    import torch

    from opendht_amd._lib import check, lib, ptr

    L = lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    res = {"cap": CAP, "reps": args.reps, "sets": {}}
    for S in (int(v) for v in args.sizes.split(",")):
        ids, offs, nodes = make_set(S, 0x11B0 + S)
        S = ids.shape[0]
        first = (ids, offs, nodes, CAP)
        entry = {"S": S}
        for name in CHANGES:
            erase, ins, cap2, final = change_of(name, ids, offs, nodes, 0x12A0 + S)
            S2, capf = final[0].shape[0], final[3]
            moved = 64 * S2 + 21 * S2 * capf
            a_wall, b_wall, c_copy = [], [], []
            remap, new_index = np.zeros(S, np.uint32), np.zeros(ins.shape[0], np.uint32)
            if not args.applies_only:
                src, dst = (torch.empty(moved, dtype=torch.uint8, device=dev) for _ in range(2))
            for rep in range(args.reps + 1):
                DS = create(first)
                torch.cuda.synchronize()
                t0 = time.perf_counter()  # the C call itself: DeviceSearches.apply also permutes its host copy of the IDs
                rc = L.kad_searches_apply(DS._h, ptr(erase), erase.shape[0], ptr(ins), None, ins.shape[0], cap2 or 0,
                                          ptr(remap), ptr(new_index))
                t1 = time.perf_counter()
                check(rc, "kad_searches_apply")
                if rep:
                    a_wall.append((t1 - t0) * 1e6)
                if rep == 0:
                    bytes_after = DS.device_bytes
                if args.applies_only:
                    DS.close()
                    continue
                t0 = time.perf_counter()
                new = create(final)
                DS.close()
                t1 = time.perf_counter()
                if rep == 0 and new.device_bytes != bytes_after:
                    raise SystemExit(f"{name} at {S}: the applied set holds {bytes_after} bytes, the created one "
                                     f"{new.device_bytes}")
                new.close()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                dst.copy_(src)
                e1.record(stream)
                torch.cuda.synchronize()
                if rep:
                    b_wall.append((t1 - t0) * 1e6)
                    c_copy.append(e0.elapsed_time(e1) * 1e3)
            ch = {"erased": int(erase.shape[0]), "inserted": int(ins.shape[0]), "S_after": S2, "cap_after": capf,
                  "relayout_bytes_written": moved, "relayout_bytes_read": (S - int(erase.shape[0])) * (64 + 21 * CAP),
                  "uploaded_bytes": 4 * S2 + 20 * int(ins.shape[0]),
                  "old_path_uploaded_bytes": 64 * S2 + 21 * S2 * capf, "a_apply_end_to_end": med(a_wall)}
            if not args.applies_only:
                a, b, c = ch["a_apply_end_to_end"], med(b_wall), med(c_copy)
                ch.update(b_create_destroy_lower_bound=b, c_device_copy=c, b_over_a=b["median_us"] / a["median_us"],
                          a_beats_b=bool(a["median_us"] < b["median_us"]),
                          c_copy_GBps=2 * moved / c["median_us"] / 1e3)
                del src, dst
            entry[name] = ch
            print(f"S {S} {name}: a {ch['a_apply_end_to_end']['median_us']:.0f} us", file=sys.stderr, flush=True)
        res["sets"][str(S)] = entry
    return res


def merge_trace(args):
    """The relayout and directory kernels' durations from a rocprofv3 kernel trace of an --applies-only run."""
    files = glob.glob(os.path.join(args.kernel_trace, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {args.kernel_trace}, found {files}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    relayout = [r for r in rows if "searches_relayout_kernel" in r["Kernel_Name"]]
    res = json.load(open(args.out))
    sets = list(res["sets"].values())
    per = res["reps"] + 1
    if len(relayout) != len(sets) * len(CHANGES) * per:
        raise SystemExit(f"{len(relayout)} relayout dispatches in the trace, expected {len(sets) * len(CHANGES) * per}")
    pairs = []  # every relayout dispatch with the directory kernel that follows it, if any
    for r in rows:
        if "searches_relayout_kernel" in r["Kernel_Name"]:
            pairs.append([r, None])
        elif "searches_rdx_kernel" in r["Kernel_Name"] and pairs and pairs[-1][1] is None:
            pairs[-1][1] = r
    k = 0
    for entry in sets:
        for name in CHANGES:
            mine = pairs[k + 1:k + per]  # without the warm-up
            k += per
            ch = entry[name]
            ch["relayout_kernel"] = med([us(r) for r, _ in mine])
            ch["relayout_kernel_variant"] = "16-byte" if "ILb1E" in mine[0][0]["Kernel_Name"] or \
                "<true>" in mine[0][0]["Kernel_Name"] else "narrow"
            ch["rdx_kernel"] = med([us(d) for _, d in mine]) if all(d is not None for _, d in mine) else None
            ch["kernel_over_c"] = ch["relayout_kernel"]["median_us"] / ch["c_device_copy"]["median_us"]
            ch.pop("relayout_GBps_twice_written", None)
            ch["relayout_GBps_read_plus_written"] = ((ch["relayout_bytes_read"] + ch["relayout_bytes_written"]) /
                                                     ch["relayout_kernel"]["median_us"] / 1e3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--applies-only", action="store_true", help="only the applies: the run to put under the profiler")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 kernel trace to fold into --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = merge_trace(args) if args.kernel_trace else run(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out and not args.applies_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
