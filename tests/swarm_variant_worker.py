"""One swarm lookup batch, hop by hop, in a process of its own: kad_search_hop reads its A/B switches (KAD_SWARM_WIDE,
KAD_SWARM_SEQ, KAD_SWARM_NETPF, KAD_SWARM_QUERY, KAD_SWARM_FUSED) once per process, so tests/test_swarm_edges.py
starts this worker once per variant, with the variant's environment.

    python swarm_variant_worker.py CASE OUT.npz

CASE is one of variant_case's names. The C ABI is called with host numpy arrays (kad_search_create's uploads are
hipMemcpyDefault). OUT.npz holds, stacked by hop: list, queried, bad, n, hops, done (kad_search_get after the hop),
overflow and active."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_HOPS = 40


def variant_case(name):
    """(ids, src, targets, offline_per_10k)"""
    import swarm_cases as SC

    if name == "tied_pairs":
        return SC.tied_pairs() + (0,)
    swarm, off = name.rsplit("@", 1)
    return SC.case(swarm) + (int(off),)


def main(argv):
    for p in (os.path.dirname(HERE), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from opendht_amd._lib import check, lib, ptr

    case, out = argv
    ids, src, tg, off = variant_case(case)
    ids, src, tg = (np.ascontiguousarray(a) for a in (ids, src.astype(np.uint32), tg))
    S = src.shape[0]
    L = lib()
    sw, x = C.c_void_p(), C.c_void_p()
    check(L.kad_swarm_create(C.byref(sw), 0, ids.shape[0], ptr(ids)), "kad_swarm_create")
    check(L.kad_search_create(C.byref(x), sw, S, ptr(src), ptr(tg), off, None), "kad_search_create")
    rec = {k: [] for k in ("list", "queried", "bad", "n", "hops", "done", "overflow", "active")}
    for _ in range(MAX_HOPS):
        active = C.c_uint32()
        check(L.kad_search_hop(x, C.byref(active)), "kad_search_hop")
        lst, q, bad = np.empty((S, 32), np.uint32), np.empty((S, 32), np.uint8), np.empty((S, 32), np.uint8)
        n, hops, done = np.empty(S, np.uint8), np.empty(S, np.uint32), np.empty(S, np.uint8)
        ovf = C.c_uint32()
        check(L.kad_search_get(x, ptr(lst), ptr(q), ptr(bad), ptr(n), ptr(hops), ptr(done), C.byref(ovf)),
              "kad_search_get")
        for k, v in zip(rec, (lst, q, bad, n, hops, done, ovf.value, active.value)):
            rec[k].append(v)
        if active.value == 0:
            break
    check(L.kad_search_destroy(x), "kad_search_destroy")
    check(L.kad_swarm_destroy(sw), "kad_swarm_destroy")
    np.savez(out, **{k: np.array(v) for k, v in rec.items()})
    assert "torch" not in sys.modules
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
