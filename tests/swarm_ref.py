"""The oracle's side of the swarm edge cases (swarm_cases.py): one SwarmModel per swarm and the capped lookups
(list_cap = 32, silent_cap = 64: the device's capacities), computed once and shared by the tests. CPU only."""
import functools

import numpy as np

import oracle as O
import swarm_cases as SC

LIST_CAP, SILENT_CAP = O.SW_LIST, O.SW_SILENT
FIELDS = ("list", "queried", "bad", "n", "hops", "done")


@functools.lru_cache(maxsize=None)
def model(name):
    return O.SwarmModel(SC.swarm(name))


@functools.lru_cache(maxsize=None)
def capped(name, off, max_hops=64):
    """The case's lookups under the device's capacities after at most max_hops hops: (list, queried, bad, n, hops,
    done, peak, silent, cap_hops), read-only."""
    _, src, tg = SC.case(name)
    out = model(name).search_cap(src, tg, off, LIST_CAP, SILENT_CAP, max_hops=max_hops)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def unbounded(name, off):
    _, src, tg = SC.case(name)
    return model(name).search_cap(src, tg, off, 0, 0)


def top64_distances(ids, tg, lst, n):
    """(distance (S, 32) uint64, valid (S, 32)) of each list entry to its lookup's target, top 64 bits."""
    key, tk = SC.key64(ids), SC.key64(tg)
    valid = np.arange(lst.shape[1])[None, :] < n.astype(np.int64)[:, None]
    return key[np.where(valid, lst, 0).astype(np.int64)] ^ tk[:, None], valid
