"""Shared by test_sr_tick*.py; nothing here touches the GPU. The trim bytes of kad_sr_plan_round
derived from a per-search trims array, plan_insert_round's result in the planner's form, and insert_ref.ModelSearches
extended with kad_sr_try_insert_tick restated over the model: the model's verdicts, the engine's planner
(opendht_amd.plan_round) and the model's insert, round by round."""
import numpy as np

import insert_ref as I
import searches_ref as R
from opendht_amd import _lib
from opendht_amd.searches import plan_insert_round, plan_round

FAR = (R.FAR, R.FAR_EXPIRED)
SKIPPED, READY, DEFERRED = _lib.KAD_SR_PLAN_SKIPPED, _lib.KAD_SR_PLAN_READY, _lib.KAD_SR_PLAN_DEFERRED
LEFT, TICK_SKIPPED, APPLIED = _lib.KAD_SR_TICK_LEFT, _lib.KAD_SR_TICK_SKIPPED, _lib.KAD_SR_TICK_APPLIED


def trim_bits(lb, fwd, back, stop, trims):
    """bit 0: the forward stopper is FAR / FAR_EXPIRED and trims[it]; bit 1: the same backwards."""
    out = np.zeros(len(stop), np.uint8)
    for k in range(len(stop)):
        l, f, b, fs, bs = int(lb[k]), int(fwd[k]), int(back[k]), int(stop[k]) & 15, int(stop[k]) >> 4
        out[k] = (1 if fs in FAR and trims[l + f] else 0) | (2 if bs in FAR and trims[l - b - 1] else 0)
    return out


def python_plan(S, lb, fwd, back, stop, trims):
    """plan_insert_round as (kind per candidate, {(search, candidate position, expected result)})."""
    skipped, ready, deferred = plan_insert_round(S, lb, fwd, back, stop, trims)
    kind = np.full(len(stop), 255, np.uint8)
    kind[skipped] = SKIPPED
    kind[[j for j, _ in ready]] = READY
    kind[deferred] = DEFERRED
    return kind, {(s, j, want) for j, pairs in ready for s, want in pairs}


def native_plan(S, lb, fwd, back, stop, trim):
    kind, pw, pc, want = plan_round(S, lb, fwd, back, stop, trim)
    assert list(pw) == sorted(set(int(s) for s in pw)), "pairs ascending by search, no search twice"
    return kind, {(int(s), int(j), int(w)) for s, j, w in zip(pw, pc, want)}


def trims_of_export(st):
    return (st["full"] != 0) & (st["t"] < st["n"])


class TickModel(I.ModelSearches):
    """insert_ref.ModelSearches with DeviceSearches.try_insert_tick."""

    def try_insert_tick(self, cand_ids, cand_flags=None, max_rounds=0):
        cand = np.asarray(cand_ids, np.uint8).reshape(-1, 20)
        q = cand.shape[0]
        fl = np.zeros(q, np.uint8) if cand_flags is None else np.asarray(cand_flags, np.uint8)
        out = {"kind": np.full(q, LEFT, np.uint8), "round": np.zeros(q, np.uint32), "lb": np.zeros(q, np.uint32),
               "fwd": np.zeros(q, np.uint32), "back": np.zeros(q, np.uint32), "stop": np.zeros(q, np.uint8),
               "trim": np.zeros(q, np.uint8)}
        st = {k: 0 for k in ("rounds", "skipped", "applied", "left", "pairs", "overflowed")}
        over = []
        if q == 0 or self.S == 0:
            out["kind"][:] = TICK_SKIPPED
            st["skipped"] = q
            return dict(out, overflow=np.zeros(0, np.uint32), stats=st)
        assert self.cap <= 64
        rem = np.arange(q)
        while len(rem) and not over and (max_rounds == 0 or st["rounds"] < max_rounds):
            st["rounds"] += 1
            lb, fwd, back, stop = self.try_insert_host(cand[rem])
            trim = trim_bits(lb, fwd, back, stop, trims_of_export(self.export(nodes=False)))
            kind, pw, pc, want = plan_round(self.S, lb, fwd, back, stop, trim)
            done = kind != DEFERRED
            for name, v in (("lb", lb), ("fwd", fwd), ("back", back), ("stop", stop), ("trim", trim)):
                out[name][rem[done]] = v[done]
            out["round"][rem[done]] = st["rounds"]
            out["kind"][rem[done]] = np.where(kind[done] == READY, APPLIED, TICK_SKIPPED)
            st["skipped"] += int((kind == SKIPPED).sum())
            st["applied"] += int((kind == READY).sum())
            if len(pw):
                ins, status = self.insert(pw, np.arange(len(pw) + 1, dtype=np.uint32), cand[rem[pc]], fl[rem[pc]])
                st["pairs"] += len(pw)
                for k in range(len(pw)):
                    if status[k] == I.INSERT_OVERFLOW:
                        over.append(int(pw[k]))
                    else:
                        assert ins[k] == want[k], (int(pw[k]), int(rem[pc[k]]))
            rem = rem[kind == DEFERRED]
        st["left"], st["overflowed"] = len(rem), len(over)
        return dict(out, overflow=np.array(over, np.uint32), stats=st)
