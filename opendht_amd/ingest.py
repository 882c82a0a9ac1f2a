"""Round-based table ingest: a stream of candidate nodes becomes kad_table_apply batches without
a host walk of the table.

Dht::onNewNode(node, 0) (dht.cpp:867-936) handles candidates one at a time, each seeing the table the earlier ones
left. kad_rt_triage_batch decides a whole batch against one snapshot, so its verdicts hold only for candidates
whose bucket no earlier candidate of the batch changed. A round therefore triages every pending candidate in one
launch, walks them in order on the host and lets at most one candidate change each bucket; the others of that
bucket wait, in order, for the next round, which sees the table after one T.apply. A verdict that changes nothing
(KNOWN, FULL, NONE) is final only while its bucket is untouched in the round, for the same reason. After a split
the reference runs onNewNode again on the same node (dht.cpp:925), so the candidate stays pending.
"""
from __future__ import annotations

import numpy as np

from ._lib import (KAD_NN_FULL, KAD_NN_INSERT, KAD_NN_KIND_MASK, KAD_NN_KNOWN, KAD_NN_NONE, KAD_NN_REPLACE,
                   KAD_NN_SPLIT, KAD_OP_INSERT, KAD_OP_REPLACE, KAD_OP_SPLIT)

KIND_NAMES = {KAD_NN_NONE: "none", KAD_NN_KNOWN: "known", KAD_NN_REPLACE: "replace", KAD_NN_INSERT: "insert",
              KAD_NN_SPLIT: "split", KAD_NN_FULL: "full"}


def ingest(T, ids, status, self_id, bootstrap: bool = False, max_rounds: int = 256) -> dict:
    """Feed candidates (ids (m, 20) uint8, status (m,) uint8, in arrival order) to the device table T as
    Dht::onNewNode(node, 0) would, one triage launch and one T.apply per round. Returns the per-kind counts of the
    verdicts acted on ("none", "known", "replace", "insert", "split", "full") and "rounds"; raises RuntimeError
    when candidates are still pending after max_rounds rounds."""
    import torch

    ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 20)
    status = np.ascontiguousarray(status, dtype=np.uint8)
    if status.shape != (ids.shape[0],):
        raise ValueError("status must have one byte per candidate")
    dev = torch.device("cuda", T.device)
    counts = {name: 0 for name in KIND_NAMES.values()}
    pending = np.arange(ids.shape[0])
    rounds = 0
    while pending.size:
        if rounds == max_rounds:
            raise RuntimeError(f"ingest: {pending.size} candidates still pending after {max_rounds} rounds")
        rounds += 1
        verdict, node, bucket = T.rt_triage(torch.from_numpy(ids[pending]).to(dev), self_id, bootstrap,
                                            want_bucket=True)
        torch.cuda.synchronize(dev)
        kind = verdict.cpu().numpy() & KAD_NN_KIND_MASK
        node = node.cpu().numpy().view(np.uint32)
        bucket = bucket.cpu().numpy().view(np.uint32)
        touched, split_at = set(), []  # buckets changed this round (snapshot indices); those split, in op order
        ops, new, later = [], [], []
        for j, c in enumerate(pending):
            k, b = int(kind[j]), int(bucket[j])
            if b in touched:
                later.append(c)
                continue
            counts[KIND_NAMES[k]] += 1
            if k == KAD_NN_REPLACE:
                ops.append((KAD_OP_REPLACE, int(node[j]) - T.index_base, len(new)))
                new.append(c)
            elif k == KAD_NN_INSERT:
                ops.append((KAD_OP_INSERT, len(new), 0))
                new.append(c)
            elif k == KAD_NN_SPLIT:
                ops.append((KAD_OP_SPLIT, b + sum(1 for s in split_at if s < b), 0))
                split_at.append(b)
                later.append(c)
            else:
                continue  # KNOWN, FULL, NONE: nothing changes
            touched.add(b)
        if ops:
            T.apply(np.array(ops, np.uint32), ids[new], status[new])
        pending = np.array(later, dtype=np.int64)
    counts["rounds"] = rounds
    return counts
