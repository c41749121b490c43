"""The expectation of sbr_recommend, from per-item scores only: mask the exclusions, order by (score descending, item id
ascending) with np.lexsort, keep the first k, pad with (NO_ITEM, -inf)."""
from __future__ import annotations

import numpy as np

NO_ITEM = 0xFFFFFFFF


def topk_expectation(scores, excluded, k):
    """scores: [num_items] f32 of one user; excluded: item ids that may not appear.  -> (items [k] u32, scores [k] f32)"""
    scores = np.asarray(scores, dtype=np.float32)
    keep = np.ones(scores.size, dtype=bool)
    ex = np.asarray(list(excluded), dtype=np.int64)
    if ex.size:
        keep[ex] = False
    ids = np.flatnonzero(keep)
    s = scores[ids]
    order = np.lexsort((ids, -s))[:k]
    items = np.full(k, NO_ITEM, dtype=np.uint32)
    out = np.full(k, -np.inf, dtype=np.float32)
    items[: order.size] = ids[order]
    out[: order.size] = s[order]
    return items, out


def oracle_recommend(o, num_items, ptr, item_ids, k, include_history=False, users=None):
    """The oracle's answer for the users `users` (default: all): orc_user_representation of each history, orc_predict over
    every item, topk_expectation with the whole history excluded unless include_history."""
    ptr = np.asarray(ptr, dtype=np.int64)
    users = range(len(ptr) - 1) if users is None else users
    all_items = np.arange(num_items, dtype=np.uint32)
    rows_i, rows_s = [], []
    for u in users:
        h = np.asarray(item_ids[ptr[u]: ptr[u + 1]], dtype=np.uint32)
        s = o.predict(o.user_representation(h), all_items)
        it, sc = topk_expectation(s, () if include_history else np.unique(h), k)
        rows_i.append(it)
        rows_s.append(sc)
    return np.array(rows_i, dtype=np.uint32).reshape(-1, k), np.array(rows_s, dtype=np.float32).reshape(-1, k)
