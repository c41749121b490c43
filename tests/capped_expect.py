"""The expectation of the *_capped calls, from the contract (include/sbr_hip.h, CAPPED) alone.

    ranking   a row's eligible items in the total order: recommend_expect.topk_expectation at k = num_items (the oracle's scores,
              np.lexsort by (score descending, id ascending)), its padding cut off
    the rule  stated twice, independently: rule_walk — a dict of per-group counts while walking the ranking — and rule_ordinal — the
              ordinal of every entry within its group through one stable argsort by group, no walk
    C level   the rule on the first `pool` entries of the ranking, and complete = (k kept) or (the ranking is shorter than the pool)

It shares no code with the product."""
from __future__ import annotations

import numpy as np

from recommend_expect import NO_ITEM, topk_expectation

NO_GROUP = 0xFFFFFFFF


def rule_walk(ids, groups, cap, k):
    """Positions in ids (a ranking, best first) of the kept entries: walk, keep an entry iff its group is NO_GROUP or fewer than cap
    entries of its group were kept before it, stop after k."""
    kept, count = [], {}
    for j, i in enumerate(ids):
        if len(kept) >= k:
            break
        g = int(groups[int(i)])
        if g != NO_GROUP:
            if count.get(g, 0) >= cap:
                continue
            count[g] = count.get(g, 0) + 1
        kept.append(j)
    return np.asarray(kept, dtype=np.int64)


def rule_ordinal(ids, groups, cap, k):
    """The same positions without a walk: an entry is kept iff its group is NO_GROUP or its ordinal within its group, among the
    entries before it, is below cap; the first k of those."""
    g = np.asarray(groups, dtype=np.uint32)[np.asarray(ids, dtype=np.int64)]
    n = g.size
    by = np.argsort(g, kind="stable")  # within a group the positions ascend
    first = np.searchsorted(g[by], g[by], side="left")  # where each entry's group starts in the sorted order
    ordinal = np.empty(n, dtype=np.int64)
    ordinal[by] = np.arange(n) - first
    return np.flatnonzero((g == NO_GROUP) | (ordinal < cap))[:k]


def ranking(scores, excluded=(), allowed=None):
    """One row's eligible items in the total order -> (ids u32 [m], scores f32 [m]).  allowed: None or a bool per item."""
    scores = np.asarray(scores, dtype=np.float32)
    ex = [int(x) for x in excluded]
    if allowed is not None:
        ex += np.flatnonzero(~np.asarray(allowed, dtype=bool)).tolist()
    it, sc = topk_expectation(scores, ex, scores.size)
    m = int(np.count_nonzero(it != NO_ITEM))
    assert np.all(it[:m] != NO_ITEM)
    return it[:m], sc[:m]


def rankings_from_reps(o, num_items, reps, exclude=None, allowed=None):
    """The rankings of representation rows under the oracle's scores; exclude: None or one list per row; allowed: None or bool
    [rows, num_items] (a tag filter evaluated by the caller)."""
    all_items = np.arange(num_items, dtype=np.uint32)
    return [ranking(o.predict(r, all_items), () if exclude is None else exclude[u], None if allowed is None else allowed[u])
            for u, r in enumerate(np.asarray(reps, dtype=np.float32))]


def rankings_from_histories(o, num_items, ptr, item_ids, include_history=False, allowed=None):
    ptr = np.asarray(ptr, dtype=np.int64)
    all_items = np.arange(num_items, dtype=np.uint32)
    out = []
    for u in range(len(ptr) - 1):
        h = np.asarray(item_ids[ptr[u]: ptr[u + 1]], dtype=np.uint32)
        s = o.predict(o.user_representation(h), all_items)
        out.append(ranking(s, () if include_history else np.unique(h), None if allowed is None else allowed[u]))
    return out


def capped_row(rank, groups, cap, k, pool=None, rule=rule_walk):
    """One row: (items [k] u32, scores [k] f32, complete).  pool None: the rule over the whole ranking, the exact answer; else the
    C-level expectation at that pool."""
    ids, sc = rank
    n = ids.size if pool is None else min(pool, ids.size)
    kept = rule(ids[:n], groups, cap, k)
    items = np.full(k, NO_ITEM, dtype=np.uint32)
    scores = np.full(k, -np.inf, dtype=np.float32)
    items[: kept.size] = ids[kept]
    scores[: kept.size] = sc[kept]
    return items, scores, bool(pool is None or kept.size >= k or ids.size < pool)


def capped_rows(ranks, groups, cap, k, pool=None, rule=rule_walk):
    """-> (items [U, k], scores [U, k], complete [U] bool)"""
    out = [capped_row(r, groups, cap, k, pool, rule) for r in ranks]
    return (np.array([r[0] for r in out], dtype=np.uint32).reshape(-1, k), np.array([r[1] for r in out], dtype=np.float32).reshape(-1, k),
            np.array([r[2] for r in out], dtype=bool))
