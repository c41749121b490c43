"""The expectation of the *_filtered calls, from the contract (include/sbr_hip.h, ITEM TAGS) alone: a numpy statement of "allowed",
and the plain expectation (recommend_expect.topk_expectation) with every item that is not allowed added to the exclusions.  It
shares no code with the product."""
from __future__ import annotations

import numpy as np

from recommend_expect import topk_expectation


def allowed(tags, any_of, none_of):
    """[num_items] bool: the items one user's mask pair lets through."""
    tags = np.asarray(tags, dtype=np.uint32)
    a, n = np.uint32(any_of), np.uint32(none_of)
    return ((tags & n) == 0) & ((a == 0) | ((tags & a) != 0))


def disallowed(tags, any_of, none_of):
    """The ids of the items that are not allowed, ascending: what the equivalent exclusion list adds."""
    return np.flatnonzero(~allowed(tags, any_of, none_of)).astype(np.uint32)


def masks_of(mask, nu):
    """None / a scalar / an array -> u32 [nu] (the Python layer's broadcast rule)."""
    if mask is None:
        return np.zeros(nu, np.uint32)
    a = np.asarray(mask)
    return np.full(nu, int(a), np.uint32) if a.ndim == 0 else a.astype(np.uint32)


def equivalent_exclusions(tags, any_of, none_of, nu, exclude=None):
    """One exclusion list per user: the caller's (None: none) extended by the user's disallowed items."""
    a, n = masks_of(any_of, nu), masks_of(none_of, nu)
    out = []
    for u in range(nu):
        own = np.zeros(0, np.uint32) if exclude is None else np.asarray(exclude[u], dtype=np.uint32).ravel()
        out.append(np.concatenate([own, disallowed(tags, a[u], n[u])]).astype(np.uint32))
    return out


def filtered_topk_expectation(scores, tags, any_of, none_of, excluded, k):
    """One user: scores [num_items] f32 -> (items [k] u32, scores [k] f32)."""
    ex = np.concatenate([np.asarray(list(excluded), dtype=np.int64), disallowed(tags, any_of, none_of).astype(np.int64)])
    return topk_expectation(scores, ex, k)


def filtered_expect(scores, tags, any_of, none_of, excl, k):
    """Every row of scores [users, num_items]; any_of / none_of as masks_of takes them; excl: one list per row, or None."""
    nu = len(scores)
    a, n = masks_of(any_of, nu), masks_of(none_of, nu)
    rows = [filtered_topk_expectation(scores[u], tags, a[u], n[u], () if excl is None else excl[u], k) for u in range(nu)]
    return (np.array([r[0] for r in rows], np.uint32).reshape(-1, k), np.array([r[1] for r in rows], np.float32).reshape(-1, k))
