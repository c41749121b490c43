"""The expectation of rank_targets under a serving policy (ELIGIBLE RANKS, include/sbr_hip.h), from per-item scores only: the
mask list M = unique(list) ∪ {items the tag masks forbid} ∪ (catalogue \\ set) as a Python set, then rank_expect's statement of
sbr_rank_targets with that list.  Nothing here is shared with the product."""
from __future__ import annotations

import numpy as np

from rank_expect import ranks_expectation


def forbidden_items(tags, any_of, none_of) -> set:
    """the items whose tag word the mask pair does not allow: a none_of bit set, or any_of != 0 and none of its bits set"""
    any_of, none_of = int(any_of), int(none_of)
    out = set()
    for i, t in enumerate(np.asarray(tags).tolist()):
        if (t & none_of) != 0 or (any_of != 0 and (t & any_of) == 0):
            out.add(i)
    return out


def mask_list(num_items, listed=(), tags=None, any_of=0, none_of=0, members=None) -> set:
    """M of one row: ``listed`` its list (history, exclusions, seen items: any order, repeats allowed), ``tags`` the catalogue's
    tag words (None: no filter), ``members`` the item set's ids (None: no set)"""
    m = {int(i) for i in np.asarray(listed).ravel().tolist()}
    if tags is not None:
        m |= forbidden_items(tags, any_of, none_of)
    if members is not None:
        m |= set(range(int(num_items))) - {int(i) for i in np.asarray(members).ravel().tolist()}
    return m


def eligible_ranks(scores, targets, listed=(), tags=None, any_of=0, none_of=0, members=None):
    """scores [num_items] f32 of one row -> [len(targets)] u32"""
    return ranks_expectation(scores, sorted(mask_list(len(scores), listed, tags, any_of, none_of, members)), targets)


def expect_rows(scores, targets, lists=None, tags=None, any_of=None, none_of=None, members=None):
    """the flat u32 ranks of every row's targets, in row and target order: scores [rows, items]; lists one per row or None; any_of /
    none_of one word per row or None"""
    out = []
    for u in range(len(targets)):
        out.append(eligible_ranks(scores[u], targets[u], () if lists is None else lists[u], tags,
                                  0 if any_of is None else any_of[u], 0 if none_of is None else none_of[u], members))
    return np.concatenate(out) if out else np.zeros(0, np.uint32)
