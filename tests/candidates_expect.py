"""The expectations of sbr_recommend_among and sbr_score_candidates, from the CPU oracle's user_representation and predict:

    recommend_among:   predict over ALL items, then recommend_expect.topk_expectation with excluded = history (or the caller's
                       list) ∪ complement(S) — the contract's "sbr_recommend with every item outside S ineligible", word for word
    score_candidates:  predict(user_representation(history), list), per user

and the tables and item sets the GPU tests share."""
from __future__ import annotations

import numpy as np

from recommend_expect import topk_expectation


def planted_params(items, d, seed):
    """0.3 * randn rows and biases rounded to 0.1, with 20 rows (and their biases) copied from item 0: exact score ties for every
    user, which must resolve to the lower id.  -> (E, bias, the ids of the 21 tied items, ascending)"""
    rs = np.random.RandomState(seed)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    bias = np.round(rs.randn(items) * 0.5, 1).astype(np.float32)
    dups = np.sort(rs.choice(np.arange(1, items), min(20, items - 1), replace=False))
    E[dups] = E[0]
    bias[dups] = bias[0]
    return E, bias, np.concatenate([[0], dups]).astype(np.uint32)


def planted_subset(items, n, tied, seed):
    """n distinct item ids, unsorted: every second tied item first (so ties exist INSIDE the set, and the lowest tied id of the
    set is not the catalogue's whenever n allows), the other tied items left out unless n == items."""
    if n >= items:
        return np.random.RandomState(seed).permutation(items).astype(np.uint32)
    rs = np.random.RandomState(seed)
    inside, outside = tied[1::2], tied[0::2]
    rest = np.setdiff1d(np.arange(items), np.concatenate([inside, outside]))
    pool = np.concatenate([inside, rs.permutation(rest), outside])  # the left-out tied items come in last
    s = pool[:n].astype(np.uint32)
    rs.shuffle(s)
    return s


class AmongExpectation:
    """Per-user score vectors over the whole catalogue (computed once), and the rows recommend_among must give for an item set."""

    def __init__(self, o, num_items, reps):
        self.num_items = num_items
        all_items = np.arange(num_items, dtype=np.uint32)
        self.scores = [o.predict(np.asarray(r, np.float32), all_items) for r in reps]

    @classmethod
    def from_histories(cls, o, num_items, ptr, item_ids):
        ptr = np.asarray(ptr, dtype=np.int64)
        hists = [np.asarray(item_ids[ptr[u]: ptr[u + 1]], dtype=np.uint32) for u in range(len(ptr) - 1)]
        e = cls(o, num_items, [o.user_representation(h) for h in hists])
        e.hists = hists
        return e

    def rows(self, subset, k, exclude=None, users=None):
        """exclude: None or one sequence of item ids per user -> (items [U, k] u32, scores [U, k] f32)"""
        outside = np.setdiff1d(np.arange(self.num_items), np.asarray(subset, dtype=np.int64))
        ri, rs = [], []
        for u in (range(len(self.scores)) if users is None else users):
            ex = outside if exclude is None else np.union1d(outside, np.asarray(exclude[u], dtype=np.int64))
            it, sc = topk_expectation(self.scores[u], ex, k)
            ri.append(it)
            rs.append(sc)
        return np.array(ri, dtype=np.uint32).reshape(-1, k), np.array(rs, dtype=np.float32).reshape(-1, k)


def oracle_candidate_scores(o, hists, cands):
    """predict(user_representation(history), candidates) per user: a list of f32 arrays"""
    return [o.predict(o.user_representation(np.asarray(h, np.uint32)), np.asarray(c, np.uint32)) if len(c) else np.zeros(0, np.float32)
            for h, c in zip(hists, cands)]
