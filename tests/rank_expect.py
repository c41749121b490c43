"""The expectation of sbr_rank_targets, from per-item scores only: mask the history to f32::MIN, then for every target count
the items whose masked score is >= the target's (evaluation.rs:30-41 applied to each target on its own)."""
from __future__ import annotations

import numpy as np

F32_MIN = np.finfo(np.float32).min


def ranks_expectation(scores, masked, targets):
    """scores: [num_items] f32 of one user; masked: item ids whose score counts as f32::MIN; targets: item ids.
    -> [len(targets)] u32, rank(t) = #{i : m(i) >= m(t)}."""
    m = np.array(scores, dtype=np.float32, copy=True)
    ex = np.asarray(list(masked), dtype=np.int64)
    if ex.size:
        m[ex] = F32_MIN
    t = np.asarray(list(targets), dtype=np.int64)
    if t.size == 0:
        return np.zeros(0, dtype=np.uint32)
    return np.array([np.count_nonzero(m >= m[x]) for x in t], dtype=np.uint32)


def oracle_scores(o, num_items, histories):
    """[users, items] f32: the oracle's score of every item for every history (user_representation + predict)."""
    all_items = np.arange(num_items, dtype=np.uint32)
    return np.array([o.predict(o.user_representation(np.asarray(h, dtype=np.uint32)), all_items) for h in histories],
                    np.float32).reshape(len(histories), num_items)


def expect_all(scores, histories, targets, mask_history=True):
    """One u32 array per user from the [users, items] score matrix."""
    return [ranks_expectation(scores[u], np.unique(histories[u]) if mask_history else (), targets[u]) for u in range(len(targets))]


def assert_ranks_equal(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, u, g.shape, w.shape)
        assert np.array_equal(g, w), f"{what}: user {u}: {g.tolist()} vs {w.tolist()}"
