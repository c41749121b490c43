"""The expectation of sbr_sequence_ranks, from per-item scores only: for every user and position the scores of ALL items for the
state of the prefix, then rank_expect.ranks_expectation with the prefix's distinct items masked to f32::MIN and the position's
item as the one target.  The scores come from a function of the prefix — the oracle's user_representation + predict on the GPU
tests, a hand-made table on the CPU tests.  Nothing here is shared with the product."""
from __future__ import annotations

import numpy as np

from rank_expect import ranks_expectation


def window_of(seq, T):
    """The last min(n, T + 1) items of a sequence."""
    seq = np.asarray(seq, dtype=np.uint32).ravel()
    return seq[max(0, seq.size - (int(T) + 1)):]


def kept_positions(W, last=None):
    """Positions 1 .. W - 1 of a window of W items, or the last `last` of them."""
    pos = list(range(1, W))
    return pos if last is None else pos[max(0, len(pos) - int(last)):]


def expect_sequence_ranks(score_fn, seqs, T, mask_history=True, last=None):
    """score_fn(prefix: u32 array) -> [num_items] f32 scores for the state of that prefix.  One u32 array per sequence."""
    out = []
    for seq in seqs:
        w = window_of(seq, T)
        row = []
        for p in kept_positions(w.size, last):
            prefix = w[:p]
            row.append(ranks_expectation(score_fn(prefix), np.unique(prefix) if mask_history else (), [int(w[p])])[0])
        out.append(np.array(row, dtype=np.uint32))
    return out


def oracle_score_fn(o, num_items):
    """The oracle's scores of every item for a prefix, cached by prefix (prefixes recur across `last` and mask settings)."""
    all_items = np.arange(num_items, dtype=np.uint32)
    cache = {}

    def fn(prefix):
        key = prefix.tobytes()
        if key not in cache:
            cache[key] = np.asarray(o.predict(o.user_representation(np.asarray(prefix, dtype=np.uint32)), all_items), np.float32)
        return cache[key]

    return fn


def csr(seqs):
    ptr = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        ptr[1:] = np.cumsum([len(s) for s in seqs])
    items = np.concatenate([np.asarray(s, dtype=np.uint32) for s in seqs]) if len(seqs) else np.zeros(0, np.uint32)
    return ptr, np.ascontiguousarray(items, dtype=np.uint32)


def rows_of(ptr, ranks):
    ptr = np.asarray(ptr).astype(np.int64)
    return [np.asarray(ranks[ptr[u]: ptr[u + 1]], dtype=np.uint32) for u in range(len(ptr) - 1)]
