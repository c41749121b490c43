"""The contract of sbr_sessions_rollout (ROLLOUT in include/sbr_hip.h) a second time, in numpy, over two callables:

    rep(history) -> h              the oracle's user_representation of a list of item ids (the empty list: the empty history)
    scores(h) -> f32 [num_items]   the oracle's predict of h over every item

On top of those it states the total order (recommend_expect), the growing exclusion set and the ended rows; sample mode reuses
sampled_expect at k = 1 and seed + j, the partition reuses partition_expect.  The oracle windows a history to max_sequence_length
where a session keeps the whole recurrence, so this is the truth only while len(history) + steps <= max_sequence_length."""
from __future__ import annotations

import numpy as np

from partition_expect import allowed_mask, partition_row
from recommend_expect import NO_ITEM, topk_expectation
from sampled_expect import inv_temperature, noise, sampled_expectation

F = np.float32


class Expected:
    """items u32 / scores f32 [n, steps], lengths u32 [n]; keys f32 [n, steps] (sample mode) and shift f32 / mass u64 [n, steps]
    (partition) or None; histories: each row's history with its real picks appended."""

    def __init__(self, n, steps, sample, partition):
        self.items = np.full((n, steps), NO_ITEM, dtype=np.uint32)
        self.scores = np.full((n, steps), -np.inf, dtype=F)
        self.lengths = np.full(n, steps, dtype=np.uint32)
        self.keys = np.full((n, steps), -np.inf, dtype=F) if sample else None
        self.shift = np.full((n, steps), -np.inf, dtype=F) if partition else None
        self.mass = np.zeros((n, steps), dtype=np.uint64) if partition else None
        self.histories = []


def eligible_at_start(num_items, excluded, tags=None, any_of=0, none_of=0):
    """X_0 of one row as a bool mask: what recommend(k = 1) may choose from at call time."""
    return allowed_mask(num_items, excluded, tags, int(any_of), int(none_of))


def rollout_row(rep, scores, history, steps, x0, *, allow_repeats=False, sample=None, partition_temperature=None):
    """One row.  x0: bool [num_items], the row's X_0.  sample: None (greedy) or (temperature, seed, stream).  Returns the per-step
    tuples (item, score, key or None, shift or None, mass or None) of the real steps — fewer than `steps` when the row ended — and
    the history with the picks appended."""
    hist = [int(x) for x in history]
    ok = np.array(x0, dtype=bool)
    all_items = np.arange(ok.size, dtype=np.uint32)
    out = []
    for j in range(steps):
        if not ok.any():  # X_j is empty: the row ends, and X only shrinks
            break
        s = np.asarray(scores(rep(hist)), dtype=F)
        barred = np.flatnonzero(~ok)
        key = shift = mass = None
        if sample is None:
            it, sc = topk_expectation(s, barred, 1)
        else:
            temperature, seed, stream = sample
            g = noise((int(seed) + j) & 0xFFFFFFFFFFFFFFFF, np.array([stream], dtype=np.uint64), all_items)[0]
            it, sc, ky = sampled_expectation(s, barred, 1, inv_temperature(temperature), g)
            key = ky[0]
        if partition_temperature is not None:
            shift, mass = partition_row(s, barred, partition_temperature)
        pick = int(it[0])
        assert pick != NO_ITEM
        out.append((pick, sc[0], key, shift, mass))
        hist.append(pick)
        if not allow_repeats:
            ok[pick] = False
    return out, hist


def rollout_expect(rep, scores, num_items, histories, steps, excl=None, *, tags=None, any_of=None, none_of=None, allow_repeats=False,
                   sample=None, streams=None, partition_temperature=None) -> Expected:
    """Every row.  excl: one list per row or None; any_of / none_of: None, one mask or one per row (with tags [num_items]); sample:
    None or (temperature, seed), with streams one per row (default: the row's index)."""
    n = len(histories)
    exp = Expected(n, steps, sample is not None, partition_temperature is not None)

    def per_row(mk):
        return np.broadcast_to(np.asarray(0 if mk is None else mk, dtype=np.uint32), (n,))

    a, z = per_row(any_of), per_row(none_of)
    streams = np.arange(n, dtype=np.uint64) if streams is None else np.asarray(streams, dtype=np.uint64)
    for i in range(n):
        x0 = eligible_at_start(num_items, () if excl is None else excl[i], tags, a[i], z[i])
        row, hist = rollout_row(rep, scores, histories[i], steps, x0, allow_repeats=allow_repeats,
                                sample=None if sample is None else (sample[0], sample[1], streams[i]),
                                partition_temperature=partition_temperature)
        exp.lengths[i] = len(row)
        exp.histories.append(hist)
        for j, (pick, sc, key, shift, mass) in enumerate(row):
            exp.items[i, j], exp.scores[i, j] = pick, sc
            if key is not None:
                exp.keys[i, j] = key
            if shift is not None:
                exp.shift[i, j], exp.mass[i, j] = shift, mass
    return exp


def oracle_callables(o, num_items):
    """rep / scores over an oracle model"""
    all_items = np.arange(num_items, dtype=np.uint32)
    return (lambda hist: o.user_representation(np.asarray(hist, dtype=np.uint32)),
            lambda h: o.predict(h, all_items))
