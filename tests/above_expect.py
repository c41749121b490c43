"""The expectation of the *_above calls, from the contract (include/sbr_hip.h, ABOVE) alone: a numpy statement over a score matrix
of "every allowed column whose score is >= the row's threshold", as CSR in either order.  It shares no code with the product."""
from __future__ import annotations

import numpy as np


def thresholds_of(threshold, rows):
    """A scalar or one value per row -> f32 [rows]"""
    t = np.asarray(threshold, dtype=np.float32)
    return np.full(rows, t, np.float32) if t.ndim == 0 else t.reshape(rows)


def passing(scores, threshold, excluded=None, allowed=None):
    """[R, C] bool: column c passes row r iff scores[r, c] >= threshold[r] (the f32 compare: -0.0 == +0.0, ties pass), c is not in
    excluded[r] (any order, repeats allowed; None: no lists) and allowed[r, c] (None: every column)."""
    s = np.asarray(scores, dtype=np.float32)
    t = thresholds_of(threshold, s.shape[0])
    ok = s >= t[:, None]
    if allowed is not None:
        ok &= np.asarray(allowed, dtype=bool)
    if excluded is not None:
        assert len(excluded) == s.shape[0]
        for r, ex in enumerate(excluded):
            ex = np.asarray(ex, dtype=np.int64).ravel()
            ok[r, ex[ex < s.shape[1]]] = False
    return ok


def above_expect(scores, threshold, excluded=None, allowed=None, order="score", ids=None):
    """(ptr u64 [R + 1], ids u32 [N], scores f32 [N]) of scores [R, C].  order "id": each row by ascending column; "score": by
    score descending, ties (-0.0 and +0.0 among them) to the lower column.  ids (ascending, [C]): what the columns stand for."""
    assert order in ("score", "id")
    s = np.asarray(scores, dtype=np.float32)
    ok = passing(s, threshold, excluded, allowed)
    ptr = np.zeros(s.shape[0] + 1, np.uint64)
    out_i, out_s = [], []
    for r in range(s.shape[0]):
        cols = np.flatnonzero(ok[r])
        sc = s[r, cols]
        if order == "score":
            at = np.lexsort((cols, -sc.astype(np.float64)))  # primary: score descending; equal scores: the lower column
            cols, sc = cols[at], sc[at]
        out_i.append(cols)
        out_s.append(sc)
        ptr[r + 1] = ptr[r] + np.uint64(cols.size)
    cols = np.concatenate(out_i + [np.zeros(0, np.int64)]).astype(np.int64)
    names = cols if ids is None else np.asarray(ids, dtype=np.int64)[cols]
    return ptr, names.astype(np.uint32), np.concatenate(out_s + [np.zeros(0, np.float32)]).astype(np.float32)


def counts_expect(scores, threshold, excluded=None, allowed=None):
    """u64 [R]: the rows' numbers of pairs"""
    return passing(scores, threshold, excluded, allowed).sum(axis=1).astype(np.uint64)


def transposed(ptr, ids, scores, rows):
    """The (row, id, score) pairs of a CSR result as a sorted list of (id, row, score bits): the pairs of the transposed question"""
    ptr = np.asarray(ptr, dtype=np.int64)
    r = np.repeat(np.arange(rows), np.diff(ptr))
    bits = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return sorted(zip(np.asarray(ids).tolist(), r.tolist(), bits.tolist()))
