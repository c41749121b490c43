"""The expectation of the *_top calls, from the contract (include/sbr_hip.h, TOP) alone: a numpy statement over a score matrix of
"the first min(n, eligible) allowed columns of a row by (score descending, column ascending), zeros tied", as CSR in either order,
with the rows' cuts taken from the definition.  It shares no code with the product."""
from __future__ import annotations

import numpy as np


def budgets_of(n, rows):
    """A scalar or one value per row -> python ints [rows]"""
    b = np.asarray(n)
    return [int(b)] * rows if b.ndim == 0 else [int(x) for x in b.reshape(rows)]


def key_of(x):
    """The monotone u32 of f32 values: a < b as floats <=> key(a) < key(b), and -0.0 has +0.0's key"""
    f = np.array(x, dtype=np.float32, ndmin=1, copy=True)
    f[f == 0] = np.float32(0.0)
    b = f.view(np.uint32)
    return np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def eligible(scores, excluded=None, allowed=None):
    """[R, C] bool: column c is eligible for row r iff it is not in excluded[r] (any order, repeats allowed; None: no lists) and
    allowed[r, c] (None: every column)"""
    s = np.asarray(scores, dtype=np.float32)
    ok = np.ones(s.shape, bool)
    if allowed is not None:
        ok &= np.asarray(allowed, dtype=bool)
    if excluded is not None:
        assert len(excluded) == s.shape[0]
        for r, ex in enumerate(excluded):
            ex = np.asarray(ex, dtype=np.int64).ravel()
            ok[r, ex[ex < s.shape[1]]] = False
    return ok


def top_expect(scores, n, excluded=None, allowed=None, order="score", ids=None):
    """(ptr u64 [R + 1], ids u32 [N], scores f32 [N], cuts f32 [R]) of scores [R, C].  Row r: its eligible columns in a stable sort by
    (key descending, column ascending), the first n[r] of them; order "id" then lists them by ascending column.  cuts[r]: the score of
    the last one taken (a zero as +0.0) when at least n[r] >= 1 are eligible, -inf when fewer than n[r] are, +inf for n[r] = 0.  ids
    (ascending, [C]): what the columns stand for."""
    assert order in ("score", "id")
    s = np.asarray(scores, dtype=np.float32)
    ok = eligible(s, excluded, allowed)
    want = budgets_of(n, s.shape[0])
    ptr = np.zeros(s.shape[0] + 1, np.uint64)
    cuts = np.zeros(s.shape[0], np.float32)
    out_i, out_s = [], []
    for r in range(s.shape[0]):
        cols = np.flatnonzero(ok[r])
        at = np.lexsort((cols, -key_of(s[r, cols]).astype(np.int64)))  # primary: key descending; equal keys: the lower column
        take = cols[at][: want[r]]
        if want[r] == 0:
            cuts[r] = np.inf
        elif cols.size < want[r]:
            cuts[r] = -np.inf
        else:
            last = s[r, take[-1]]
            cuts[r] = np.float32(0.0) if last == 0 else last
        if order == "id":
            take = np.sort(take)
        out_i.append(take)
        out_s.append(s[r, take])
        ptr[r + 1] = ptr[r] + np.uint64(take.size)
    cols = np.concatenate(out_i + [np.zeros(0, np.int64)]).astype(np.int64)
    names = cols if ids is None else np.asarray(ids, dtype=np.int64)[cols]
    return ptr, names.astype(np.uint32), np.concatenate(out_s + [np.zeros(0, np.float32)]).astype(np.float32), cuts
