"""The expectation of recommend_sampled, stated a second time from the contract (include/sbr_hip.h SAMPLING) alone:
the counter-keyed Gumbel noise in numpy — uint32 / uint64 wrapping arithmetic and float32 element-wise +, -, *, /, each rounded
once — and the plain top-k expectation (recommend_expect.topk_expectation) over the keys

    key(u, i) = fl(fl(score(u, i) * inv_t) + g(seed, stream_u, i)).

The k best keys in key order are k draws without replacement from softmax(score / T) (the Gumbel-top-k identity).  It shares no
code with the product."""
from __future__ import annotations

import numpy as np

from recommend_expect import NO_ITEM, topk_expectation

F = np.float32
M64 = (1 << 64) - 1
LN2_HI = F(0.693359375)
LN2_LO = F(-2.12194440e-4)
SQRT2 = F(1.41421356)
C9, C7, C5, C3 = F(1.0 / 9.0), F(1.0 / 7.0), F(1.0 / 5.0), F(1.0 / 3.0)


def mix64(z):
    """sbr_mix64 on a Python int (mod 2^64)."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def row_keys(seed, streams):
    """K of each row: (k0 [n] u32, k1 [n] u32) = the low and high halves of mix64(seed ^ mix64(stream * 0x9E3779B97F4A7C15 + 1))."""
    streams = streams.ravel().tolist() if isinstance(streams, np.ndarray) else list(streams)  # Python ints: all 64 bits survive
    ks = [mix64(int(seed) ^ mix64(int(s) * 0x9E3779B97F4A7C15 + 1)) for s in streams]
    k = np.array(ks, dtype=np.uint64)
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32), (k >> np.uint64(32)).astype(np.uint32)


def hash_r(k0, k1, items):
    """The 23 noise bits of (row key, item): broadcasts k0 / k1 against items (all uint32)."""
    with np.errstate(over="ignore"):
        x = np.asarray(items, dtype=np.uint32) ^ np.asarray(k0, dtype=np.uint32)
        x ^= x >> np.uint32(16); x = x * np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13); x = x * np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
        x = x + np.asarray(k1, dtype=np.uint32)
        x ^= x >> np.uint32(16); x = x * np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15); x = x * np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x >> np.uint32(9)


def log32(x):
    """The contract's natural logarithm of positive normal float32 values: +, -, *, / and integer operations only."""
    x = np.asarray(x, dtype=F)
    bits = x.view(np.uint32)
    e = (bits >> np.uint32(23)).astype(np.int32) - 127
    m = ((bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(F)
    big = m > SQRT2
    m = np.where(big, m * F(0.5), m).astype(F)
    e = e + big.astype(np.int32)
    f = m - F(1.0)
    s = f / (F(2.0) + f)
    z = s * s
    p = C9 * z + C7
    p = p * z + C5
    p = p * z + C3
    p = p * z
    s2 = s + s
    lm = s2 + s2 * p
    ef = e.astype(F)
    out = ef * LN2_HI + (ef * LN2_LO + lm)
    assert out.dtype == F
    return out


def unit_of_r(r):
    """u = (2 r + 1) 2^-24: exact in float32, in (0, 1)."""
    return (np.asarray(r, dtype=np.uint32) * np.uint32(2) + np.uint32(1)).astype(F) * F(2.0 ** -24)


def gumbel_of_r(r):
    return -log32(-log32(unit_of_r(r)))


def noise(seed, streams, items):
    """g [len(streams), len(items)] f32: the standard Gumbel noise of every (stream, item) pair under `seed`."""
    k0, k1 = row_keys(seed, streams)
    return gumbel_of_r(hash_r(k0[:, None], k1[:, None], np.asarray(items, dtype=np.uint32)[None, :]))


def inv_temperature(temperature):
    return F(1.0) / F(temperature)


def keys_of(scores, inv_t, g):
    """fl(fl(score * inv_t) + g), the two operations rounded separately."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(scores, dtype=F) * F(inv_t)
        return (t + np.asarray(g, dtype=F)).astype(F)


def sampled_expectation(scores, excluded, k, inv_t, g):
    """One row: scores, g [num_items] f32 -> (items [k] u32, scores [k] f32 — the plain scores of those items, -inf for padding —,
    keys [k] f32, descending)."""
    scores = np.asarray(scores, dtype=F)
    items, keys = topk_expectation(keys_of(scores, inv_t, g), excluded, k)
    plain = np.full(k, -np.inf, dtype=F)
    real = items != NO_ITEM
    plain[real] = scores[items[real]]
    return items, plain, keys


def sampled_expect(scores, excl, k, temperature, seed, streams=None):
    """Every row of scores [rows, num_items]; excl: one list per row or None; streams default to the row index."""
    scores = np.asarray(scores, dtype=F)
    n, num_items = scores.shape
    streams = np.arange(n, dtype=np.uint64) if streams is None else np.asarray(streams, dtype=np.uint64)
    g = noise(seed, streams, np.arange(num_items, dtype=np.uint32))
    inv_t = inv_temperature(temperature)
    rows = [sampled_expectation(scores[u], () if excl is None else excl[u], k, inv_t, g[u]) for u in range(n)]
    return tuple(np.array([r[j] for r in rows], dt).reshape(-1, k) for j, dt in ((0, np.uint32), (1, F), (2, F)))


def oracle_recommend_sampled(o, num_items, ptr, item_ids, k, temperature, seed, streams=None, include_history=False, users=None):
    """The oracle's answer for the users `users` (default: all), built like recommend_expect.oracle_recommend: the oracle's
    representation of each history and its predict over every item, then sampled_expectation with the whole history excluded
    unless include_history.  streams: one per user of `users` (default: the position in `users`)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    users = list(range(len(ptr) - 1) if users is None else users)
    all_items = np.arange(num_items, dtype=np.uint32)
    streams = np.arange(len(users), dtype=np.uint64) if streams is None else np.asarray(streams, dtype=np.uint64)
    g = noise(seed, streams, all_items)
    inv_t = inv_temperature(temperature)
    rows = []
    for j, u in enumerate(users):
        h = np.asarray(item_ids[ptr[u]: ptr[u + 1]], dtype=np.uint32)
        s = o.predict(o.user_representation(h), all_items)
        rows.append(sampled_expectation(s, () if include_history else np.unique(h), k, inv_t, g[j]))
    return tuple(np.array([r[j] for r in rows], dt).reshape(-1, k) for j, dt in ((0, np.uint32), (1, F), (2, F)))
