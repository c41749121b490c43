"""The expectation of log_partition, stated a second time from the contract (include/sbr_hip.h PARTITION) alone, in
numpy: float32 element-wise +, -, * each rounded once, integer shifts, and Python / uint64 integer sums.

    inv_t = fl(1 / T);  t_i = fl(s_i * inv_t);  shift = max over allowed i of t_i  (-inf: nothing allowed; a zero is +0.0)
    d_i = fl(t_i - shift);  w_i = 0 if d_i > 0 or d_i < -64 (or not a number), else fix_F(exp32(d_i))
    mass = sum over allowed i of w_i  (u64);  log_z = shift + log(mass / 2^F)  (float64)

It shares no code with the product."""
from __future__ import annotations

import numpy as np

F = np.float32
LOG2E = F(1.44269504)
MAGIC = F(12582912.0)  # 1.5 * 2^23: adding and subtracting it rounds to the nearest integer
LN2_HI = F(0.693359375)
LN2_LO = F(-2.12194440e-4)
C2, C3, C4, C5, C6 = F(1.0 / 2.0), F(1.0 / 6.0), F(1.0 / 24.0), F(1.0 / 120.0), F(1.0 / 720.0)
D_MIN = F(-64.0)


def exp32(d):
    """The contract's exponential of float32 values in [-64, 0]: n = round(d log2 e), r = d - n ln 2 in two pieces, the degree-6
    Taylor polynomial of e^r in Horner form, times 2^n built from its exponent bits."""
    d = np.asarray(d, dtype=F)
    n = (d * LOG2E + MAGIC) - MAGIC
    r = (d - n * LN2_HI) - n * LN2_LO
    p = C6 * r + C5
    p = p * r + C4
    p = p * r + C3
    p = p * r + C2
    p = p * r + F(1.0)
    p = p * r + F(1.0)
    scale = ((n.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(F)
    out = p * scale
    assert out.dtype == F
    return out


def frac_bits(num_items: int) -> int:
    return min(40, 63 - int(num_items).bit_length())


def fix(x, fbits: int):
    """floor(x * 2^fbits) of positive normal float32 values as uint64, by shifting the 24-bit significand."""
    bits = np.asarray(x, dtype=F).view(np.uint32).astype(np.int64)
    e = bits >> 23 & 0xFF
    m = (bits & 0x7FFFFF) | 0x800000
    sh = e - 150 + int(fbits)
    left = m << np.clip(sh, 0, 39)
    right = m >> np.clip(-sh, 0, 24)
    out = np.where(sh >= 0, left, right)
    return np.where(e == 0, 0, out).astype(np.uint64)


def inv_temperature(temperature):
    return F(1.0) / F(temperature)


def weights(scores, temperature, shift, fbits: int):
    """w of plain scores (any shape) against a row's shift (broadcast)."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(scores, dtype=F) * inv_temperature(temperature)
        d = (t - np.asarray(shift, dtype=F)).astype(F)
    live = (d <= 0) & (d >= D_MIN)
    w = fix(exp32(np.where(live, d, F(0.0))), fbits)
    return np.where(live, w, np.uint64(0)).astype(np.uint64)


def allowed_mask(num_items: int, excluded, tags=None, any_of=0, none_of=0):
    ok = np.ones(num_items, dtype=bool)
    ex = np.asarray(list(excluded), dtype=np.int64)
    ok[ex[ex < num_items]] = False
    if tags is not None:
        tags = np.asarray(tags, dtype=np.uint32)
        ok &= (tags & np.uint32(none_of)) == 0
        if any_of:
            ok &= (tags & np.uint32(any_of)) != 0
    return ok


def partition_row(scores, excluded, temperature, tags=None, any_of=0, none_of=0):
    """One row: (shift f32, mass int)."""
    scores = np.asarray(scores, dtype=F)
    ok = allowed_mask(scores.size, excluded, tags, any_of, none_of)
    if not ok.any():
        return F(-np.inf), 0
    t = scores[ok] * inv_temperature(temperature)
    shift = F(t.max()) + F(0.0)
    w = weights(scores[ok], temperature, shift, frac_bits(scores.size))
    return shift, int(w.sum(dtype=np.uint64))  # fewer than 2^(63 - F) weights of at most 2^F each: no wrap


def partition_expect(scores, excl, temperature, tags=None, any_of=None, none_of=None):
    """Every row of scores [rows, num_items] -> (shift [rows] f32, mass [rows] u64).  excl: one list per row or None; any_of /
    none_of: None, one mask or one per row (with tags [num_items])."""
    scores = np.asarray(scores, dtype=F)
    n = scores.shape[0]

    def per_row(mk):
        return np.broadcast_to(np.asarray(0 if mk is None else mk, dtype=np.uint32), (n,))

    a, z = per_row(any_of), per_row(none_of)
    rows = [partition_row(scores[u], () if excl is None else excl[u], temperature, tags, int(a[u]), int(z[u])) for u in range(n)]
    return np.array([r[0] for r in rows], dtype=F), np.array([r[1] for r in rows], dtype=np.uint64)


def log_z_expect(shift, mass, fbits: int):
    with np.errstate(divide="ignore"):
        return np.asarray(shift, dtype=np.float64) + np.log(np.asarray(mass, dtype=np.float64) / 2.0 ** fbits)


def slate_log_prob_expect(scores, temperature, shift, mass, fbits: int):
    """Plackett-Luce conditional log-probabilities of draws in draw order: scores [rows, k] plain scores (-inf: padding).
    log(w_j) - log(mass - sum_{l<j} w_l), the remaining mass an exact integer; NaN for padding or w_j == 0."""
    scores = np.asarray(scores, dtype=F)
    out = np.full(scores.shape, np.nan, dtype=np.float64)
    for u in range(scores.shape[0]):
        w = weights(scores[u], temperature, F(shift[u]), fbits)
        rest = int(mass[u])
        for j in range(scores.shape[1]):
            wj = int(w[j])
            if np.isneginf(scores[u, j]) or wj == 0:
                continue
            if rest > 0:
                out[u, j] = np.log(float(wj)) - np.log(float(rest))
            rest -= wj
    return out
