"""The contract of sbr_sessions_beam_search (BEAM SEARCH in include/sbr_hip.h) a second time, in numpy, over rollout_expect's two
callables:

    rep(history) -> h              the oracle's user_representation of a list of item ids (the empty list: the empty history)
    scores(h) -> f32 [num_items]   the oracle's predict of h over every item

A beam's offers are recommend_expect's top-W over what it may still see, its (shift, mass) partition_expect's partition_row, and
its lp / cum the contract's f32 chain with sampled_expect's log32; the row keeps the W best offers by (cum descending, parent
ascending, position ascending), a plain sort.  The oracle windows a history to max_sequence_length where a session keeps the whole
recurrence, so this is the truth only while len(history) + steps <= max_sequence_length."""
from __future__ import annotations

import numpy as np

from partition_expect import allowed_mask, frac_bits, inv_temperature, partition_row
from recommend_expect import NO_ITEM, topk_expectation
from sampled_expect import log32

F = np.float32


def log_mass(mass: int, fbits: int):
    """L = log32(x), x = f32(mass >> s) 2^(s - F), s = max(0, bit_length(mass) - 24): exact, x >= 1 for mass >= 2^F."""
    mass = int(mass)
    s = max(0, mass.bit_length() - 24)
    x = F(np.ldexp(F(mass >> s), s - int(fbits)))
    return F(log32(np.array([x], dtype=F))[0])


def step_log_prob(score, shift, L, temperature):
    """lp = fl(fl(fl(score * inv_t) - shift) - L), each operation rounded once in f32."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = F(F(score) * inv_temperature(temperature))
        d = F(t - F(shift))
        return F(d - F(L))


class Expected:
    """items u32 / scores f32 / step_lp f32 / shift f32 / mass u64 [n, W, steps], cum f32 [n, W], lengths / beams u32 [n]"""

    def __init__(self, n, w, steps):
        shape = (n, w, steps)
        self.items = np.full(shape, NO_ITEM, dtype=np.uint32)
        self.scores = np.full(shape, -np.inf, dtype=F)
        self.step_lp = np.full(shape, -np.inf, dtype=F)
        self.shift = np.full(shape, -np.inf, dtype=F)
        self.mass = np.zeros(shape, dtype=np.uint64)
        self.cum = np.full((n, w), -np.inf, dtype=F)
        self.lengths = np.full(n, steps, dtype=np.uint32)
        self.beams = np.zeros(n, dtype=np.uint32)


def beam_row(rep, scores, history, steps, w, x0, temperature, *, allow_repeats=False):
    """One row.  x0: bool [num_items], the row's X_0.  Returns (beams, length): the live beams at the last real step in selection
    order, each a dict with path / scores / lp / shift / mass (lists over the real steps) and cum, and the real steps."""
    hist = [int(x) for x in history]
    fb = frac_bits(x0.size)
    beams = [dict(path=[], scores=[], lp=[], shift=[], mass=[], cum=F(0.0))]
    for j in range(steps):
        offers = []
        for p, b in enumerate(beams):
            ok = np.array(x0, dtype=bool)
            if not allow_repeats:
                ok[b["path"]] = False
            if not ok.any():
                continue
            s = np.asarray(scores(rep(hist + b["path"])), dtype=F)
            barred = np.flatnonzero(~ok)
            it, sc = topk_expectation(s, barred, w)
            shift, mass = partition_row(s, barred, temperature)
            L = log_mass(mass, fb)
            for q in range(w):
                if it[q] == NO_ITEM:
                    break
                lp = step_log_prob(sc[q], shift, L, temperature)
                offers.append((F(b["cum"] + lp), p, q, int(it[q]), F(sc[q]), lp, F(shift), int(mass)))
        if not offers:
            return beams if j else [], j
        offers.sort(key=lambda o: (-float(o[0]), o[1], o[2]))
        beams = [dict(path=beams[p]["path"] + [item], scores=beams[p]["scores"] + [sc], lp=beams[p]["lp"] + [lp],
                      shift=beams[p]["shift"] + [shift], mass=beams[p]["mass"] + [mass], cum=cum)
                 for cum, p, q, item, sc, lp, shift, mass in offers[:w]]
    return beams, steps


def beam_expect(rep, scores, num_items, histories, steps, w, temperature, excl=None, *, tags=None, any_of=None, none_of=None,
                allow_repeats=False) -> Expected:
    """Every row.  excl: one list per row or None (a row's X_0 with the seen-item memory: its list holds the remembered items);
    any_of / none_of: None, one mask or one per row (with tags [num_items])."""
    n = len(histories)
    exp = Expected(n, w, steps)

    def per_row(mk):
        return np.broadcast_to(np.asarray(0 if mk is None else mk, dtype=np.uint32), (n,))

    a, z = per_row(any_of), per_row(none_of)
    for i in range(n):
        x0 = allowed_mask(num_items, () if excl is None else excl[i], tags, int(a[i]), int(z[i]))
        beams, length = beam_row(rep, scores, histories[i], steps, w, x0, temperature, allow_repeats=allow_repeats)
        exp.lengths[i] = length
        exp.beams[i] = len(beams)
        for b, bm in enumerate(beams):
            m = len(bm["path"])
            exp.items[i, b, :m] = bm["path"]
            exp.scores[i, b, :m] = bm["scores"]
            exp.step_lp[i, b, :m] = bm["lp"]
            exp.shift[i, b, :m] = bm["shift"]
            exp.mass[i, b, :m] = bm["mass"]
            exp.cum[i, b] = bm["cum"]
    return exp
