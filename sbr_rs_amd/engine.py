"""Thin object layer over the C-ABI (include/sbr_hip.h).  Mirrors oracle/oracle.py's shape so
parity tests read symmetrically, but talks only to libsbr_hip.so."""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._abi import NUM_KERNEL_FAMILIES, KernelFamily, SbrGuardReport, SbrHparams, Status, storage_dim
from .errors import EngineError, FittingError, InvalidArgument, PredictionError


RECOMMEND_MAX_K = 1024  # SBR_RECOMMEND_MAX_K
RECOMMEND_INCLUDE_HISTORY = 1  # SBR_RECOMMEND_INCLUDE_HISTORY
RANK_INCLUDE_HISTORY = 1  # SBR_RANK_INCLUDE_HISTORY
RECOMMEND_NO_ITEM = 0xFFFFFFFF  # item id of a padding entry (its score is -inf)
SIMILAR_COSINE = 0  # SBR_SIMILAR_COSINE
SIMILAR_DOT = 1  # SBR_SIMILAR_DOT
SIMILAR_INCLUDE_SELF = 1  # SBR_SIMILAR_INCLUDE_SELF
RECOMMEND_INCLUDE_HISTORY = 1  # SBR_RECOMMEND_INCLUDE_HISTORY
SESSIONS_MAX_SEEN = 1024  # SBR_SESSIONS_MAX_SEEN
_SIMILAR_METRICS = {"cosine": SIMILAR_COSINE, "dot": SIMILAR_DOT}
NO_GROUP = 0xFFFFFFFF  # SBR_NO_GROUP: an item of no group, never capped


def _check(st: int):
    if st == Status.OK:
        return
    msg = _lib.load().sbr_status_string(st).decode()
    if st == Status.NO_INTERACTIONS:
        raise FittingError.NoInteractions(msg)
    if st == Status.INVALID_PREDICTION:
        raise PredictionError.InvalidPredictionValue(msg)
    raise EngineError(Status(st), msg)


def _similar_metric(metric) -> int:
    """"cosine" / "dot", or the C value as it is (the library refuses an unknown one)"""
    if isinstance(metric, str):
        if metric not in _SIMILAR_METRICS:
            raise ValueError(f"metric {metric!r}: 'cosine' or 'dot'")
        return _SIMILAR_METRICS[metric]
    return int(metric) & 0xFFFFFFFF


def _exclusion_csr(exclude, nu: int):
    """One sequence of item ids per user -> (ptr u64 [nu + 1], items u32, never empty: a one-element dummy stands in for no
    items at all); (None, None) for exclude = None."""
    if exclude is None:
        return None, None
    if len(exclude) != nu:
        raise ValueError("one exclusion list per user")
    lists = [np.asarray(e, dtype=np.uint32).ravel() for e in exclude]
    ep = np.zeros(nu + 1, dtype=np.uint64)
    ep[1:] = np.cumsum([x.size for x in lists])
    ei = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0, np.uint32), dtype=np.uint32)
    if ei.size == 0:
        ei = np.zeros(1, dtype=np.uint32)
    return ep, ei


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _tag_masks(any_of, none_of, nu: int):
    """The mask keywords of a filtered call -> None when both are None (the plain entry point is called), else (any_of, none_of) as
    u32 [nu] arrays: a scalar applies to every user, None is all zeros, an array must have one entry per user."""
    if any_of is None and none_of is None:
        return None

    def one(mask, name):
        if mask is None:
            return np.zeros(max(nu, 1), dtype=np.uint32)
        a = np.asarray(mask)
        if a.ndim == 0:
            return np.full(max(nu, 1), int(a) & 0xFFFFFFFF, dtype=np.uint32)
        a = np.ascontiguousarray(a.ravel(), dtype=np.uint32)
        if a.size != nu:
            raise ValueError(f"{name}: one mask per user ({nu}), or a scalar; got {a.size}")
        return a if nu else np.zeros(1, dtype=np.uint32)

    return one(any_of, "any_of"), one(none_of, "none_of")


def _sample_args(temperature, seed, streams, n: int):
    """The noise keywords of a *_sampled call -> (SbrSampleArgs, the array it points into, kept alive by the caller).  streams: None
    (the library's default: the row's index, or a session's slot id) or one u64 per row."""
    from ._abi import SbrSampleArgs

    sa = SbrSampleArgs()
    sa.temperature = float(np.float32(temperature))
    sa.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    st = None
    if streams is not None:
        st = np.ascontiguousarray(np.asarray(streams).ravel(), dtype=np.uint64)
        if st.size != n:
            raise ValueError(f"streams: one per row ({n}); got {st.size}")
        if n == 0:
            st = np.zeros(1, dtype=np.uint64)
        sa.streams = st.ctypes.data
    return sa, st


def softmax_frac_bits(num_items: int) -> int:
    """F of a catalogue of num_items (sbr_softmax_frac_bits): min(40, 63 - bit_length(num_items)).  Needs no device."""
    return int(_lib.load().sbr_softmax_frac_bits(int(num_items) & 0xFFFFFFFF))


def softmax_weights(scores, temperature, shift, frac_bits: int) -> np.ndarray:
    """The fixed-point softmax weights w (u64, the shape of ``scores``) of plain scores against a row's ``shift`` — one shift, or an
    array that broadcasts against the scores' leading axes — by sbr_softmax_weights_rows, one call over all the rows of
    sbr_softmax_weights, the library's one host statement of the t / d / exp32 / fix_F chain.  Needs no device."""
    sc = np.ascontiguousarray(scores, dtype=np.float32)
    w = np.zeros(sc.shape, dtype=np.uint64)
    if sc.size == 0:
        return w
    rows_s = sc.reshape(-1, sc.shape[-1]) if sc.ndim > 1 else sc.reshape(1, -1)
    shifts = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, dtype=np.float32).reshape(-1, 1) if np.ndim(shift) else np.float32(shift),
                                                  (rows_s.shape[0], 1)).ravel())
    _check(_lib.load().sbr_softmax_weights_rows(_ptr(rows_s), rows_s.shape[0], rows_s.shape[1], float(np.float32(temperature)), _ptr(shifts),
                                                int(frac_bits), _ptr(w)))
    return w


class Partition:
    """What the log_partition calls return: per row the ``shift`` (f32 [U], the largest score / T over the items the row may see),
    the fixed-point ``mass`` (u64 [U], the sum of the items' weights w = floor(exp32(score / T - shift) 2^frac_bits)) and the
    catalogue's ``frac_bits``; ``log_z`` (f64 [U]) = shift + log(mass / 2^frac_bits), -inf for a row that may see nothing.  The
    model's probability of an item is w / mass."""

    def __init__(self, temperature, shift, mass, frac_bits: int):
        self.temperature = float(np.float32(temperature))
        self.shift, self.mass, self.frac_bits = shift, mass, int(frac_bits)

    @property
    def log_z(self) -> np.ndarray:
        with np.errstate(divide="ignore"):
            return self.shift.astype(np.float64) + np.log(self.mass.astype(np.float64) / 2.0 ** self.frac_bits)

    def _weights(self, scores):
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        if sc.ndim != 2 or sc.shape[0] != self.shift.size:
            raise ValueError(f"scores: [{self.shift.size}, m] plain scores, one row per row of the partition")
        return sc, softmax_weights(sc, self.temperature, self.shift, self.frac_bits)

    def log_prob(self, scores) -> np.ndarray:
        """log(w / mass), f64 [U, m], of items with the plain ``scores`` [U, m] (score_candidates' or a recommend call's): the
        log-probability that one draw from the row's softmax is that item; -inf where w == 0."""
        _, w = self._weights(scores)
        live = w != 0  # then the row's mass is not 0 either, for a partition taken with the items' exclusions and masks
        with np.errstate(divide="ignore", invalid="ignore"):
            lp = np.log(w.astype(np.float64)) - np.log(self.mass.astype(np.float64))[:, None]
        return np.where(live, lp, -np.inf)

    def slate_log_prob(self, scores) -> np.ndarray:
        """The Plackett-Luce conditional log-probabilities, f64 [U, k], of draws without replacement with the plain ``scores``
        [U, k] in draw order, as recommend_sampled returns them: log(w_j) - log(mass - sum of the w before j), the remaining mass
        an exact integer.  NaN at padding (-inf score) and where w_j == 0.  Meaningful only for a partition taken with the draws'
        exclusions and masks."""
        sc, w = self._weights(scores)
        before = np.zeros(w.shape, dtype=np.uint64)
        if w.shape[1] > 1:
            before[:, 1:] = np.cumsum(w[:, :-1], axis=1, dtype=np.uint64)
        enough = before < self.mass[:, None]
        rest = np.where(enough, self.mass[:, None] - np.where(enough, before, np.uint64(0)), np.uint64(1))
        out = np.log(np.maximum(w, np.uint64(1)).astype(np.float64)) - np.log(rest.astype(np.float64))
        out[~enough | (w > rest) | (w == 0) | np.isneginf(sc)] = np.nan  # a slate that overdraws its partition has no probability
        return out


def _partition_outputs(n: int):
    return np.zeros(max(n, 1), dtype=np.float32)[:n], np.zeros(max(n, 1), dtype=np.uint64)[:n], C.c_uint32(0)


ROLLOUT_MODES = ("greedy", "sample")


class Rollout:
    """What ``Sessions.rollout`` returns: ``items`` u32 [n, steps] and ``scores`` f32 [n, steps] — row i's picks in pick order with
    their plain scores, (0xFFFFFFFF, -inf) from the step at which the row had nothing left to choose from — and ``lengths`` u32 [n],
    the real steps of each row.  ``keys`` f32 [n, steps]: the winning keys of a sampled rollout, else None.  With ``log_prob``:
    ``shift`` f32 / ``mass`` u64 [n, steps] and ``frac_bits``, each step's ``log_partition`` over what the row could still see, and
    ``log_prob`` f64 [n, steps] = ``Partition.log_prob`` of the pick on them (NaN at padding); else None.  With ``final_state``:
    ``h``, ``c`` (None for EWMA) and ``len``, in ``Sessions.state``'s format, after all picks; else None."""

    def __init__(self, items, scores, lengths, keys=None, shift=None, mass=None, frac_bits=None, log_prob=None, h=None, c=None, len=None):
        self.items, self.scores, self.lengths, self.keys = items, scores, lengths, keys
        self.shift, self.mass, self.frac_bits, self.log_prob = shift, mass, frac_bits, log_prob
        self.h, self.c, self.len = h, c, len

    def rows(self):
        """Each row's real picks, one u32 array per row: what ``Sessions.append(slots, rollout.rows())`` makes happen."""
        return [self.items[i, : int(n)].copy() for i, n in enumerate(self.lengths)]


def _rollout_args(steps, mode, temperature):
    """The checks of a rollout that need no library: steps, mode, temperature -> (steps, sample)."""
    from ._abi import ROLLOUT_MAX_STEPS

    if mode not in ROLLOUT_MODES:
        raise ValueError(f"mode {mode!r}: 'greedy' or 'sample'")
    if isinstance(steps, bool) or int(steps) != steps or not 1 <= int(steps) <= ROLLOUT_MAX_STEPS:
        raise ValueError(f"steps: 1..{ROLLOUT_MAX_STEPS}; got {steps!r}")
    t = np.float32(temperature)
    with np.errstate(divide="ignore", over="ignore"):
        inv = np.float32(1.0) / t
    if not (np.isfinite(t) and t > 0 and np.isfinite(inv) and inv != 0):
        raise ValueError(f"temperature: finite and > 0, with a finite f32 reciprocal; got {temperature!r}")
    return int(steps), mode == "sample"


class Beams:
    """What ``Sessions.beam_search`` returns, beams in selection order at each row's last real step: ``items`` u32 / ``scores`` f32
    [n, W, steps] — beam b's path and each pick's plain score against the beam's state at that step — ``step_log_probs`` f32 [n, W,
    steps], the contract's lp of each pick, and ``log_probs`` f32 [n, W], the beam's cum; padding (0xFFFFFFFF, -inf), -inf in both
    log-probabilities.  ``lengths`` u32 [n]: the real steps of each row; ``beams`` u32 [n]: its live beams (fewer than W while the
    distinct paths are fewer).  With ``partitions``: ``shift`` f32 / ``mass`` u64 [n, W, steps] and ``frac_bits``, each step's
    ``log_partition`` of the beam (-inf / 0 at padding); else None."""

    def __init__(self, items, scores, step_log_probs, log_probs, lengths, beams, shift=None, mass=None, frac_bits=None):
        self.items, self.scores, self.step_log_probs, self.log_probs = items, scores, step_log_probs, log_probs
        self.lengths, self.beams = lengths, beams
        self.shift, self.mass, self.frac_bits = shift, mass, frac_bits

    def best(self):
        """Beam 0 of every row, u32 [n, steps]: the most likely continuation found."""
        return self.items[:, 0, :].copy()

    def rows(self, b: int = 0):
        """Beam b's real picks of each row, one u32 array per row (empty where the row has fewer than b + 1 beams): what
        ``Sessions.append(slots, beams.rows(b))`` makes happen."""
        return [self.items[i, b, : int(n)].copy() if b < int(k) else np.zeros(0, np.uint32)
                for i, (n, k) in enumerate(zip(self.lengths, self.beams))]


def _beam_args(steps, width, temperature):
    """The checks of a beam search that need no library: steps, width, temperature -> (steps, width)."""
    from ._abi import BEAM_MAX_WIDTH, ROLLOUT_MAX_STEPS

    if isinstance(steps, bool) or int(steps) != steps or not 1 <= int(steps) <= ROLLOUT_MAX_STEPS:
        raise ValueError(f"steps: 1..{ROLLOUT_MAX_STEPS}; got {steps!r}")
    if isinstance(width, bool) or int(width) != width or not 1 <= int(width) <= BEAM_MAX_WIDTH:
        raise ValueError(f"width: 1..{BEAM_MAX_WIDTH}; got {width!r}")
    _rollout_args(1, "greedy", temperature)
    return int(steps), int(width)


ABOVE_MAX_RESULTS = 1 << 24  # the *_above calls' default max_results: the entries of the one buffer they call with
ABOVE_ORDERS = ("score", "id")


def above_sort(ptr, ids, scores, order: str = "score"):
    """The rows of a CSR result (ptr u64 [R + 1], ids u32, scores f32, each row in ascending id order, as the library returns it) in
    ``order``: "id" as they are, "score" by score descending with ties to the lower id — a stable sort on top of the id order, the
    total order every top-k call uses (-0.0 and +0.0 tie).  Returns (ids, scores)."""
    if order not in ABOVE_ORDERS:
        raise ValueError(f"order {order!r}: 'score' or 'id'")
    ids, scores = np.asarray(ids, dtype=np.uint32), np.asarray(scores, dtype=np.float32)
    if order == "id" or ids.size == 0:
        return ids, scores
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(np.asarray(ptr, dtype=np.uint64)).astype(np.int64))
    at = np.lexsort((-scores, rows))  # stable: equal (row, score) keep their id order
    return ids[at], scores[at]


class Above:
    """What the *_above and *_top calls return, a CSR set of (row, id, score) pairs: ``ptr`` u64 [R + 1], ``ids`` u32 [N], ``scores``
    f32 [N]; row i's pairs are entries ptr[i] .. ptr[i + 1], in the call's ``order``.  ``counts`` u64 [R] = diff(ptr).  ``cuts``:
    f32 [R] from a *_top call (the score of a row's last entry; -inf where the row holds everything eligible, +inf for n = 0),
    None from an *_above call."""

    def __init__(self, ptr, ids, scores, order: str = "score", cuts=None):
        self.ptr, self.ids, self.scores, self.order, self.cuts = ptr, ids, scores, order, cuts

    @property
    def counts(self) -> np.ndarray:
        return np.diff(self.ptr)

    def __len__(self) -> int:
        return len(self.ptr) - 1

    def row(self, i: int):
        """(ids, scores) of row i"""
        a, b = int(self.ptr[i]), int(self.ptr[i + 1])
        return self.ids[a:b], self.scores[a:b]

    def pairs(self):
        """(row index i64 [N], id u32 [N], score f32 [N]), row-major"""
        return np.repeat(np.arange(len(self), dtype=np.int64), self.counts.astype(np.int64)), self.ids, self.scores


def _above_thresholds(threshold, n: int) -> np.ndarray:
    """``threshold`` -> f32 [n]: a scalar applies to every row, an array must have one value per row; a NaN is refused"""
    t = np.asarray(threshold, dtype=np.float32)
    t = np.full(n, t, dtype=np.float32) if t.ndim == 0 else np.ascontiguousarray(t.ravel())
    if t.size != n:
        raise ValueError(f"threshold: one per row ({n}), or a scalar; got {t.size}")
    if np.isnan(t).any():
        raise ValueError("threshold: NaN")
    return t if n else np.zeros(1, dtype=np.float32)


def _top_budgets(budget, n: int) -> np.ndarray:
    """``budget`` (the n of a *_top call) -> u64 [rows]: a scalar applies to every row, an array must have one value per row; whole
    numbers from 0 to 2^64 - 1, so a NaN, a fraction, a negative value or a float of 2^64 and more (which no u64 holds) is refused"""
    b = np.asarray(budget)
    if b.dtype.kind not in "iuf" or (b.dtype.kind == "f" and not (np.isfinite(b).all() and (b == np.floor(b)).all())):
        raise ValueError("n: whole numbers >= 0")
    if (b < 0).any():
        raise ValueError("n: >= 0")
    if b.dtype.kind == "f" and (b >= 2.0 ** 64).any():
        raise ValueError("n: below 2^64 (any n past the eligible columns returns them all)")
    b = np.full(n, b, dtype=np.uint64) if b.ndim == 0 else np.ascontiguousarray(b.ravel()).astype(np.uint64)
    if b.size != n:
        raise ValueError(f"n: one per row ({n}), or a scalar; got {b.size}")
    return b if n else np.zeros(1, dtype=np.uint64)


def _above(call, n: int, threshold, max_results, order: str, count_only: bool, budget=None):
    """The shared tail of the *_above / count_above* methods.  ``call(thresholds, out_counts, out_total, capacity, out_ids, out_scores)``
    invokes the entry point with the method's leading arguments.  One call with a buffer of ``max_results`` entries (np.empty
    touches nothing); a total above it is a ValueError that states the total, never a truncated result.
    With ``budget`` (the *_top / nth_score* methods; threshold unused) the entry point is the *_top sibling, whose list differs in
    two places: n u64 [rows] where the thresholds stand and out_cuts ahead of out_counts, so ``call(n, out_cuts, out_counts, ...)``.
    count_only then returns (cuts, counts), and the Above carries the cuts."""
    if order not in ABOVE_ORDERS:
        raise ValueError(f"order {order!r}: 'score' or 'id'")
    cuts = None
    if budget is None:
        lead = (_ptr(_above_thresholds(threshold, n)),)
    else:
        cuts = np.zeros(max(n, 1), dtype=np.float32)
        lead = (_ptr(_top_budgets(budget, n)), _ptr(cuts))
    counts = np.zeros(max(n, 1), dtype=np.uint64)
    total = C.c_uint64(0)
    if count_only:
        _check(call(*lead, _ptr(counts), C.byref(total), 0, None, None))
        return counts[:n] if budget is None else (cuts[:n], counts[:n])
    cap = ABOVE_MAX_RESULTS if max_results is None else int(max_results)
    if cap < 0:
        raise ValueError("max_results: >= 0")
    ids = np.empty(max(cap, 1), dtype=np.uint32)
    scores = np.empty(max(cap, 1), dtype=np.float32)
    _check(call(*lead, _ptr(counts), C.byref(total), cap, _ptr(ids), _ptr(scores)))
    if total.value > cap:
        if budget is not None:
            raise ValueError(f"{total.value} pairs make up the rows' best n, above max_results = {cap}: raise max_results or lower n "
                             f"(nth_score* returns the per-row counts and cuts)")
        raise ValueError(f"{total.value} pairs pass the threshold, above max_results = {cap}: raise max_results or the threshold "
                         f"(count_above* returns the per-row counts)")
    ptr = np.zeros(n + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(counts[:n], dtype=np.uint64)
    ids, scores = above_sort(ptr, ids[: total.value].copy(), scores[: total.value].copy(), order)
    return Above(ptr, ids, scores, order, None if cuts is None else cuts[:n])


def capped_default_pool(k: int) -> int:
    """The pool of a *_capped call that names none: min(1 024, max(64, 4 k)), the library's default."""
    return min(RECOMMEND_MAX_K, max(64, 4 * int(k)))


def _cap_args(k, cap, pool):
    """The rule keywords of a *_capped call -> (SbrCapArgs, the pool it names); a ValueError, before any call into the library, for
    cap < 1, k < 1, pool < k or pool > 1 024."""
    from ._abi import SbrCapArgs

    k, cap = int(k), int(cap)
    pool = capped_default_pool(k) if pool is None else int(pool)
    if cap < 1 or cap > 0xFFFFFFFF:
        raise ValueError(f"cap {cap}: at least 1")
    if k < 1:
        raise ValueError(f"k {k}: at least 1")
    if pool < k:
        raise ValueError(f"pool {pool} < k {k}")
    if pool > RECOMMEND_MAX_K:
        raise ValueError(f"pool {pool} > {RECOMMEND_MAX_K}")
    ca = SbrCapArgs()
    ca.cap, ca.pool = cap, pool
    return ca, pool


def capped_keep(ids, groups, cap: int, k: int) -> np.ndarray:
    """The rule R(L, cap, k) of the *_capped calls on one row: ``ids`` are the row's items in the total order (no padding), ``groups``
    the u32 group word of every item of the catalogue.  Returns the positions in ``ids`` of the first k kept entries, ascending.  An
    entry is kept iff its group is NO_GROUP or its ordinal within its group, among the entries before it, is below cap — found
    with one stable sort by group, no walk."""
    ids = np.asarray(ids, dtype=np.int64)
    g = np.asarray(groups, dtype=np.uint32)[ids]
    n = g.size
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    by = np.argsort(g, kind="stable")
    gs = g[by]
    heads = np.flatnonzero(np.concatenate(([True], gs[1:] != gs[:-1])))
    run0 = np.repeat(heads, np.diff(np.concatenate((heads, [n]))))
    ordinal = np.empty(n, dtype=np.int64)
    ordinal[by] = np.arange(n, dtype=np.int64) - run0
    return np.flatnonzero((g == NO_GROUP) | (ordinal < int(cap)))[: int(k)]


def capped_complete(top, items, scores, complete, groups, cap: int, k: int, pool: int, num_items: int, max_results=None):
    """Finishes the rows a *_capped call returned incomplete, in place, and returns the number of ``top`` calls it made.
    ``top(rows, n)`` is the matching recommend_top* over those rows of the call only — same exclusions, masks and include_seen,
    order="score" — an ``Above`` (anything with ``row(i) -> (ids, scores)``).  n starts at 4 pool and grows fourfold per round up to
    num_items; the rule runs on the host over ``groups``; a row is done when k are kept or its returned row is shorter than n
    (everything eligible was seen).  The rows of a round go in batches whose rows x n stay within max_results (recommend_top's
    default).  Both routes carry predict's bits in the same order, so a finished row is what an unbounded pool would have given."""
    cap_results = ABOVE_MAX_RESULTS if max_results is None else int(max_results)
    todo = np.flatnonzero(~np.asarray(complete, dtype=bool))
    calls = 0
    n = 4 * int(pool)
    while todo.size:
        n = min(n, max(int(num_items), 1))
        per = max(1, cap_results // n)
        left = []
        for b0 in range(0, todo.size, per):
            rows = todo[b0 : b0 + per]
            res = top(rows, n)
            calls += 1
            for i, r in enumerate(rows):
                ids, sc = res.row(i)
                kept = capped_keep(ids, groups, cap, k)
                if kept.size < k and ids.size >= n and n < num_items:
                    left.append(r)
                    continue
                items[r, : kept.size], items[r, kept.size :] = ids[kept], RECOMMEND_NO_ITEM
                scores[r, : kept.size], scores[r, kept.size :] = sc[kept], -np.inf
                complete[r] = True
        todo = np.asarray(left, dtype=np.int64)
        n *= 4
    return calls


STREAM_ROLES = ("main", "side", "sorter", "copier", "xs")  # the roles SBR_TEST_STREAM_DELAY names, in the counter's order


def selftest_stream_delay(delay_us: int, with_join: bool) -> float:
    """sbr_selftest_stream_delay: what a stream reads of a float (1.0) that a stream late by ``delay_us`` sets to 2.0."""
    out = C.c_float()
    _check(_lib.load().sbr_selftest_stream_delay(int(delay_us), 1 if with_join else 0, C.byref(out)))
    return out.value


def guard_report(model=None) -> SbrGuardReport:
    """sbr_test_guard_report (SBR_TEST_GUARD): what the guard bands around the scratch cache's live blocks and, with ``model``, its
    arena's current carve show now, plus what the checks at put / carve found since the last report.  Reads and resets."""
    out = SbrGuardReport()
    _check(_lib.load().sbr_test_guard_report(None if model is None else model._h, C.byref(out)))
    return out


def selftest_guard(model, where: int, side: int):
    """sbr_selftest_guard: the reports of one byte set by the library just past (side > 0) or just before (side < 0) an
    allocation of kind ``where`` (GUARD_*), on the first and on the re-used allocation."""
    out = (SbrGuardReport * 2)()
    _check(_lib.load().sbr_selftest_guard(None if model is None else model._h, int(where), int(side), out))
    return out[0], out[1]


def device_info():
    L = _lib.load()
    name = C.create_string_buffer(64)
    cus, hbm = C.c_uint32(), C.c_uint64()
    _check(L.sbr_device_info(name, 64, C.byref(cus), C.byref(hbm)))
    return name.value.decode(), cus.value, hbm.value


def set_device(ordinal: int):
    _check(_lib.load().sbr_set_device(int(ordinal)))


def device_count() -> int:
    n = C.c_int32()
    _check(_lib.load().sbr_device_count(C.byref(n)))
    return n.value


GROUP_PARTITION_ITEM_TABLE = 1


def group_create(hp: SbrHparams, n: int, partition_item_table: bool = False):
    """The n replicas of a single-process group (sbr_group_create): replica r on HIP device r mod device
    count.  ``partition_item_table``: the item table exists once, row range r on replica r's device,
    mapped into every replica (BASELINE configs[4]); results equal the replicated group bit for bit."""
    import copy

    L = _lib.load()
    handles = (C.c_void_p * n)()
    _check(L.sbr_group_create(C.byref(hp), n, GROUP_PARTITION_ITEM_TABLE if partition_item_table else 0, handles))
    out = []
    for r in range(n):
        h = copy.copy(hp)
        h.num_devices, h.device_rank = n, r
        out.append(Model._from_handle(h, C.c_void_p(handles[r])))
    return out


def group_fit(models, user_ptr, item_ids) -> float:
    """Single-process multi-device fit (sbr_group_fit): models[r] built with num_devices = len(models),
    device_rank = r and the same seed.  ≙ fit with num_threads(n) in one process."""
    L = _lib.load()
    up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
    it = np.ascontiguousarray(item_ids, dtype=np.uint32)
    handles = (C.c_void_p * len(models))(*[m._h for m in models])
    loss = C.c_float()
    _check(L.sbr_group_fit(handles, len(models), _ptr(up), _ptr(it), len(up) - 1, C.byref(loss)))
    return loss.value


class GroupPlan:
    """sbr_group_fit taken apart (sbr_group_fit_begin .. sbr_group_fit_end): the single-process group's steps one at a time —
    the bench's ``--driver group`` and the parity tests of the multi-device step.  ``host_threads``: None = the library's
    default (one host thread per device from four devices on), True / False = force."""

    def __init__(self, models, user_ptr, item_ids, host_threads=None):
        self.models = list(models)
        self._L = _lib.load()
        self._up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        self._it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        handles = (C.c_void_p * len(self.models))(*[m._h for m in self.models])
        h = C.c_void_p()
        _check(self._L.sbr_group_fit_begin(handles, len(self.models), _ptr(self._up), _ptr(self._it), len(self._up) - 1, C.byref(h)))
        self._h = h
        if host_threads is not None:
            _check(self._L.sbr_group_plan_set_host_threads(self._h, 1 if host_threads else 0))
        self._members = {}

    def epoch_prepare(self, prefetch_next: bool = False) -> int:
        n = C.c_uint64()
        _check(self._L.sbr_group_epoch_prepare(self._h, C.byref(n), 1 if prefetch_next else 0))
        return n.value

    def step(self, mb: int):
        _check(self._L.sbr_group_step(self._h, mb))

    def step_local(self, mb: int):
        _check(self._L.sbr_group_step_local(self._h, mb))

    def member(self, r: int) -> "FitPlan":
        """Replica r's plan, borrowed from the group (debug_fetch, minibatch_rows, counters)."""
        if r not in self._members:
            h = C.c_void_p()
            _check(self._L.sbr_group_member_plan(self._h, r, C.byref(h)))
            self._members[r] = FitPlan._borrowed(self.models[r], h)
        return self._members[r]

    def synchronize(self):
        _check(self._L.sbr_group_synchronize(self._h))

    def set_exchange(self, gradient_all_gather: bool):
        """Synchronous, replicated: False (default) = owner-applied update, parameter slices gathered in place; True = rounds 1-5's
        gradient all-gather + whole-table update on every replica (sbr_group_plan_set_exchange).  Same bits."""
        _check(self._L.sbr_group_plan_set_exchange(self._h, 1 if gradient_all_gather else 0))

    def gather_optimizer_state(self):
        """Every replica's item-table optimiser state made complete from the owners' slices (fit end does it)."""
        _check(self._L.sbr_group_gather_optimizer_state(self._h))

    def stats(self):
        """(host ms spent queueing steps, steps, host threads in use)."""
        ms, n, th = C.c_double(), C.c_uint64(), C.c_int32()
        _check(self._L.sbr_group_plan_stats(self._h, C.byref(ms), C.byref(n), C.byref(th)))
        return ms.value, n.value, th.value

    def end(self) -> float:
        loss = C.c_float()
        h, self._h = self._h, None
        self._members = {}
        _check(self._L.sbr_group_fit_end(h, C.byref(loss)))
        return loss.value

    def close(self):
        if getattr(self, "_h", None):
            self._members = {}
            self._L.sbr_group_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL inside the library (sbr_comm_*): for hosts with one process per GPU and no collective library of their own.
    ``Comm.unique_id()`` on rank 0, the 128 bytes to every rank by any channel, ``Comm(id, world, rank)`` on every rank."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(_lib.load().sbr_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, uid: bytes, world: int, rank: int):
        if len(uid) != 128:
            raise ValueError("the id is 128 bytes")
        self._L = _lib.load()
        h = C.c_void_p()
        _check(self._L.sbr_comm_create((C.c_uint8 * 128)(*uid), world, rank, C.byref(h)))
        self._h, self.world, self.rank = h, world, rank

    def fit(self, model: "Model", user_ptr, item_ids) -> float:
        """This rank's whole fit through the library's own transport (sbr_model_fit_comm)."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        loss = C.c_float()
        _check(self._L.sbr_model_fit_comm(model._h, self._h, _ptr(up), _ptr(it), len(up) - 1, C.byref(loss)))
        return loss.value

    def step_exchange(self, plan: "FitPlan", mb: int):
        _check(self._L.sbr_fit_step_exchange(plan._h, mb, self._h))

    def gather_optimizer_state(self, model: "Model"):
        _check(self._L.sbr_comm_gather_optimizer_state(model._h, self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.sbr_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DBG_U32 = {1, 7, 8, 9}


class FitPlan:
    def __init__(self, model: "Model", user_ptr, item_ids):
        self.model = model
        self._L = _lib.load()
        self._up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        self._it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        h = C.c_void_p()
        _check(self._L.sbr_fit_begin(model._h, _ptr(self._up), _ptr(self._it), len(self._up) - 1, C.byref(h)))
        self._h = h

    @classmethod
    def _borrowed(cls, model: "Model", handle) -> "FitPlan":
        p = cls.__new__(cls)
        p.model, p._L, p._h, p._owned = model, _lib.load(), handle, False
        return p

    def epoch_prepare(self) -> int:
        n = C.c_uint64()
        _check(self._L.sbr_fit_epoch_prepare(self._h, C.byref(n)))
        return n.value

    def epoch_prefetch(self):
        _check(self._L.sbr_fit_epoch_prefetch(self._h))

    def minibatch_rows(self, mb: int) -> int:
        n = C.c_uint64()
        _check(self._L.sbr_fit_minibatch_rows(self._h, mb, C.byref(n)))
        return n.value

    def step(self, mb: int):
        _check(self._L.sbr_fit_step(self._h, mb))

    def steps(self, first: int, count: int):
        """``count`` consecutive optimiser steps (sbr_fit_steps): one-sequence steps at d <= 32 run as one launch per run."""
        _check(self._L.sbr_fit_steps(self._h, first, count))

    def phase_clocks(self):
        """Per-phase ticks (100 MHz) of the one-launch step runs since fit_begin: forward, score + tail, backward, dense, sparse; steps."""
        out = (C.c_uint64 * 6)()
        _check(self._L.sbr_fit_debug_phase_clocks(self._h, out))
        return list(out)

    def step_local(self, mb: int):
        _check(self._L.sbr_fit_step_local(self._h, mb))

    def step_apply(self, mb: int):
        _check(self._L.sbr_fit_step_apply(self._h, mb))

    # ---- multi-device owner-reduce protocol (device pointers supplied by the caller) ----
    def chunk_bytes(self) -> int:
        n = C.c_uint64()
        _check(self._L.sbr_fit_chunk_bytes(self._h, C.byref(n)))
        return n.value

    def dense_bytes(self) -> int:
        n = C.c_uint64()
        _check(self._L.sbr_fit_dense_bytes(self._h, C.byref(n)))
        return n.value

    def step_scatter(self, mb: int, send_ptr: int):
        _check(self._L.sbr_fit_step_scatter(self._h, mb, C.c_void_p(send_ptr)))

    def step_dense(self, dense_ptr: int):
        _check(self._L.sbr_fit_step_dense(self._h, C.c_void_p(dense_ptr)))

    def step_owner_reduce(self, recv_ptr: int, own_ptr: int, stream_ptr: int = None):
        """``stream_ptr``: launch on that HIP stream without synchronising it or the model's stream (the caller
        orders them) — the exchange stream of the staleness-one pipeline."""
        if stream_ptr is None:
            _check(self._L.sbr_fit_step_owner_reduce(self._h, C.c_void_p(recv_ptr), C.c_void_p(own_ptr)))
        else:
            _check(self._L.sbr_fit_step_owner_reduce_on(self._h, C.c_void_p(recv_ptr), C.c_void_p(own_ptr), C.c_void_p(stream_ptr)))

    def step_apply_table(self, table_ptr: int, dense_all_ptr: int):
        _check(self._L.sbr_fit_step_apply_table(self._h, C.c_void_p(table_ptr), C.c_void_p(dense_all_ptr)))

    def step_apply_rows(self, table_ptr: int):
        """Item-table half of step_apply_table (opens the optimiser step; does not wait for the dense-gradient GEMM)."""
        _check(self._L.sbr_fit_step_apply_rows(self._h, C.c_void_p(table_ptr)))

    def step_apply_dense(self, dense_all_ptr: int):
        _check(self._L.sbr_fit_step_apply_dense(self._h, C.c_void_p(dense_all_ptr)))

    def step_owner_update(self, recv_ptr: int):
        """Owner-applied update (sbr_fit_step_owner_update): device-order sum of the devices' contributions to this rank's slice and
        the one optimiser update of its touched rows, in place; opens the optimiser step."""
        _check(self._L.sbr_fit_step_owner_update(self._h, C.c_void_p(recv_ptr)))

    def end(self):
        loss, ex = C.c_float(), C.c_uint64()
        _check(self._L.sbr_fit_end(self._h, C.byref(loss), C.byref(ex)))
        return loss.value, ex.value

    def end_lagged(self) -> float:
        """This device's term of the figure the reference's ``fit`` returns (stale loss-node values, sequence_model.rs:157)."""
        v = C.c_float()
        _check(self._L.sbr_fit_end_lagged(self._h, C.byref(v)))
        return v.value

    def counters(self):
        ex, neg = C.c_uint64(), C.c_uint64()
        _check(self._L.sbr_fit_counters(self._h, C.byref(ex), C.byref(neg)))
        return ex.value, neg.value

    def sparse_stats(self):
        """(gradient entries, distinct table rows) of the last step's sparse update on this device."""
        ent, uniq = C.c_uint64(), C.c_uint64()
        _check(self._L.sbr_fit_sparse_stats(self._h, C.byref(ent), C.byref(uniq)))
        return ent.value, uniq.value

    def debug_fetch(self, which: int, rows: int) -> np.ndarray:
        d = self.model.storage_dim
        which = int(which)
        if which in (0, 4, 5):
            out = np.zeros((rows, d), dtype=np.float32)
        elif which == 6:
            out = np.zeros(self.model.dense_count(), dtype=np.float32)
        elif which == 10:
            out = np.zeros((rows, {0: 4, 1: 3, 2: 0}[int(self.model.hp.model)] * d), dtype=np.float32)
        else:
            out = np.zeros(rows, dtype=np.uint32 if which in _DBG_U32 else np.float32)
        _check(self._L.sbr_fit_debug_fetch(self._h, which, _ptr(out), out.nbytes))
        return out

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                self._L.sbr_fit_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """Owns one sbr_model handle (device-resident parameters)."""

    def __init__(self, hp: SbrHparams):
        self._L = _lib.load()
        self.hp = hp
        self.dim = int(hp.embedding_dim)
        h = C.c_void_p()
        _check(self._L.sbr_model_create(C.byref(hp), C.byref(h)))  # rejects an embedding_dim outside 1..256
        self._h = h
        self.storage_dim = storage_dim(self.dim)

    @classmethod
    def _from_handle(cls, hp: SbrHparams, handle) -> "Model":
        m = cls.__new__(cls)
        m._L = _lib.load()
        m.hp = hp
        m.dim = int(hp.embedding_dim)
        m.storage_dim = storage_dim(m.dim)
        m._h = handle
        return m

    def is_partitioned(self) -> bool:
        v = C.c_int32()
        _check(self._L.sbr_model_is_partitioned(self._h, C.byref(v)))
        return bool(v.value)

    def partition_parts(self):
        """[(home rank, bytes)] of the partitioned table's parts — runs of pages with one home, in address order over the arrays
        E, E_acc, (E_m), b, b_acc, (b_m) (sbr_partition_part_info)."""
        n = C.c_uint32()
        _check(self._L.sbr_partition_num_parts(self._h, C.byref(n)))
        out = []
        for i in range(n.value):
            home, nbytes = C.c_uint32(), C.c_uint64()
            _check(self._L.sbr_partition_part_info(self._h, i, C.byref(home), C.byref(nbytes)))
            out.append((home.value, nbytes.value))
        return out

    def dense_count(self) -> int:
        d = self.storage_dim
        ng = {0: 4, 1: 3, 2: 0}[int(self.hp.model)]
        return (2 * d + 1) * ng * d if ng else d

    def param_count(self, which: int) -> int:
        n = C.c_uint64()
        _check(self._L.sbr_model_param_count(self._h, int(which), C.byref(n)))
        return n.value

    def get_param(self, which: int) -> np.ndarray:
        out = np.zeros(self.param_count(which), dtype=np.float32)
        if out.size:
            _check(self._L.sbr_model_get_param(self._h, int(which), _ptr(out), out.size))
        return out

    def get_param_rows(self, which: int, rows) -> np.ndarray:
        """Selected rows of an item-table block ([n, embedding_dim]; biases: [n]) without moving the whole table."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        table = self.param_count(which) != int(self.hp.num_items)
        out = np.zeros((rows.size, self.dim) if table else rows.size, dtype=np.float32)
        _check(self._L.sbr_model_get_param_rows(self._h, int(which), _ptr(rows), rows.size, _ptr(out)))
        return out

    def set_param(self, which: int, values):
        values = np.ascontiguousarray(values, dtype=np.float32).ravel()
        _check(self._L.sbr_model_set_param(self._h, int(which), _ptr(values), values.size))

    def set_item_tags(self, tags):
        """One 32-bit tag word per item, kept on the device for the ``any_of=`` / ``none_of=`` filters of the top-k calls
        (sbr_model_set_item_tags); ``None`` clears them.  Serving metadata: fit, set_param and load leave them alone, a session
        store stays usable, and ``save`` does not write them."""
        if tags is None:
            _check(self._L.sbr_model_set_item_tags(self._h, None))
            return
        t = np.ascontiguousarray(np.asarray(tags).ravel(), dtype=np.uint32)
        if t.size != int(self.hp.num_items):
            raise ValueError(f"one tag word per item ({int(self.hp.num_items)}); got {t.size}")
        _check(self._L.sbr_model_set_item_tags(self._h, _ptr(t)))

    def item_tags(self) -> np.ndarray:
        """The tag words last set, u32 [num_items] (sbr_model_get_item_tags); raises while the model has none."""
        out = np.zeros(int(self.hp.num_items), dtype=np.uint32)
        _check(self._L.sbr_model_get_item_tags(self._h, _ptr(out)))
        return out

    def set_item_groups(self, groups):
        """One u32 group word per item (a series, a seller, a category; ``NO_GROUP`` = never capped), kept on the device for the
        ``recommend_capped`` calls (sbr_model_set_item_groups); ``None`` clears them.  Serving metadata exactly as the item tags:
        fit, set_param and load leave them alone, a session store stays usable, and ``save`` does not write them."""
        if groups is None:
            _check(self._L.sbr_model_set_item_groups(self._h, None))
            self._groups = None
            return
        g = np.asarray(groups).ravel()
        if g.size != int(self.hp.num_items):
            raise ValueError(f"one group word per item ({int(self.hp.num_items)}); got {g.size}")
        if g.dtype.kind not in "iu" or (g.size and (int(g.min()) < 0 or int(g.max()) > 0xFFFFFFFF)):
            raise ValueError("groups: whole numbers from 0 to 2^32 - 1 (NO_GROUP)")
        g = np.ascontiguousarray(g, dtype=np.uint32)
        _check(self._L.sbr_model_set_item_groups(self._h, _ptr(g)))
        self._groups = g.copy()

    def item_groups(self) -> np.ndarray:
        """The group words last set, u32 [num_items] (sbr_model_get_item_groups); raises while the model has none."""
        out = np.zeros(int(self.hp.num_items), dtype=np.uint32)
        _check(self._L.sbr_model_get_item_groups(self._h, _ptr(out)))
        return out

    def _capped_finish(self, top, items, scores, flags, cap, k, pool, exact):
        """the shared tail of the *_capped methods: flags u8 -> complete bool, the incomplete rows finished when exact"""
        complete = flags.astype(bool)
        if exact and not complete.all():
            groups = getattr(self, "_groups", None)
            capped_complete(top, items, scores, complete, self.item_groups() if groups is None else groups, cap, k, pool,
                            int(self.hp.num_items))
        return items, scores, complete

    def recommend_capped(self, user_ptr, item_ids, k: int, cap: int = 1, pool=None, include_history: bool = False, any_of=None,
                         none_of=None, exact: bool = True):
        """Exact top-k with at most ``cap`` items of one item group (``set_item_groups``) per row — "one per series", "two per
        seller" (sbr_recommend_capped): (items [U, k] u32, scores [U, k] f32, complete [U] bool).  A row is ``recommend``'s order
        walked from the top, an entry kept while fewer than cap kept entries share its group (NO_GROUP: always), k kept entries
        in all; eligibility (history, any_of / none_of) is ``recommend``'s, the scores are predict's bits.  The device applies the
        rule to each row's best ``pool`` (default min(1 024, max(64, 4 k))); a row that neither kept k nor saw everything eligible
        comes back short with complete False — a prefix of the exact answer.  ``exact=True`` finishes such rows with
        ``recommend_top`` at a growing n and the rule on the host, so every row is the exact answer and complete is all True;
        ``exact=False`` returns the library's rows and flags as they are."""
        ca, pool = _cap_args(k, cap, pool)
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        nu = max(len(up) - 1, 0)
        masks = _tag_masks(any_of, none_of, nu)
        items, scores = np.zeros((nu, int(k)), dtype=np.uint32), np.zeros((nu, int(k)), dtype=np.float32)
        flags_out = np.zeros(max(nu, 1), dtype=np.uint8)
        flags = RECOMMEND_INCLUDE_HISTORY if include_history else 0
        _check(self._L.sbr_recommend_capped(self._h, _ptr(up), _ptr(it), nu, int(k), flags, C.byref(ca),
                                            None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]),
                                            _ptr(items), _ptr(scores), _ptr(flags_out)))

        def top(rows, n):
            sp = np.zeros(rows.size + 1, dtype=np.uint64)
            lens = (up[rows + 1] - up[rows]).astype(np.int64)
            sp[1:] = np.cumsum(lens)
            si = np.concatenate([it[int(up[r]) : int(up[r + 1])] for r in rows]) if rows.size else np.zeros(0, np.uint32)
            return self.recommend_top(sp, si, n, include_history=include_history, any_of=None if masks is None else masks[0][rows],
                                      none_of=None if masks is None else masks[1][rows])

        return self._capped_finish(top, items, scores, flags_out[:nu], int(cap), int(k), pool, exact)

    def recommend_capped_reps(self, reps, k: int, cap: int = 1, pool=None, exclude=None, any_of=None, none_of=None, exact: bool = True):
        """As recommend_capped, from representations [U, embedding_dim]; exclude: None or one sequence of item ids per user."""
        ca, pool = _cap_args(k, cap, pool)
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        nu = reps.shape[0]
        masks = _tag_masks(any_of, none_of, nu)
        items, scores = np.zeros((nu, int(k)), dtype=np.uint32), np.zeros((nu, int(k)), dtype=np.float32)
        flags_out = np.zeros(max(nu, 1), dtype=np.uint8)
        ep, ei = _exclusion_csr(exclude, nu)
        _check(self._L.sbr_recommend_capped_reps(self._h, _ptr(reps), nu, int(k), None if ep is None else _ptr(ep),
                                                 None if ei is None else _ptr(ei), C.byref(ca),
                                                 None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]),
                                                 _ptr(items), _ptr(scores), _ptr(flags_out)))

        def top(rows, n):
            return self.recommend_top_reps(reps[rows], n, exclude=None if exclude is None else [exclude[int(r)] for r in rows],
                                           any_of=None if masks is None else masks[0][rows],
                                           none_of=None if masks is None else masks[1][rows])

        return self._capped_finish(top, items, scores, flags_out[:nu], int(cap), int(k), pool, exact)

    def global_epoch(self) -> int:
        n = C.c_uint64()
        _check(self._L.sbr_model_get_epoch(self._h, C.byref(n)))
        return n.value

    def counters(self):
        e, t = C.c_uint64(), C.c_uint64()
        _check(self._L.sbr_model_get_counters(self._h, C.byref(e), C.byref(t)))
        return e.value, t.value

    def set_counters(self, global_epoch: int, optimizer_steps: int):
        _check(self._L.sbr_model_set_counters(self._h, global_epoch, optimizer_steps))

    def get_rng(self) -> bytes:
        """The model RNG's state as the 16 bytes that re-create it through ``XorShiftRng.from_seed``."""
        buf = (C.c_uint8 * 16)()
        _check(self._L.sbr_model_get_rng(self._h, buf))
        return bytes(buf)

    def set_rng(self, state: bytes):
        state = bytes(state)
        if len(state) != 16:
            raise ValueError("RNG state is 16 bytes")
        _check(self._L.sbr_model_set_rng(self._h, (C.c_uint8 * 16)(*state)))

    def table_slice(self, which: int):
        """(device pointer of an item-table block of this replica, bytes per owner slice): rank r's slice is [ptr + r * bytes, + bytes)
        (sbr_model_table_slice; the block is allocated for num_devices equal slices).  (0, 0): the model has no such block."""
        base, nb = C.c_void_p(), C.c_uint64()
        _check(self._L.sbr_model_table_slice(self._h, int(which), C.byref(base), C.byref(nb)))
        return (base.value or 0), nb.value

    def optimizer_state_gathered(self):
        """The host has all-gathered the owners' optimiser-state slices into this replica (sbr_model_optimizer_state_gathered)."""
        _check(self._L.sbr_model_optimizer_state_gathered(self._h))

    def optimizer_state_is_partial(self) -> bool:
        v = C.c_int32()
        _check(self._L.sbr_model_optimizer_state_is_partial(self._h, C.byref(v)))
        return bool(v.value)

    def set_stream(self, hip_stream_ptr: int):
        _check(self._L.sbr_model_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def synchronize(self):
        _check(self._L.sbr_model_synchronize(self._h))

    def timing_enable(self, on: bool = True):
        _check(self._L.sbr_model_timing_enable(self._h, 1 if on else 0))

    def timing_select(self, families=None):
        """Which kernel families are bracketed by events while timing is on (names of ``KernelFamily``; None = all)."""
        mask = 0xFFFFFFFF if families is None else sum(1 << int(KernelFamily[f]) for f in families)
        _check(self._L.sbr_model_timing_select(self._h, mask))

    def set_reference_order(self, on: bool = True):
        """Negatives from the worker's own sequential xorshift stream (sequence_model.rs:58-65, :137) instead of the counter-keyed
        draws: one subsequence per step; one device, or a Synchronous replicated group driven by `group_fit` (every worker's gradient then
        goes in as its own optimiser step); max_sequence_length <= 256 / 221 / 81 at d <= 64 / 128 / 256 (sbr_model_set_reference_order)."""
        _check(self._L.sbr_model_set_reference_order(self._h, 1 if on else 0))

    def set_step_fusion(self, level: int):
        """How one-sequence steps at d <= 32 are launched: 0 separate launches, 1 fused launches (four per step), 2 (default)
        runs of steps in one launch where the shape allows (sbr_model_set_step_fusion).  Same bits."""
        _check(self._L.sbr_model_set_step_fusion(self._h, int(level)))

    def set_overlap(self, on: bool = True):
        """False: side-stream work runs on the main stream, so kernel families are timed standalone."""
        _check(self._L.sbr_model_set_overlap(self._h, 1 if on else 0))

    def test_delays_queued(self):
        """Delay kernels the stream-delay test hook (SBR_TEST_STREAM_DELAY) has queued on this model's streams since the last
        read, per role (sbr_test_delays_queued)."""
        n = (C.c_uint64 * len(STREAM_ROLES))()
        _check(self._L.sbr_test_delays_queued(self._h, n))
        return {role: int(n[i]) for i, role in enumerate(STREAM_ROLES)}

    def timing_read(self):
        ms = (C.c_double * NUM_KERNEL_FAMILIES)()
        n = (C.c_uint64 * NUM_KERNEL_FAMILIES)()
        _check(self._L.sbr_model_timing_read(self._h, ms, n))
        return {KernelFamily(i).name: (ms[i], n[i]) for i in range(NUM_KERNEL_FAMILIES)}

    def fit(self, user_ptr, item_ids) -> float:
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        loss = C.c_float()
        _check(self._L.sbr_model_fit(self._h, _ptr(up), _ptr(it), len(up) - 1, C.byref(loss)))
        return loss.value

    def last_fit_lagged_loss(self) -> float:
        """What the reference's ``fit`` would have returned for the last ``fit`` / ``group_fit``; ``fit`` itself
        returns the true mean loss."""
        v = C.c_float()
        _check(self._L.sbr_model_last_fit_lagged_loss(self._h, C.byref(v)))
        return v.value

    def fit_begin(self, user_ptr, item_ids) -> FitPlan:
        return FitPlan(self, user_ptr, item_ids)

    def user_representation(self, item_ids) -> np.ndarray:
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        out = np.zeros(self.dim, dtype=np.float32)
        _check(self._L.sbr_user_representation(self._h, _ptr(it), it.size, _ptr(out)))
        return out

    def predict(self, user, item_ids) -> np.ndarray:
        user = np.ascontiguousarray(user, dtype=np.float32)
        if user.size != self.dim:
            raise ValueError("user representation has the wrong dimension")
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        out = np.zeros(it.size, dtype=np.float32)
        _check(self._L.sbr_predict(self._h, _ptr(user), _ptr(it), it.size, _ptr(out)))
        return out

    def mrr_score(self, user_ptr, item_ids):
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        ranks = np.zeros(max(len(up) - 1, 1), dtype=np.uint32)
        mrr, n = C.c_float(), C.c_uint64()
        _check(self._L.sbr_mrr_score(self._h, _ptr(up), _ptr(it), len(up) - 1, C.byref(mrr), _ptr(ranks), C.byref(n)))
        return mrr.value, ranks[: n.value].copy()

    def recommend(self, user_ptr, item_ids, k: int, include_history: bool = False, any_of=None, none_of=None):
        """Exact top-k of the whole catalogue for each history (CSR, the layout of mrr_score): items [U, k] u32 and scores
        [U, k] f32, score descending, ties to the lower id; short rows padded with (RECOMMEND_NO_ITEM, -inf).
        any_of / none_of: the per-user tag filter (sbr_recommend_filtered; the model needs ``set_item_tags``) — a u32 mask per
        user, or a scalar for all: item i is eligible for user u iff tags[i] & none_of[u] == 0 and (any_of[u] == 0 or
        tags[i] & any_of[u] != 0)."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        nu = max(len(up) - 1, 0)
        masks = _tag_masks(any_of, none_of, nu)
        items = np.zeros((nu, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((nu, max(int(k), 0)), dtype=np.float32)
        flags = RECOMMEND_INCLUDE_HISTORY if include_history else 0
        if masks is None:
            _check(self._L.sbr_recommend(self._h, _ptr(up), _ptr(it), nu, int(k) & 0xFFFFFFFF, flags, _ptr(items), _ptr(scores)))
        else:
            _check(self._L.sbr_recommend_filtered(self._h, _ptr(up), _ptr(it), nu, int(k) & 0xFFFFFFFF, flags, _ptr(masks[0]),
                                                  _ptr(masks[1]), _ptr(items), _ptr(scores)))
        return items, scores

    def recommend_reps(self, reps, k: int, exclude=None, any_of=None, none_of=None):
        """As recommend, from representations [U, embedding_dim] (user_representation's); exclude: None or one sequence of
        item ids per user; any_of / none_of: recommend's tag filter."""
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        nu = reps.shape[0]
        masks = _tag_masks(any_of, none_of, nu)
        items = np.zeros((nu, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((nu, max(int(k), 0)), dtype=np.float32)
        ep, ei = _exclusion_csr(exclude, nu)
        if masks is None:
            _check(self._L.sbr_recommend_reps(self._h, _ptr(reps), nu, int(k) & 0xFFFFFFFF, None if ep is None else _ptr(ep),
                                              None if ei is None else _ptr(ei), _ptr(items), _ptr(scores)))
        else:
            _check(self._L.sbr_recommend_filtered_reps(self._h, _ptr(reps), nu, int(k) & 0xFFFFFFFF, None if ep is None else _ptr(ep),
                                                       None if ei is None else _ptr(ei), _ptr(masks[0]), _ptr(masks[1]), _ptr(items),
                                                       _ptr(scores)))
        return items, scores

    def recommend_sampled(self, user_ptr, item_ids, k: int, temperature: float = 1.0, seed: int = 0, streams=None,
                          include_history: bool = False, any_of=None, none_of=None, log_prob: bool = False):
        """k draws without replacement from softmax(score / temperature) over the items each user may see (sbr_recommend_sampled):
        items [U, k] u32, scores [U, k] f32 — the plain scores of the drawn items, predict's bits, in draw order — and keys [U, k]
        f32, descending; short rows padded with (RECOMMEND_NO_ITEM, -inf, -inf).  Eligibility is ``recommend``'s (history, any_of /
        none_of).  The noise of (row, item) is a function of (seed, streams[row], item) alone — streams: one u64 per row, default the
        row's index — so the same (seed, stream) returns the same row bit for bit; vary ``seed`` per request.  ``log_prob=True``
        appends a fourth output, log_prob [U, k] f64: the draws' propensities, ``log_partition`` of the same arguments applied to
        the scores by ``Partition.slate_log_prob``."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        nu = max(len(up) - 1, 0)
        masks = _tag_masks(any_of, none_of, nu)
        sa, _keep = _sample_args(temperature, seed, streams, nu)
        items, scores, keys = (np.zeros((nu, max(int(k), 0)), dtype=dt) for dt in (np.uint32, np.float32, np.float32))
        flags = RECOMMEND_INCLUDE_HISTORY if include_history else 0
        _check(self._L.sbr_recommend_sampled(self._h, _ptr(up), _ptr(it), nu, int(k) & 0xFFFFFFFF, flags, C.byref(sa),
                                             None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]),
                                             _ptr(items), _ptr(scores), _ptr(keys)))
        if log_prob:
            part = self.log_partition(up, it, temperature, include_history=include_history, any_of=any_of, none_of=none_of)
            return items, scores, keys, part.slate_log_prob(scores)
        return items, scores, keys

    def recommend_sampled_reps(self, reps, k: int, temperature: float = 1.0, seed: int = 0, streams=None, exclude=None, any_of=None,
                               none_of=None, log_prob: bool = False):
        """As recommend_sampled, from representations [U, embedding_dim]; exclude: None or one sequence of item ids per user."""
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        nu = reps.shape[0]
        masks = _tag_masks(any_of, none_of, nu)
        sa, _keep = _sample_args(temperature, seed, streams, nu)
        items, scores, keys = (np.zeros((nu, max(int(k), 0)), dtype=dt) for dt in (np.uint32, np.float32, np.float32))
        ep, ei = _exclusion_csr(exclude, nu)
        _check(self._L.sbr_recommend_sampled_reps(self._h, _ptr(reps), nu, int(k) & 0xFFFFFFFF, None if ep is None else _ptr(ep),
                                                  None if ei is None else _ptr(ei), C.byref(sa),
                                                  None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]),
                                                  _ptr(items), _ptr(scores), _ptr(keys)))
        if log_prob:
            part = self.log_partition_reps(reps, temperature, exclude=exclude, any_of=any_of, none_of=none_of)
            return items, scores, keys, part.slate_log_prob(scores)
        return items, scores, keys

    def log_partition(self, user_ptr, item_ids, temperature: float = 1.0, include_history: bool = False, any_of=None,
                      none_of=None) -> Partition:
        """The exact fixed-point mass of softmax(score / temperature) over the items each user may see (sbr_log_partition):
        eligibility is ``recommend``'s; the result does not depend on the batch or on how the scan is cut up."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        nu = max(len(up) - 1, 0)
        masks = _tag_masks(any_of, none_of, nu)
        shift, mass, fb = _partition_outputs(nu)
        flags = RECOMMEND_INCLUDE_HISTORY if include_history else 0
        _check(self._L.sbr_log_partition(self._h, _ptr(up), _ptr(it), nu, flags, float(np.float32(temperature)),
                                         None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]),
                                         _ptr(shift), _ptr(mass), C.byref(fb)))
        return Partition(temperature, shift, mass, fb.value)

    def log_partition_reps(self, reps, temperature: float = 1.0, exclude=None, any_of=None, none_of=None) -> Partition:
        """As log_partition, from representations [U, embedding_dim]; exclude: None or one sequence of item ids per user."""
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        nu = reps.shape[0]
        masks = _tag_masks(any_of, none_of, nu)
        shift, mass, fb = _partition_outputs(nu)
        ep, ei = _exclusion_csr(exclude, nu)
        _check(self._L.sbr_log_partition_reps(self._h, _ptr(reps), nu, None if ep is None else _ptr(ep), None if ei is None else _ptr(ei),
                                              float(np.float32(temperature)), None if masks is None else _ptr(masks[0]),
                                              None if masks is None else _ptr(masks[1]), _ptr(shift), _ptr(mass), C.byref(fb)))
        return Partition(temperature, shift, mass, fb.value)

    def _recommend_above(self, user_ptr, item_ids, threshold, include_history, any_of, none_of, max_results, order, count_only, n=None):
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        nu = max(len(up) - 1, 0)
        masks = _tag_masks(any_of, none_of, nu)
        flags = RECOMMEND_INCLUDE_HISTORY if include_history else 0
        return _above(lambda *out: (self._L.sbr_recommend_above if n is None else self._L.sbr_recommend_top)(
                          self._h, _ptr(up), _ptr(it), nu, out[0], flags, None if masks is None else _ptr(masks[0]),
                          None if masks is None else _ptr(masks[1]), *out[1:]),
                      nu, threshold, max_results, order, count_only, n)

    def recommend_above(self, user_ptr, item_ids, threshold, include_history: bool = False, any_of=None, none_of=None,
                        max_results=None, order: str = "score") -> Above:
        """Every item a user may see whose score is >= ``threshold`` (sbr_recommend_above) — a set, so no k and no cap of 1 024:
        an ``Above`` over the histories' rows, item ids with predict's score bits.  Eligibility is ``recommend``'s (history,
        any_of / none_of).  threshold: a scalar or one f32 per row; the compare is the f32 ``>=`` (ties at the bar all pass,
        -0.0 == +0.0, -inf returns every eligible item, +inf none, a NaN is a ValueError).  order: "score" (descending, ties to
        the lower id: with the threshold at ``recommend(k)``'s k-th score the row starts with that call's row, bit for bit) or
        "id" (ascending, as the library writes it).  max_results (default ABOVE_MAX_RESULTS = 2^24 pairs) sizes the one call's
        buffer; a larger total raises a ValueError that states it — ``count_above`` costs one scan and says how many to expect.
        With ``log_partition``: ``threshold = temperature * (np.log(p) + part.log_z)`` returns every item the user would be drawn
        with probability at least p."""
        return self._recommend_above(user_ptr, item_ids, threshold, include_history, any_of, none_of, max_results, order, False)

    def count_above(self, user_ptr, item_ids, threshold, include_history: bool = False, any_of=None, none_of=None) -> np.ndarray:
        """``recommend_above(...).counts`` (u64 [U]) without writing any pair: one scan.  With no masks and include_history it is
        ``rank_targets``' rank of an item that scores exactly the threshold."""
        return self._recommend_above(user_ptr, item_ids, threshold, include_history, any_of, none_of, None, "id", True)

    def _recommend_above_reps(self, reps, threshold, exclude, any_of, none_of, max_results, order, count_only, n=None):
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        nu = reps.shape[0]
        masks = _tag_masks(any_of, none_of, nu)
        ep, ei = _exclusion_csr(exclude, nu)
        return _above(lambda *out: (self._L.sbr_recommend_above_reps if n is None else self._L.sbr_recommend_top_reps)(
                          self._h, _ptr(reps), nu, out[0], None if ep is None else _ptr(ep), None if ei is None else _ptr(ei),
                          None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]), *out[1:]),
                      nu, threshold, max_results, order, count_only, n)

    def recommend_above_reps(self, reps, threshold, exclude=None, any_of=None, none_of=None, max_results=None,
                             order: str = "score") -> Above:
        """As recommend_above, from representations [U, embedding_dim]; exclude: None or one sequence of item ids per user."""
        return self._recommend_above_reps(reps, threshold, exclude, any_of, none_of, max_results, order, False)

    def count_above_reps(self, reps, threshold, exclude=None, any_of=None, none_of=None) -> np.ndarray:
        """``recommend_above_reps(...).counts`` without writing any pair: one scan."""
        return self._recommend_above_reps(reps, threshold, exclude, any_of, none_of, None, "id", True)

    def _audience_above_reps(self, reps, items, threshold, exclude, max_results, order, count_only, n=None):
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        q = np.ascontiguousarray(items, dtype=np.uint32).ravel()
        ep, ei = _exclusion_csr(exclude, q.size)
        return _above(lambda *out: (self._L.sbr_audience_above_reps if n is None else self._L.sbr_audience_top_reps)(
                          self._h, _ptr(reps), reps.shape[0], _ptr(q), q.size, out[0], None if ep is None else _ptr(ep),
                          None if ei is None else _ptr(ei), *out[1:]),
                      q.size, threshold, max_results, order, count_only, n)

    def audience_above_reps(self, reps, items, threshold, exclude=None, max_results=None, order: str = "score") -> Above:
        """The reverse scan's threshold form (sbr_audience_above_reps): for each query item ``items[j]`` every row of ``reps``
        [S, embedding_dim] that scores it >= ``threshold`` (a scalar or one per query) — an ``Above`` over the queries, row
        indices with the bits of ``predict(reps[s], [item])``.  exclude: None or one sequence of row indices per query.  The
        pairs are exactly the transposed pairs of ``recommend_above_reps(reps, t)`` restricted to the query items."""
        return self._audience_above_reps(reps, items, threshold, exclude, max_results, order, False)

    def count_audience_above_reps(self, reps, items, threshold, exclude=None) -> np.ndarray:
        """``audience_above_reps(...).counts`` without writing any pair: one scan."""
        return self._audience_above_reps(reps, items, threshold, exclude, None, "id", True)

    def _audience_above(self, user_ptr, item_ids, items, threshold, include_history, max_results, order, count_only, n=None):
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        q = np.ascontiguousarray(items, dtype=np.uint32).ravel()
        nu = max(len(up) - 1, 0)
        flags = RECOMMEND_INCLUDE_HISTORY if include_history else 0
        return _above(lambda *out: (self._L.sbr_audience_above if n is None else self._L.sbr_audience_top)(
                          self._h, _ptr(up), _ptr(it), nu, _ptr(q), q.size, out[0], flags, *out[1:]),
                      q.size, threshold, max_results, order, count_only, n)

    def audience_above(self, user_ptr, item_ids, items, threshold, include_history: bool = False, max_results=None,
                       order: str = "score") -> Above:
        """``audience_above_reps`` on ``user_representations`` of the histories (sbr_audience_above): user indices.  Unless
        include_history a user whose history holds the query item is left out of that item's row."""
        return self._audience_above(user_ptr, item_ids, items, threshold, include_history, max_results, order, False)

    def count_audience_above(self, user_ptr, item_ids, items, threshold, include_history: bool = False) -> np.ndarray:
        """``audience_above(...).counts`` without writing any pair."""
        return self._audience_above(user_ptr, item_ids, items, threshold, include_history, None, "id", True)

    def recommend_top(self, user_ptr, item_ids, n, include_history: bool = False, any_of=None, none_of=None, max_results=None,
                      order: str = "score") -> Above:
        """Each user's exact best ``n`` items (sbr_recommend_top) — a budget, with no cap of 1 024: an ``Above`` over the histories'
        rows with ``cuts`` set.  n: a scalar or one whole number >= 0 per row; 0 gives an empty row, an n past the eligible items
        all of them.  Eligibility is ``recommend``'s, the order every call's (score descending, ties to the lower id, -0.0 == +0.0):
        for n <= 1 024 a row is ``recommend(k=n)``'s without padding, for any n the first n of
        ``recommend_above(threshold=cuts[row])``'s; a tie group that straddles the cut gives up exactly its lowest ids.
        ``cuts[row]``: the score of the row's last item (a zero as +0.0), -inf where the row holds everything eligible, +inf for
        n = 0.  The cuts cost 8 catalogue scans on the device (a radix select on the score bits, no host round trip), the pairs
        ``recommend_above``'s count and fill at the cuts and a trim.  max_results and order as in ``recommend_above``; max_results
        is held against the pairs returned, sum(min(n, eligible))."""
        return self._recommend_above(user_ptr, item_ids, None, include_history, any_of, none_of, max_results, order, False, n)

    def nth_score(self, user_ptr, item_ids, n, include_history: bool = False, any_of=None, none_of=None):
        """``(r.cuts, r.counts)`` of ``r = recommend_top(...)`` (f32 [U], u64 [U]) from the select alone: no pair is written."""
        return self._recommend_above(user_ptr, item_ids, None, include_history, any_of, none_of, None, "id", True, n)

    def recommend_top_reps(self, reps, n, exclude=None, any_of=None, none_of=None, max_results=None, order: str = "score") -> Above:
        """As recommend_top, from representations [U, embedding_dim]; exclude: None or one sequence of item ids per user."""
        return self._recommend_above_reps(reps, None, exclude, any_of, none_of, max_results, order, False, n)

    def nth_score_reps(self, reps, n, exclude=None, any_of=None, none_of=None):
        """``(cuts, counts)`` of ``recommend_top_reps(...)`` from the select alone."""
        return self._recommend_above_reps(reps, None, exclude, any_of, none_of, None, "id", True, n)

    def audience_top_reps(self, reps, items, n, exclude=None, max_results=None, order: str = "score") -> Above:
        """The reverse scan's budget form (sbr_audience_top_reps): for each query item ``items[j]`` the exact best ``n`` (a scalar or
        one per query; any size) rows of ``reps`` [S, embedding_dim] — "we can reach 50 000 people: which 50 000?".  An ``Above``
        over the queries with ``cuts``, row indices with the bits of ``predict(reps[s], [item])``; exclude as in ``audience_reps``.
        For n <= 1 024 a row is ``audience_reps(k=n)``'s without padding."""
        return self._audience_above_reps(reps, items, None, exclude, max_results, order, False, n)

    def nth_audience_score_reps(self, reps, items, n, exclude=None):
        """``(cuts, counts)`` of ``audience_top_reps(...)`` from the select alone."""
        return self._audience_above_reps(reps, items, None, exclude, None, "id", True, n)

    def audience_top(self, user_ptr, item_ids, items, n, include_history: bool = False, max_results=None, order: str = "score") -> Above:
        """``audience_top_reps`` on ``user_representations`` of the histories (sbr_audience_top): user indices.  Unless
        include_history a user whose history holds the query item is left out of that item's row."""
        return self._audience_above(user_ptr, item_ids, items, None, include_history, max_results, order, False, n)

    def nth_audience_score(self, user_ptr, item_ids, items, n, include_history: bool = False):
        """``(cuts, counts)`` of ``audience_top(...)`` from the select alone."""
        return self._audience_above(user_ptr, item_ids, items, None, include_history, None, "id", True, n)

    def diverse_max_pool(self) -> int:
        """The largest ``pool`` of recommend_diverse on this model (sbr_recommend_diverse_max_pool): a user's pool lives in one
        workgroup's LDS, min(1024, 32768 / storage width) rows."""
        n = C.c_uint32()
        _check(self._L.sbr_recommend_diverse_max_pool(self._h, C.byref(n)))
        return n.value

    def recommend_diverse(self, user_ptr, item_ids, k: int, pool: int, trade_off: float = 0.5, metric="cosine",
                          include_history: bool = False, any_of=None, none_of=None):
        """Diversified top-k (sbr_recommend_diverse): from the ``pool`` best items of each history — recommend's row at k = pool —
        k are picked greedily by maximal marginal relevance, trade_off * score - (1 - trade_off) * (the largest similarity to an
        item picked before), the first pick being the best item.  Items [U, k] u32 in pick order and their scores [U, k] f32
        (recommend's bits); short rows padded with (RECOMMEND_NO_ITEM, -inf).  metric: similar_items' "cosine" or "dot".
        trade_off = 1 is recommend(k); pool == k reorders it.  k <= pool <= diverse_max_pool().  any_of / none_of: recommend's
        tag filter; the pool is then the filtered row."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        nu = max(len(up) - 1, 0)
        masks = _tag_masks(any_of, none_of, nu)
        items = np.zeros((nu, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((nu, max(int(k), 0)), dtype=np.float32)
        flags = RECOMMEND_INCLUDE_HISTORY if include_history else 0
        if masks is None:
            _check(self._L.sbr_recommend_diverse(self._h, _ptr(up), _ptr(it), nu, int(k) & 0xFFFFFFFF, int(pool) & 0xFFFFFFFF,
                                                 float(trade_off), _similar_metric(metric), flags, _ptr(items), _ptr(scores)))
        else:
            _check(self._L.sbr_recommend_diverse_filtered(self._h, _ptr(up), _ptr(it), nu, int(k) & 0xFFFFFFFF, int(pool) & 0xFFFFFFFF,
                                                          float(trade_off), _similar_metric(metric), flags, _ptr(masks[0]),
                                                          _ptr(masks[1]), _ptr(items), _ptr(scores)))
        return items, scores

    def recommend_diverse_reps(self, reps, k: int, pool: int, trade_off: float = 0.5, metric="cosine", exclude=None, any_of=None,
                               none_of=None):
        """As recommend_diverse, from representations [U, embedding_dim]; exclude: None or one sequence of item ids per user."""
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        nu = reps.shape[0]
        masks = _tag_masks(any_of, none_of, nu)
        items = np.zeros((nu, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((nu, max(int(k), 0)), dtype=np.float32)
        ep, ei = _exclusion_csr(exclude, nu)
        if masks is None:
            _check(self._L.sbr_recommend_diverse_reps(self._h, _ptr(reps), nu, int(k) & 0xFFFFFFFF, int(pool) & 0xFFFFFFFF,
                                                      float(trade_off), _similar_metric(metric), None if ep is None else _ptr(ep),
                                                      None if ei is None else _ptr(ei), _ptr(items), _ptr(scores)))
        else:
            _check(self._L.sbr_recommend_diverse_filtered_reps(self._h, _ptr(reps), nu, int(k) & 0xFFFFFFFF, int(pool) & 0xFFFFFFFF,
                                                               float(trade_off), _similar_metric(metric),
                                                               None if ep is None else _ptr(ep), None if ei is None else _ptr(ei),
                                                               _ptr(masks[0]), _ptr(masks[1]), _ptr(items), _ptr(scores)))
        return items, scores

    def similar_items(self, query_items, k: int, metric="cosine", include_self: bool = False, exclude=None, any_of=None, none_of=None):
        """Exact top-k neighbours of each query item among the whole catalogue (sbr_similar_items): items [Q, k] u32 and scores
        [Q, k] f32, score descending, ties to the lower id; short rows padded with (RECOMMEND_NO_ITEM, -inf).  metric: "cosine"
        (of the item embeddings; a zero row has similarity 0 with everything) or "dot" (their plain dot product) — the item bias
        takes no part in either.  The query itself is left out of its row unless include_self; exclude: None or one sequence of
        item ids per query.  Queries may repeat.  any_of / none_of: recommend's tag filter with one mask pair per query
        (sbr_similar_items_filtered: "similar items of the same category")."""
        q = np.ascontiguousarray(query_items, dtype=np.uint32).ravel()
        metric = _similar_metric(metric)
        nq = q.size
        masks = _tag_masks(any_of, none_of, nq)
        items = np.zeros((nq, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((nq, max(int(k), 0)), dtype=np.float32)
        ep, ei = _exclusion_csr(exclude, nq)
        flags = SIMILAR_INCLUDE_SELF if include_self else 0
        if masks is None:
            _check(self._L.sbr_similar_items(self._h, _ptr(q), nq, int(k) & 0xFFFFFFFF, metric, flags, None if ep is None else _ptr(ep),
                                             None if ei is None else _ptr(ei), _ptr(items), _ptr(scores)))
        else:
            _check(self._L.sbr_similar_items_filtered(self._h, _ptr(q), nq, int(k) & 0xFFFFFFFF, metric, flags,
                                                      None if ep is None else _ptr(ep), None if ei is None else _ptr(ei),
                                                      _ptr(masks[0]), _ptr(masks[1]), _ptr(items), _ptr(scores)))
        return items, scores

    def user_representations(self, user_ptr, item_ids) -> np.ndarray:
        """user_representation of every history of a CSR in one call (sbr_user_representations): [U, embedding_dim] f32, row u
        with the bits of the single call on history u; an empty history gets item 0's state."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        nu = max(len(up) - 1, 0)
        out = np.zeros((nu, self.dim), dtype=np.float32)
        _check(self._L.sbr_user_representations(self._h, _ptr(up), _ptr(it), nu, _ptr(out)))
        return out

    @staticmethod
    def _per_user(flat: np.ndarray, ptr: np.ndarray):
        base = int(ptr[0])
        return [flat[int(ptr[u]) - base: int(ptr[u + 1]) - base] for u in range(len(ptr) - 1)]

    def score_candidates(self, user_ptr, item_ids, cand_ptr, cand_items):
        """predict for many users in one call (sbr_score_candidates): user u's history is item_ids[user_ptr[u]: user_ptr[u + 1]],
        its candidates cand_items[cand_ptr[u]: cand_ptr[u + 1]] (any order, duplicates allowed, none included).  One f32 array
        per user, in candidate order, with the bits of predict(user_representation(history), candidates); nothing is masked."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        cp = np.ascontiguousarray(cand_ptr, dtype=np.uint64)
        ci = np.ascontiguousarray(cand_items, dtype=np.uint32)
        if len(cp) != len(up):
            raise ValueError("one candidate range per user")
        nu = max(len(up) - 1, 0)
        scores = np.zeros(max(ci.size, 1), dtype=np.float32)
        _check(self._L.sbr_score_candidates(self._h, _ptr(up), _ptr(it), nu, _ptr(cp), _ptr(ci) if ci.size else None, _ptr(scores)))
        return self._per_user(scores, cp)

    def score_candidates_reps(self, reps, cand_ptr, cand_items):
        """As score_candidates, from representations [U, embedding_dim]."""
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        nu = reps.shape[0]
        cp = np.ascontiguousarray(cand_ptr, dtype=np.uint64)
        ci = np.ascontiguousarray(cand_items, dtype=np.uint32)
        if len(cp) != nu + 1:
            raise ValueError("one candidate range per user")
        scores = np.zeros(max(ci.size, 1), dtype=np.float32)
        _check(self._L.sbr_score_candidates_reps(self._h, _ptr(reps), nu, _ptr(cp), _ptr(ci) if ci.size else None, _ptr(scores)))
        return self._per_user(scores, cp)

    def audience_reps(self, reps, items, k: int, exclude=None):
        """The reverse scan (sbr_audience_reps): for each query item ``items[j]`` the k rows of ``reps`` [S, embedding_dim] that
        score it highest — rows [Q, k] u32 (indices into ``reps``) and scores [Q, k] f32 with the bits of ``predict(reps[s],
        [item])``, score descending, ties to the lower row, short rows padded with (RECOMMEND_NO_ITEM, -inf).  Queries may repeat
        and come in any order.  exclude: None or one sequence of row indices per query."""
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        q = np.ascontiguousarray(items, dtype=np.uint32).ravel()
        rows = np.zeros((q.size, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((q.size, max(int(k), 0)), dtype=np.float32)
        ep, ei = _exclusion_csr(exclude, q.size)
        _check(self._L.sbr_audience_reps(self._h, _ptr(reps), reps.shape[0], _ptr(q), q.size, int(k) & 0xFFFFFFFF,
                                         None if ep is None else _ptr(ep), None if ei is None else _ptr(ei), _ptr(rows), _ptr(scores)))
        return rows, scores

    def audience(self, user_ptr, item_ids, items, k: int, include_history: bool = False):
        """``audience_reps`` on ``user_representations`` of the histories (sbr_audience): users [Q, k] u32 and scores [Q, k] f32.
        Unless include_history a user whose history holds the query item is left out of that item's row."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        q = np.ascontiguousarray(items, dtype=np.uint32).ravel()
        nu = max(len(up) - 1, 0)
        users = np.zeros((q.size, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((q.size, max(int(k), 0)), dtype=np.float32)
        flags = RECOMMEND_INCLUDE_HISTORY if include_history else 0
        _check(self._L.sbr_audience(self._h, _ptr(up), _ptr(it), nu, _ptr(q), q.size, int(k) & 0xFFFFFFFF, flags, _ptr(users),
                                    _ptr(scores)))
        return users, scores

    def recommend_among(self, user_ptr, item_ids, k: int, among, include_history: bool = False):
        """recommend with every item outside `among` ineligible (sbr_recommend_among): the exact top-k of that item set — item
        ids in any order, duplicates allowed — as catalogue ids, ordered and padded as recommend's rows.  Only the set's rows are
        scanned."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        sub = np.ascontiguousarray(among, dtype=np.uint32).ravel()
        nu = max(len(up) - 1, 0)
        items = np.zeros((nu, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((nu, max(int(k), 0)), dtype=np.float32)
        flags = RECOMMEND_INCLUDE_HISTORY if include_history else 0
        _check(self._L.sbr_recommend_among(self._h, _ptr(up), _ptr(it), nu, int(k) & 0xFFFFFFFF, flags, _ptr(sub) if sub.size else None,
                                           sub.size, _ptr(items), _ptr(scores)))
        return items, scores

    def recommend_among_reps(self, reps, k: int, among, exclude=None):
        """As recommend_among, from representations [U, embedding_dim]; exclude: None or one sequence of item ids per user."""
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        sub = np.ascontiguousarray(among, dtype=np.uint32).ravel()
        nu = reps.shape[0]
        items = np.zeros((nu, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((nu, max(int(k), 0)), dtype=np.float32)
        ep, ei = _exclusion_csr(exclude, nu)
        _check(self._L.sbr_recommend_among_reps(self._h, _ptr(reps), nu, int(k) & 0xFFFFFFFF, None if ep is None else _ptr(ep),
                                                None if ei is None else _ptr(ei), _ptr(sub) if sub.size else None, sub.size,
                                                _ptr(items), _ptr(scores)))
        return items, scores

    def rank_targets(self, user_ptr, item_ids, target_ptr, target_items, include_history: bool = False, any_of=None,
                     none_of=None) -> np.ndarray:
        """Exact ranks of every user's targets among the whole catalogue from one scan (sbr_rank_targets): user u's history is
        item_ids[user_ptr[u]: user_ptr[u + 1]], its targets target_items[target_ptr[u]: target_ptr[u + 1]]; rank =
        #{items whose masked score >= the target's}, the whole history masked to f32::MIN unless include_history.  One u32 per
        target, in target order.  With ``any_of`` / ``none_of`` (``recommend``'s masks; needs ``set_item_tags``) every item the
        masks forbid is masked as well (sbr_rank_targets_rows): a forbidden target has rank num_items."""
        if any_of is not None or none_of is not None:
            return _rank_targets_rows(self._L.sbr_rank_targets_rows, self._h, _check,
                                      _ModelRows(self)._hist(user_ptr, item_ids, include_history, any_of, none_of), target_ptr, target_items)
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        tp = np.ascontiguousarray(target_ptr, dtype=np.uint64)
        ti = np.ascontiguousarray(target_items, dtype=np.uint32)
        if len(tp) != len(up):
            raise ValueError("one target range per user")
        nu = max(len(up) - 1, 0)
        ranks = np.zeros(max(ti.size, 1), dtype=np.uint32)
        flags = RANK_INCLUDE_HISTORY if include_history else 0
        _check(self._L.sbr_rank_targets(self._h, _ptr(up), _ptr(it), nu, _ptr(tp), _ptr(ti), flags, _ptr(ranks)))
        return ranks[: ti.size]

    def rank_targets_reps(self, reps, target_ptr, target_items, exclude=None, any_of=None, none_of=None) -> np.ndarray:
        """As rank_targets, from representations [U, embedding_dim]; exclude: None or one sequence of masked item ids per
        user."""
        if any_of is not None or none_of is not None:
            return _rank_targets_rows(self._L.sbr_rank_targets_rows, self._h, _check, _ModelRows(self)._reps(reps, exclude, any_of, none_of),
                                      target_ptr, target_items)
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.dim)
        nu = reps.shape[0]
        tp = np.ascontiguousarray(target_ptr, dtype=np.uint64)
        ti = np.ascontiguousarray(target_items, dtype=np.uint32)
        if len(tp) != nu + 1:
            raise ValueError("one target range per user")
        ep, ei = _exclusion_csr(exclude, nu)
        ranks = np.zeros(max(ti.size, 1), dtype=np.uint32)
        _check(self._L.sbr_rank_targets_reps(self._h, _ptr(reps), nu, None if ep is None else _ptr(ep),
                                             None if ei is None else _ptr(ei), _ptr(tp), _ptr(ti), _ptr(ranks)))
        return ranks[: ti.size]

    def sequence_ranks(self, user_ptr, item_ids, include_history: bool = False, last=None):
        """Exact next-item rank at every position of every sequence from one forward pass per sequence (sbr_sequence_ranks):
        with W = min(n, max_sequence_length + 1) and w the last W items of user u, position p = 1 .. W - 1 ranks w[p] against
        the state after w[:p], the distinct items of w[:p] masked to f32::MIN unless include_history — the number
        rank_targets(history=w[:p], targets=[w[p]]) gives.  ``last`` (None = all) keeps only the last ``last`` positions of
        each window.  -> (ptr u64 [U + 1], ranks u32 [ptr[U]]); row u holds its positions ascending, empty for n < 2."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        if up.ndim != 1 or up.size < 1:
            raise ValueError("user_ptr holds num_users + 1 offsets")
        if last is None:
            last = 0
        elif not 1 <= int(last) <= 0xFFFFFFFF:
            raise ValueError("last must be None or in [1, 2**32)")
        nu = up.size - 1
        flags = RANK_INCLUDE_HISTORY if include_history else 0
        ptr = np.zeros(nu + 1, dtype=np.uint64)
        _check(self._L.sbr_sequence_ranks(self._h, _ptr(up), _ptr(it), nu, flags, int(last), _ptr(ptr), None))  # sizing: no device work
        ranks = np.zeros(max(int(ptr[nu]), 1), dtype=np.uint32)
        _check(self._L.sbr_sequence_ranks(self._h, _ptr(up), _ptr(it), nu, flags, int(last), _ptr(ptr), _ptr(ranks)))
        return ptr, ranks[: int(ptr[nu])]

    def sequence_partition(self, user_ptr, item_ids, temperature: float = 1.0, include_history: bool = False, last=None):
        """What softmax(score / temperature) needs to price the next item at every position of every sequence, from one forward
        pass per sequence (sbr_sequence_partition).  Windows, positions, ``last`` and the rows are ``sequence_ranks``'; per kept
        position p the shift and mass are those of ``log_partition([w[:p]], temperature, include_history)`` bit for bit, the
        score is the plain score of w[p] and ``masked`` is 1 where the prefix is masked and w[p] occurs in it (the policy never
        shows it).  -> (ptr u64 [U + 1], Partition over the ptr[U] flat positions, scores f32, masked u8);
        ``part.log_prob(scores[:, None])[:, 0]`` is the log-probability of each target that is not masked."""
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        if up.ndim != 1 or up.size < 1:
            raise ValueError("user_ptr holds num_users + 1 offsets")
        if last is None:
            last = 0
        elif not 1 <= int(last) <= 0xFFFFFFFF:
            raise ValueError("last must be None or in [1, 2**32)")
        t = float(np.float32(temperature))
        if not (np.isfinite(t) and t > 0.0):
            raise ValueError("temperature must be finite and > 0")
        nu = up.size - 1
        flags = RANK_INCLUDE_HISTORY if include_history else 0
        ptr = np.zeros(nu + 1, dtype=np.uint64)
        _check(self._L.sbr_sequence_partition(self._h, _ptr(up), _ptr(it), nu, t, flags, int(last), _ptr(ptr), None, None, None, None))  # sizing
        n = int(ptr[nu])
        shift, mass, _fb = _partition_outputs(n)
        scores = np.zeros(max(n, 1), dtype=np.float32)
        masked = np.zeros(max(n, 1), dtype=np.uint8)
        _check(self._L.sbr_sequence_partition(self._h, _ptr(up), _ptr(it), nu, t, flags, int(last), _ptr(ptr), _ptr(shift), _ptr(mass),
                                              _ptr(scores), _ptr(masked)))
        return ptr, Partition(temperature, shift, mass, softmax_frac_bits(self.hp.num_items)), scores[:n], masked[:n]

    def sessions(self, capacity: int, remember: int = 0) -> "Sessions":
        """A session store of ``capacity`` slots on this model (sbr_sessions_create): device-resident user states advanced one
        appended item at a time and read in place by recommend / score_candidates.  ``remember`` > 0 (at most 1 024;
        sbr_sessions_create_seen): each slot also remembers the last ``remember`` items appended to it, and the store's
        recommend / recommend_diverse exclude them."""
        return Sessions(self, capacity, remember)

    def rollout(self, histories, steps: int, mode: str = "greedy", temperature: float = 1.0, seed: int = 0, streams=None,
                exclude_history: bool = True, any_of=None, none_of=None, allow_repeats: bool = False, log_prob: bool = False,
                final_state: bool = False) -> Rollout:
        """``Sessions.rollout`` from histories (a list of item-id sequences), DEFINED as this sequence of calls: a temporary store
        of one slot per history, ``append`` of each history's last max_sequence_length items, and ``store.rollout`` of all slots
        with — ``exclude_history`` — each history's items as ``exclude``.  Streams default to the row's index, the slot id."""
        _rollout_args(steps, mode, temperature)
        seqs = [np.asarray(h, dtype=np.uint32).ravel() for h in histories]
        if not seqs:
            raise ValueError("histories: at least one")
        T = int(self.hp.max_sequence_length)
        store = Sessions(self, len(seqs))
        try:
            slots = np.arange(len(seqs), dtype=np.uint32)
            store.append(slots, [s[-T:] if s.size > T else s for s in seqs])
            return store.rollout(slots, steps, mode=mode, temperature=temperature, seed=seed, streams=streams,
                                 exclude=seqs if exclude_history else None, any_of=any_of, none_of=none_of, allow_repeats=allow_repeats,
                                 log_prob=log_prob, final_state=final_state)
        finally:
            store.close()

    def beam_search(self, histories, steps: int, width: int = 4, temperature: float = 1.0, exclude_history: bool = True, any_of=None,
                    none_of=None, allow_repeats: bool = False, partitions: bool = False) -> "Beams":
        """``Sessions.beam_search`` from histories (a list of item-id sequences), DEFINED as rollout's Model form is: a temporary
        store of one slot per history, ``append`` of each history's last max_sequence_length items, and ``store.beam_search`` of all
        slots with — ``exclude_history`` — each history's items as ``exclude``."""
        _beam_args(steps, width, temperature)
        seqs = [np.asarray(h, dtype=np.uint32).ravel() for h in histories]
        if not seqs:
            raise ValueError("histories: at least one")
        T = int(self.hp.max_sequence_length)
        store = Sessions(self, len(seqs))
        try:
            slots = np.arange(len(seqs), dtype=np.uint32)
            store.append(slots, [s[-T:] if s.size > T else s for s in seqs])
            return store.beam_search(slots, steps, width=width, temperature=temperature, exclude=seqs if exclude_history else None,
                                     any_of=any_of, none_of=none_of, allow_repeats=allow_repeats, partitions=partitions)
        finally:
            store.close()

    def item_set(self, item_ids) -> "ItemSet":
        """An item set of this model (sbr_item_set_create; ``ItemSet``): ``item_ids`` in any order, duplicates allowed, each below
        num_items.  Its rows are gathered to the device once; every catalogue call is then offered restricted to the set."""
        return ItemSet(self, item_ids)

    def load_sessions(self, path, capacity=None, remember=None, replay: bool = False) -> "Sessions":
        """A store of this model restored from a file written by ``Sessions.save`` (``persistence.load_sessions``)."""
        from .persistence import load_sessions

        return load_sessions(self, path, capacity=capacity, remember=remember, replay=replay)

    def close(self):
        if getattr(self, "_h", None):
            for st in list(getattr(self, "_stores", ())):  # stores and item sets are destroyed before their model
                st.close()
            self._L.sbr_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _items_csr(items, n: int):
    """``items`` of Sessions.append — a list of item-id sequences, one per slot, or a (ptr, ids) tuple — as (ptr u64 [n + 1], ids
    u32, never empty)."""
    if isinstance(items, tuple):  # a tuple is always the CSR pair
        if len(items) != 2 or len(items[0]) != n + 1:
            raise ValueError("a (ptr, ids) pair with one range per slot")
        ptr = np.ascontiguousarray(items[0], dtype=np.uint64)
        ids = np.ascontiguousarray(items[1], dtype=np.uint32).ravel()
    else:
        if len(items) != n:
            raise ValueError("one item sequence per slot")
        seqs = [np.asarray(x, dtype=np.uint32).ravel() for x in items]
        ptr = np.zeros(n + 1, dtype=np.uint64)
        ptr[1:] = np.cumsum([x.size for x in seqs])
        ids = np.ascontiguousarray(np.concatenate(seqs) if seqs else np.zeros(0, np.uint32), dtype=np.uint32)
    if ids.size == 0:
        ids = np.zeros(1, dtype=np.uint32)
    return ptr, ids


class Sessions:
    """A session store (sbr_sessions_*): ``capacity`` slots of recurrent state on the device — h, c of the LSTM, s of EWMA — each
    advanced by the items appended to it, one cell step per item.  A slot's representation has the bits of
    ``user_representation`` of the items appended since its last reset (an empty slot: of the empty history) as long as they are
    at most max_sequence_length; beyond that a session keeps the recurrence over everything appended where the windowed call
    truncates.  After the model's parameters change (fit, set_param, load) every call but ``reset()`` of the whole store — which
    empties it — and, on a store with seen-item memory, ``replay()`` of the whole store — which recomputes every state from the
    remembered items under the new parameters — raises until one of the two re-binds it; while a fit plan is open on the model
    every call raises.  The object keeps its model alive, and ``Model.close`` closes the model's live stores first.

    With ``remember`` = W > 0 a slot also remembers, on the device, the last W items appended to it since its last reset, in
    append order with repeats (``seen``); ``reset`` and ``set_state`` empty that memory, ``set_seen`` restores it.  ``recommend``
    and ``recommend_diverse`` of such a store exclude each slot's remembered items, united with ``exclude``, as
    ``Model.recommend`` excludes the history; ``score_candidates`` masks nothing."""

    def __init__(self, model: Model, capacity: int, remember: int = 0):
        self.model = model
        self._L = _lib.load()
        h = C.c_void_p()
        remember = int(remember)
        if remember < 0 or remember > SESSIONS_MAX_SEEN:
            raise ValueError(f"remember: 0..{SESSIONS_MAX_SEEN} items per slot")
        if remember:
            _check(self._L.sbr_sessions_create_seen(model._h, int(capacity), remember, C.byref(h)))
        else:
            _check(self._L.sbr_sessions_create(model._h, int(capacity), C.byref(h)))
        self._h = h
        self._seen = remember
        self._lstm = int(model.hp.model) != 2
        if not hasattr(model, "_stores"):
            model._stores = weakref.WeakSet()  # Model.close closes its live stores first
        model._stores.add(self)

    @property
    def capacity(self) -> int:
        n = C.c_uint64()
        _check(self._L.sbr_sessions_capacity(self._h, C.byref(n)))
        return n.value

    @property
    def seen_capacity(self) -> int:
        """Items each slot remembers (0: a store without seen-item memory)."""
        n = C.c_uint32()
        _check(self._L.sbr_sessions_seen_capacity(self._h, C.byref(n)))
        return n.value

    def seen(self, slots):
        """Each named slot's remembered items, oldest first (at most ``seen_capacity``, repeats kept): a list of u32 arrays."""
        sl = self._slots(slots)
        ptr = np.zeros(sl.size + 1, dtype=np.uint64)
        items = np.zeros(max(sl.size * self._seen, 1), dtype=np.uint32)
        _check(self._L.sbr_sessions_get_seen(self._h, _ptr(sl), sl.size, _ptr(ptr), _ptr(items)))
        return Model._per_user(items, ptr)

    def set_seen(self, slots, items):
        """Replaces each named slot's memory with the last ``seen_capacity`` of ``items[i]`` (one sequence per slot, or a CSR
        pair): after ``set_state`` it completes the restore of a checkpoint taken with ``state`` + ``seen``."""
        sl = self._slots(slots)
        ptr, ids = _items_csr(items, sl.size)
        _check(self._L.sbr_sessions_set_seen(self._h, _ptr(sl), sl.size, _ptr(ptr), _ptr(ids)))

    @staticmethod
    def _slots(slots) -> np.ndarray:
        return np.ascontiguousarray(slots, dtype=np.uint32).ravel()

    def append(self, slots, items):
        """Appends ``items[i]`` (a sequence of item ids, possibly empty), in order, to slot ``slots[i]``; ``items`` may also be a
        CSR pair (ptr [n + 1], ids)."""
        sl = self._slots(slots)
        ptr, ids = _items_csr(items, sl.size)
        _check(self._L.sbr_sessions_append(self._h, _ptr(sl), sl.size, _ptr(ptr), _ptr(ids)))

    def lengths(self, slots) -> np.ndarray:
        sl = self._slots(slots)
        out = np.zeros(max(sl.size, 1), dtype=np.uint64)
        _check(self._L.sbr_sessions_lengths(self._h, _ptr(sl), sl.size, _ptr(out)))
        return out[: sl.size]

    def representations(self, slots) -> np.ndarray:
        """[n, embedding_dim] f32: row i is slot ``slots[i]``'s representation."""
        sl = self._slots(slots)
        out = np.zeros((sl.size, self.model.dim), dtype=np.float32)
        _check(self._L.sbr_sessions_representations(self._h, _ptr(sl), sl.size, _ptr(out)))
        return out

    def recommend(self, slots, k: int, exclude=None, any_of=None, none_of=None, include_seen: bool = False):
        """``Model.recommend_reps(self.representations(slots), k, exclude)`` with the scan reading the store's rows in place: items
        [n, k] u32, scores [n, k] f32.  ``exclude`` is None or one sequence of item ids per slot; a store with seen-item memory
        unites it with ``seen`` of the slot unless ``include_seen`` (a ValueError on a store without memory, which has nothing to
        include).  any_of / none_of: ``Model.recommend``'s tag filter, one mask pair per slot of the call."""
        if include_seen and not self._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        flags = RECOMMEND_INCLUDE_HISTORY if include_seen else 0
        sl = self._slots(slots)
        masks = _tag_masks(any_of, none_of, sl.size)
        items = np.zeros((sl.size, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((sl.size, max(int(k), 0)), dtype=np.float32)
        ep, ei = _exclusion_csr(exclude, sl.size)
        if masks is None:
            _check(self._L.sbr_sessions_recommend(self._h, _ptr(sl), sl.size, int(k) & 0xFFFFFFFF, None if ep is None else _ptr(ep),
                                                  None if ei is None else _ptr(ei), flags, _ptr(items), _ptr(scores)))
        else:
            _check(self._L.sbr_sessions_recommend_filtered(self._h, _ptr(sl), sl.size, int(k) & 0xFFFFFFFF,
                                                           None if ep is None else _ptr(ep), None if ei is None else _ptr(ei), flags,
                                                           _ptr(masks[0]), _ptr(masks[1]), _ptr(items), _ptr(scores)))
        return items, scores

    def recommend_capped(self, slots, k: int, cap: int = 1, pool=None, exclude=None, any_of=None, none_of=None,
                         include_seen: bool = False, exact: bool = True):
        """``Model.recommend_capped_reps(self.representations(slots), k, ...)`` with the scan reading the store's rows in place and
        the seen-item memory excluded exactly as in ``recommend`` (sbr_sessions_recommend_capped): (items, scores, complete)."""
        ca, pool = _cap_args(k, cap, pool)
        if include_seen and not self._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        flags = RECOMMEND_INCLUDE_HISTORY if include_seen else 0
        sl = self._slots(slots)
        masks = _tag_masks(any_of, none_of, sl.size)
        items, scores = np.zeros((sl.size, int(k)), dtype=np.uint32), np.zeros((sl.size, int(k)), dtype=np.float32)
        flags_out = np.zeros(max(sl.size, 1), dtype=np.uint8)
        ep, ei = _exclusion_csr(exclude, sl.size)
        _check(self._L.sbr_sessions_recommend_capped(self._h, _ptr(sl), sl.size, int(k), None if ep is None else _ptr(ep),
                                                     None if ei is None else _ptr(ei), flags, C.byref(ca),
                                                     None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]),
                                                     _ptr(items), _ptr(scores), _ptr(flags_out)))

        def top(rows, n):
            return self.recommend_top(sl[rows], n, exclude=None if exclude is None else [exclude[int(r)] for r in rows],
                                      any_of=None if masks is None else masks[0][rows],
                                      none_of=None if masks is None else masks[1][rows], include_seen=include_seen)

        return self.model._capped_finish(top, items, scores, flags_out[: sl.size], int(cap), int(k), pool, exact)

    def recommend_sampled(self, slots, k: int, temperature: float = 1.0, seed: int = 0, streams=None, exclude=None, any_of=None,
                          none_of=None, include_seen: bool = False, log_prob: bool = False):
        """``Model.recommend_sampled_reps(self.representations(slots), k, ...)`` with the scan reading the store's rows in place and
        the seen-item memory excluded exactly as in ``recommend``; streams default to the slot ids, so a session's draw under one
        seed does not depend on who else is in the call."""
        if include_seen and not self._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        flags = RECOMMEND_INCLUDE_HISTORY if include_seen else 0
        sl = self._slots(slots)
        masks = _tag_masks(any_of, none_of, sl.size)
        sa, _keep = _sample_args(temperature, seed, streams, sl.size)
        items, scores, keys = (np.zeros((sl.size, max(int(k), 0)), dtype=dt) for dt in (np.uint32, np.float32, np.float32))
        ep, ei = _exclusion_csr(exclude, sl.size)
        _check(self._L.sbr_sessions_recommend_sampled(self._h, _ptr(sl), sl.size, int(k) & 0xFFFFFFFF, None if ep is None else _ptr(ep),
                                                      None if ei is None else _ptr(ei), flags, C.byref(sa),
                                                      None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]),
                                                      _ptr(items), _ptr(scores), _ptr(keys)))
        if log_prob:  # the draws' propensities: log_partition of the same arguments (Partition.slate_log_prob)
            part = self.log_partition(sl, temperature, exclude=exclude, any_of=any_of, none_of=none_of, include_seen=include_seen)
            return items, scores, keys, part.slate_log_prob(scores)
        return items, scores, keys

    def log_partition(self, slots, temperature: float = 1.0, exclude=None, any_of=None, none_of=None,
                      include_seen: bool = False) -> Partition:
        """``Model.log_partition_reps(self.representations(slots), temperature, ...)`` with the scans reading the store's rows in
        place and the seen-item memory excluded exactly as in ``recommend``."""
        if include_seen and not self._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        flags = RECOMMEND_INCLUDE_HISTORY if include_seen else 0
        sl = self._slots(slots)
        masks = _tag_masks(any_of, none_of, sl.size)
        shift, mass, fb = _partition_outputs(sl.size)
        ep, ei = _exclusion_csr(exclude, sl.size)
        _check(self._L.sbr_sessions_log_partition(self._h, _ptr(sl), sl.size, None if ep is None else _ptr(ep),
                                                  None if ei is None else _ptr(ei), flags, float(np.float32(temperature)),
                                                  None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]),
                                                  _ptr(shift), _ptr(mass), C.byref(fb)))
        return Partition(temperature, shift, mass, fb.value)

    def recommend_diverse(self, slots, k: int, pool: int, trade_off: float = 0.5, metric="cosine", exclude=None, any_of=None,
                          none_of=None):
        """``Model.recommend_diverse_reps(self.representations(slots), k, pool, ...)`` with the scan reading the store's rows in
        place: items [n, k] u32 in pick order, scores [n, k] f32.  A store with seen-item memory always excludes ``seen`` of the
        slot here; ``representations`` + ``Model.recommend_diverse_reps`` is the call that does not."""
        sl = self._slots(slots)
        masks = _tag_masks(any_of, none_of, sl.size)
        items = np.zeros((sl.size, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((sl.size, max(int(k), 0)), dtype=np.float32)
        ep, ei = _exclusion_csr(exclude, sl.size)
        if masks is None:
            _check(self._L.sbr_sessions_recommend_diverse(self._h, _ptr(sl), sl.size, int(k) & 0xFFFFFFFF, int(pool) & 0xFFFFFFFF,
                                                          float(trade_off), _similar_metric(metric), None if ep is None else _ptr(ep),
                                                          None if ei is None else _ptr(ei), _ptr(items), _ptr(scores)))
        else:
            _check(self._L.sbr_sessions_recommend_diverse_filtered(self._h, _ptr(sl), sl.size, int(k) & 0xFFFFFFFF, int(pool) & 0xFFFFFFFF,
                                                                   float(trade_off), _similar_metric(metric),
                                                                   None if ep is None else _ptr(ep), None if ei is None else _ptr(ei),
                                                                   _ptr(masks[0]), _ptr(masks[1]), _ptr(items), _ptr(scores)))
        return items, scores

    def audience(self, items, k: int, slots=None, exclude=None, include_seen: bool = False):
        """Which sessions for this item (sbr_sessions_audience): for each query item ``items[j]`` the k candidate slots whose
        states score it highest — slots [Q, k] u32 (slot ids) and scores [Q, k] f32 with the bits of ``score_candidates`` for
        that (slot, item) pair, score descending, ties to the lower slot id, short rows padded with (RECOMMEND_NO_ITEM, -inf).
        Candidates: ``slots`` (any valid slots, none twice, any order; an empty slot reads the empty-history row), or with
        ``slots=None`` every slot of length > 0.  ``exclude`` is None or one sequence of slot ids per query.  On a store with
        seen-item memory a candidate whose memory holds the query item is left out unless ``include_seen`` (a ValueError on a
        store without memory).  The state rows, the memories and the Q x S scores stay on the device."""
        if include_seen and not self._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        if not 1 <= int(k) <= RECOMMEND_MAX_K:
            raise ValueError(f"k: 1..{RECOMMEND_MAX_K}")
        flags = RECOMMEND_INCLUDE_HISTORY if include_seen else 0
        q = np.ascontiguousarray(items, dtype=np.uint32).ravel()
        sl = None if slots is None else self._slots(slots)
        if sl is not None and np.unique(sl).size != sl.size:
            raise ValueError("slots: none twice")
        out_slots = np.zeros((q.size, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((q.size, max(int(k), 0)), dtype=np.float32)
        ep, ei = _exclusion_csr(exclude, q.size)
        if sl is not None and sl.size == 0:
            sl = np.zeros(1, dtype=np.uint32)  # an empty candidate list, not "every live slot": a valid pointer, zero slots
            nsl = 0
        else:
            nsl = 0 if sl is None else sl.size
        _check(self._L.sbr_sessions_audience(self._h, _ptr(q), q.size, int(k) & 0xFFFFFFFF, None if sl is None else _ptr(sl), nsl,
                                             None if ep is None else _ptr(ep), None if ei is None else _ptr(ei), flags,
                                             _ptr(out_slots), _ptr(scores)))
        return out_slots, scores

    def _recommend_above(self, slots, threshold, exclude, any_of, none_of, include_seen, max_results, order, count_only, n=None):
        if include_seen and not self._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        flags = RECOMMEND_INCLUDE_HISTORY if include_seen else 0
        sl = self._slots(slots)
        masks = _tag_masks(any_of, none_of, sl.size)
        ep, ei = _exclusion_csr(exclude, sl.size)
        return _above(lambda *out: (self._L.sbr_sessions_recommend_above if n is None else self._L.sbr_sessions_recommend_top)(
                          self._h, _ptr(sl), sl.size, out[0], None if ep is None else _ptr(ep), None if ei is None else _ptr(ei), flags,
                          None if masks is None else _ptr(masks[0]), None if masks is None else _ptr(masks[1]), *out[1:]),
                      sl.size, threshold, max_results, order, count_only, n)

    def recommend_above(self, slots, threshold, exclude=None, any_of=None, none_of=None, include_seen: bool = False, max_results=None,
                        order: str = "score") -> Above:
        """``Model.recommend_above_reps(self.representations(slots), threshold, ...)`` with the scan reading the store's rows in
        place and the seen-item memory excluded exactly as in ``recommend`` (sbr_sessions_recommend_above)."""
        return self._recommend_above(slots, threshold, exclude, any_of, none_of, include_seen, max_results, order, False)

    def rank_targets(self, slots, targets, exclude=None, any_of=None, none_of=None, include_seen: bool = False) -> np.ndarray:
        """``Model.rank_targets_reps(self.representations(slots), targets, exclude=seen + exclude, ...)`` with the scan reading the
        store's rows in place (sbr_rank_targets_rows): ``targets`` is one sequence of item ids per slot, or a CSR pair (ptr, ids);
        the slot's seen items are masked as ``recommend`` excludes them unless ``include_seen``.  One u32 per target, in target
        order.  Prequential evaluation is this call, then ``append`` of the same events."""
        sl = self._slots(slots)
        tp, ti = _items_csr(targets, sl.size)
        return _rank_targets_rows(self._L.sbr_rank_targets_rows, self.model._h, _check,
                                  _ModelRows(self.model)._store(self, sl, exclude, any_of, none_of, include_seen), tp, ti)

    def count_above(self, slots, threshold, exclude=None, any_of=None, none_of=None, include_seen: bool = False) -> np.ndarray:
        """``recommend_above(...).counts`` without writing any pair: one scan."""
        return self._recommend_above(slots, threshold, exclude, any_of, none_of, include_seen, None, "id", True)

    def _audience_above(self, items, threshold, slots, exclude, include_seen, max_results, order, count_only, n=None):
        if include_seen and not self._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        flags = RECOMMEND_INCLUDE_HISTORY if include_seen else 0
        q = np.ascontiguousarray(items, dtype=np.uint32).ravel()
        sl = None if slots is None else self._slots(slots)
        if sl is not None and np.unique(sl).size != sl.size:
            raise ValueError("slots: none twice")
        ep, ei = _exclusion_csr(exclude, q.size)
        if sl is not None and sl.size == 0:
            sl = np.zeros(1, dtype=np.uint32)  # an empty candidate list, not "every live slot": a valid pointer, zero slots
            nsl = 0
        else:
            nsl = 0 if sl is None else sl.size
        return _above(lambda *out: (self._L.sbr_sessions_audience_above if n is None else self._L.sbr_sessions_audience_top)(
                          self._h, _ptr(q), q.size, out[0], None if sl is None else _ptr(sl), nsl, None if ep is None else _ptr(ep),
                          None if ei is None else _ptr(ei), flags, *out[1:]),
                      q.size, threshold, max_results, order, count_only, n)

    def audience_above(self, items, threshold, slots=None, exclude=None, include_seen: bool = False, max_results=None,
                       order: str = "score") -> Above:
        """Who should hear about this item (sbr_sessions_audience_above): for each query item ``items[j]`` EVERY candidate slot
        whose state scores it >= ``threshold`` (a scalar or one per query) — an ``Above`` over the queries, slot ids with the bits
        of ``score_candidates``.  Candidates, ``exclude`` and the seen-item memory as in ``audience``; no k and no cap of 1 024."""
        return self._audience_above(items, threshold, slots, exclude, include_seen, max_results, order, False)

    def count_audience_above(self, items, threshold, slots=None, exclude=None, include_seen: bool = False) -> np.ndarray:
        """``audience_above(...).counts`` without writing any pair: one scan."""
        return self._audience_above(items, threshold, slots, exclude, include_seen, None, "id", True)

    def recommend_top(self, slots, n, exclude=None, any_of=None, none_of=None, include_seen: bool = False, max_results=None,
                      order: str = "score") -> Above:
        """``Model.recommend_top_reps(self.representations(slots), n, ...)`` with the scan reading the store's rows in place and the
        seen-item memory excluded exactly as in ``recommend`` (sbr_sessions_recommend_top)."""
        return self._recommend_above(slots, None, exclude, any_of, none_of, include_seen, max_results, order, False, n)

    def nth_score(self, slots, n, exclude=None, any_of=None, none_of=None, include_seen: bool = False):
        """``(cuts, counts)`` of ``recommend_top(...)`` from the select alone: no pair is written."""
        return self._recommend_above(slots, None, exclude, any_of, none_of, include_seen, None, "id", True, n)

    def audience_top(self, items, n, slots=None, exclude=None, include_seen: bool = False, max_results=None, order: str = "score") -> Above:
        """We can reach n people: which n (sbr_sessions_audience_top)?  For each query item ``items[j]`` the exact best ``n`` (a
        scalar or one per query; no cap of 1 024) candidate slots — an ``Above`` over the queries with ``cuts``, slot ids with the
        bits of ``score_candidates``.  Candidates, ``exclude`` and the seen-item memory as in ``audience``."""
        return self._audience_above(items, None, slots, exclude, include_seen, max_results, order, False, n)

    def nth_audience_score(self, items, n, slots=None, exclude=None, include_seen: bool = False):
        """``(cuts, counts)`` of ``audience_top(...)`` from the select alone."""
        return self._audience_above(items, None, slots, exclude, include_seen, None, "id", True, n)

    def score_candidates(self, slots, candidates):
        """``Model.score_candidates_reps`` on the slots' representations, read in place: one f32 array per slot, in candidate
        order.  ``candidates``: one sequence of item ids per slot, or a CSR pair (ptr, ids)."""
        sl = self._slots(slots)
        cp, ci = _items_csr(candidates, sl.size)
        scores = np.zeros(max(int(cp[-1] - cp[0]), 1), dtype=np.float32)
        _check(self._L.sbr_sessions_score_candidates(self._h, _ptr(sl), sl.size, _ptr(cp), _ptr(ci), _ptr(scores)))
        return Model._per_user(scores, cp)

    def reset(self, slots=None):
        """Empties the named slots; ``slots=None``: every slot, and the store is re-bound to the model's current parameters."""
        if slots is None:
            _check(self._L.sbr_sessions_reset_all(self._h))
        else:
            sl = self._slots(slots)
            _check(self._L.sbr_sessions_reset(self._h, _ptr(sl), sl.size))

    def replay(self, slots=None) -> int:
        """Recomputes states from the remembered items, on the device, under the model's current parameters
        (sbr_sessions_replay); a store with seen-item memory only.  ``slots=None``: every slot, and the store is re-bound to the
        current parameters — the call for a store gone stale after a retrain.  Otherwise the named slots of a current store
        (repeats count once); the others keep their bits.  A replayed slot holds the bits a fresh slot holds after ``append`` of
        ``seen`` of it, and that many items as its length — at most ``seen_capacity``: a slot that was told more keeps the
        recurrence over what it still remembers; a slot with an empty memory becomes empty.  The memory itself is unchanged.
        Returns the number of slots that had a non-empty memory."""
        n = C.c_uint64()
        if slots is None:
            _check(self._L.sbr_sessions_replay(self._h, None, 0, C.byref(n)))
        else:
            sl = self._slots(slots)
            if sl.size == 0:
                sl = np.zeros(1, dtype=np.uint32)  # no slots, not "every slot": a valid pointer, zero slots
                _check(self._L.sbr_sessions_replay(self._h, _ptr(sl), 0, C.byref(n)))
            else:
                _check(self._L.sbr_sessions_replay(self._h, _ptr(sl), sl.size, C.byref(n)))
        return n.value

    def save(self, path) -> None:
        """The store's live slots — states, lengths, memories — into an ``.npz`` (``persistence.save_sessions``); a stale store
        raises: ``replay()`` first."""
        from .persistence import save_sessions

        save_sessions(self, path)

    def rollout(self, slots, steps: int, mode: str = "greedy", temperature: float = 1.0, seed: int = 0, streams=None, exclude=None,
                any_of=None, none_of=None, include_seen: bool = False, allow_repeats: bool = False, log_prob: bool = False,
                final_state: bool = False) -> Rollout:
        """Each slot's next ``steps`` items, each chosen given the ones before it, picked and fed back on the device
        (sbr_sessions_rollout) — what a host loop of ``recommend(slots, 1, exclude)`` + ``append`` + a rebuilt ``exclude`` returns,
        without its round trips and WITHOUT writing the store: a rollout is hypothetical, ``append(slots, result.rows())`` makes it
        happen.  Step j picks among what ``recommend`` would offer at call time (``exclude``, the seen-item memory unless
        ``include_seen``, ``any_of`` / ``none_of``) minus picks 0 .. j - 1 — with ``allow_repeats`` the picks stay eligible — scored
        against the state after those picks, advanced as ``append`` advances it.  ``mode="greedy"``: the top-1 in every call's
        order.  ``mode="sample"``: the one draw of ``recommend_sampled(k=1, temperature, seed=seed + j, streams)``; ``streams``
        default to the slot ids, so the same (seed, streams) returns the same trajectory whatever the batch.  A row with nothing
        left ends: padding from there on, ``lengths[i]`` its real steps.  ``log_prob``: each step's exact partition at
        ``temperature`` and the pick's log-probability under it, in either mode.  ``final_state``: the states after all picks.
        The insert of a pick into its row's exclusion list costs O(list) per step; steps <= 1 024."""
        return self._rollout(None, slots, steps, mode, temperature, seed, streams, exclude, any_of, none_of, include_seen, allow_repeats,
                             log_prob, final_state)

    def _rollout(self, item_set, slots, steps, mode, temperature, seed, streams, exclude, any_of, none_of, include_seen, allow_repeats,
                 log_prob, final_state) -> Rollout:
        """``rollout`` of this store, or within ``item_set`` (sbr_item_set_rollout; None: the catalogue).  Every argument is
        checked here before the library is called."""
        from ._abi import ROLLOUT_ALLOW_REPEATS, ROLLOUT_INCLUDE_SEEN, ROLLOUT_SAMPLE, SbrRolloutArgs

        steps, sample = _rollout_args(steps, mode, temperature)
        if include_seen and not self._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        sl = self._slots(slots)
        n = sl.size
        masks = _tag_masks(any_of, none_of, n)
        sa, _keep = _sample_args(temperature, seed, streams, n)
        ep, ei = _exclusion_csr(exclude, n)
        ra = SbrRolloutArgs()
        ra.steps = steps
        ra.flags = (ROLLOUT_SAMPLE if sample else 0) | (ROLLOUT_ALLOW_REPEATS if allow_repeats else 0) | (ROLLOUT_INCLUDE_SEEN if include_seen else 0)
        ra.sample = sa
        items = np.zeros((n, steps), dtype=np.uint32)
        scores = np.zeros((n, steps), dtype=np.float32)
        keys = np.zeros((n, steps), dtype=np.float32) if sample else None
        lengths = np.zeros(max(n, 1), dtype=np.uint32)
        shift = np.zeros((n, steps), dtype=np.float32) if log_prob else None
        mass = np.zeros((n, steps), dtype=np.uint64) if log_prob else None
        fb = C.c_uint32(0)
        h = np.zeros((n, self.model.dim), dtype=np.float32) if final_state else None
        c = np.zeros((n, self.model.dim), dtype=np.float32) if final_state and self._lstm else None

        def opt(a):
            return None if a is None else _ptr(a)

        outs = (_ptr(items), _ptr(scores), opt(keys), _ptr(lengths), opt(shift), opt(mass), C.byref(fb) if log_prob else None, opt(h), opt(c))
        if item_set is None:
            _check(self._L.sbr_sessions_rollout(self._h, _ptr(sl), n, C.byref(ra), opt(ep), opt(ei), None if masks is None else _ptr(masks[0]),
                                                None if masks is None else _ptr(masks[1]), *outs))
        else:
            src = self._set_rows(sl, masks, ep, ei)
            item_set._check(self._L.sbr_item_set_rollout(item_set._h, C.byref(src.desc), n, C.byref(ra), *outs))
        lengths = lengths[:n]
        out = Rollout(items, scores, lengths, keys=keys)
        if log_prob:  # one partition row per (row, step): the host's one statement of the weights, no second exponential
            part = Partition(temperature, shift.reshape(-1), mass.reshape(-1), fb.value)
            lp = part.log_prob(scores.reshape(-1, 1)).reshape(n, steps)
            lp[items == RECOMMEND_NO_ITEM] = np.nan
            out.shift, out.mass, out.frac_bits, out.log_prob = shift, mass, fb.value, lp
        if final_state:
            out.h, out.c, out.len = h, c, self.lengths(sl) + lengths.astype(np.uint64)
        return out

    def beam_search(self, slots, steps: int, width: int = 4, temperature: float = 1.0, exclude=None, any_of=None, none_of=None,
                    include_seen: bool = False, allow_repeats: bool = False, partitions: bool = False) -> Beams:
        """The ``width`` most likely next-``steps`` continuations of each slot, searched on the device (sbr_sessions_beam_search;
        greedy, deterministic) WITHOUT writing the store.  Eligibility is ``rollout``'s: ``exclude``, the seen-item memory unless
        ``include_seen``, ``any_of`` / ``none_of``, minus the beam's own path unless ``allow_repeats``.  At every step each live
        beam offers its first ``width`` eligible items in every call's order, each offer's log-probability lp is the contract's f32
        approximation of log(w / mass) under ``log_partition`` at ``temperature`` (finite where the scores are; not
        ``Partition.log_prob``, which is -inf where w == 0), and the row keeps the ``width`` best offers by (cumulative lp
        descending, parent beam ascending, offer position ascending).  ``partitions``: each (beam, step)'s exact shift and mass too.
        With width 1 the items are greedy ``rollout``'s."""
        return self._beam_search(None, slots, steps, width, temperature, exclude, any_of, none_of, include_seen, allow_repeats, partitions)

    def _beam_search(self, item_set, slots, steps, width, temperature, exclude, any_of, none_of, include_seen, allow_repeats,
                     partitions) -> Beams:
        """``beam_search`` of this store, or within ``item_set`` (sbr_item_set_beam_search; None: the catalogue).  Every argument
        is checked here before the library is called."""
        from ._abi import ROLLOUT_ALLOW_REPEATS, ROLLOUT_INCLUDE_SEEN, SbrBeamArgs

        steps, width = _beam_args(steps, width, temperature)
        if include_seen and not self._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        sl = self._slots(slots)
        n = sl.size
        masks = _tag_masks(any_of, none_of, n)
        ep, ei = _exclusion_csr(exclude, n)
        ba = SbrBeamArgs()
        ba.steps, ba.width = steps, width
        ba.flags = (ROLLOUT_ALLOW_REPEATS if allow_repeats else 0) | (ROLLOUT_INCLUDE_SEEN if include_seen else 0)
        ba.temperature = float(np.float32(temperature))
        shape = (n, width, steps)
        items = np.zeros(shape, dtype=np.uint32)
        scores = np.zeros(shape, dtype=np.float32)
        step_lp = np.zeros(shape, dtype=np.float32)
        cum = np.zeros((n, width), dtype=np.float32)
        lengths = np.zeros(max(n, 1), dtype=np.uint32)
        beams = np.zeros(max(n, 1), dtype=np.uint32)
        shift = np.zeros(shape, dtype=np.float32) if partitions else None
        mass = np.zeros(shape, dtype=np.uint64) if partitions else None
        fb = C.c_uint32(0)

        def opt(a):
            return None if a is None else _ptr(a)

        outs = (_ptr(items), _ptr(scores), _ptr(step_lp), _ptr(cum), _ptr(lengths), _ptr(beams), opt(shift), opt(mass),
                C.byref(fb) if partitions else None)
        if item_set is None:
            _check(self._L.sbr_sessions_beam_search(self._h, _ptr(sl), n, C.byref(ba), opt(ep), opt(ei), None if masks is None else _ptr(masks[0]),
                                                    None if masks is None else _ptr(masks[1]), *outs))
        else:
            src = self._set_rows(sl, masks, ep, ei)
            item_set._check(self._L.sbr_item_set_beam_search(item_set._h, C.byref(src.desc), n, C.byref(ba), *outs))
        return Beams(items, scores, step_lp, cum, lengths[:n], beams[:n], shift=shift, mass=mass, frac_bits=fb.value if partitions else None)

    def _set_rows(self, sl, masks, ep, ei) -> "_ScanRows":
        """The store descriptor of a rollout or beam search through an item set: flags 0, include_seen goes in the args."""
        buf = sl if sl.size else np.zeros(1, dtype=np.uint32)
        return _scan_rows(sl.size, masks, ep, ei, (self, buf), None, store=self._h.value, slots=buf.ctypes.data)

    def state(self, slots):
        """Checkpoint of the named slots: (h [n, embedding_dim], c likewise — None for EWMA —, len [n] u64)."""
        sl = self._slots(slots)
        h = np.zeros((sl.size, self.model.dim), dtype=np.float32)
        c = np.zeros((sl.size, self.model.dim), dtype=np.float32) if self._lstm else None
        n = np.zeros(max(sl.size, 1), dtype=np.uint64)
        _check(self._L.sbr_sessions_get_state(self._h, _ptr(sl), sl.size, _ptr(h), None if c is None else _ptr(c), _ptr(n)))
        return h, c, n[: sl.size]

    def set_state(self, slots, h, c, lengths):
        """Restores a checkpoint taken by ``state`` (of this store or another one of the same model and parameters)."""
        sl = self._slots(slots)
        h = np.ascontiguousarray(h, dtype=np.float32).reshape(sl.size, self.model.dim)
        c = None if c is None else np.ascontiguousarray(c, dtype=np.float32).reshape(sl.size, self.model.dim)
        n = np.ascontiguousarray(lengths, dtype=np.uint64).ravel()
        if n.size != sl.size:
            raise ValueError("one length per slot")
        _check(self._L.sbr_sessions_set_state(self._h, _ptr(sl), sl.size, _ptr(h), None if c is None else _ptr(c), _ptr(n)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.sbr_sessions_destroy(self._h)
            self._h = None
            self.model._stores.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ScanRows:
    """The rows of one call through an ItemSet: the sbr_scan_rows descriptor, the number of rows, the arrays it points into (kept
    alive here) and ``take(rows)``, the same source restricted to some rows of the call (recommend_capped's completion)."""

    def __init__(self, desc, n: int, keep, take):
        self.desc, self.n, self._keep, self.take = desc, n, keep, take


def _scan_rows(n: int, masks, ep, ei, keep, take, **fields):
    from ._abi import SbrScanRows

    d = SbrScanRows()
    for name, value in fields.items():
        setattr(d, name, value)
    if ep is not None:
        d.excl_ptr, d.excl_items = ep.ctypes.data, ei.ctypes.data
    if masks is not None:
        d.any_of, d.none_of = masks[0].ctypes.data, masks[1].ctypes.data
    return _ScanRows(d, n, (keep, masks, ep, ei), take)


class ItemSet:
    """An item set of a model (sbr_item_set_*; ``Model.item_set(item_ids)``): the sorted unique ids ``items`` and a device copy
    of their embedding rows and biases, gathered once, so that every catalogue call restricted to the set costs what the set
    costs, not what the catalogue does.  Every method returns, bit for bit, what the model's method of the same name returns
    with every item outside the set added to each row's exclusions — catalogue ids, predict's score bits, the same noise per
    (seed, stream, item), the model's ``frac_bits``.  Histories, ``exclude`` lists and a session's seen items stay catalogue
    ids; entries outside the set are ignored.  After the model's parameters change (fit, set_param, load) every call raises
    (``errors.InvalidArgument``, a ValueError) until ``refresh()`` gathers the rows again, and likewise while a fit plan is
    open; ``set_item_tags`` / ``set_item_groups`` take effect without one.  An empty set is legal.  ``on(store)`` gives the
    session store's scan methods through the set.  The object keeps its model alive; ``Model.close`` closes its sets first."""

    def __init__(self, model: "Model", item_ids):
        self.model = model
        self._L = _lib.load()
        ids = np.ascontiguousarray(np.asarray(item_ids, dtype=np.int64).ravel())
        if ids.size and (ids.min() < 0 or ids.max() >= int(model.hp.num_items)):
            raise ValueError(f"item_set: ids must be below num_items = {int(model.hp.num_items)}")
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        h = C.c_void_p()
        self._h = None
        self._check(self._L.sbr_item_set_create(model._h, _ptr(ids) if ids.size else None, ids.size, C.byref(h)))
        self._h = h
        if not hasattr(model, "_stores"):
            model._stores = weakref.WeakSet()
        model._stores.add(self)

    @staticmethod
    def _check(st: int):
        if st == Status.INVALID_ARGUMENT:
            raise InvalidArgument(Status(st), _lib.load().sbr_status_string(st).decode())
        _check(st)

    @property
    def size(self) -> int:
        n = C.c_uint64()
        self._check(self._L.sbr_item_set_size(self._h, C.byref(n)))
        return n.value

    def __len__(self) -> int:
        return self.size

    @property
    def items(self) -> np.ndarray:
        """The set's ids, sorted and unique (u32)."""
        out = np.zeros(max(self.size, 1), dtype=np.uint32)
        self._check(self._L.sbr_item_set_items(self._h, _ptr(out)))
        return out[: self.size]

    def refresh(self):
        """Gathers the set's rows again from the model's current parameters (sbr_item_set_refresh)."""
        self._check(self._L.sbr_item_set_refresh(self._h))
        return self

    def on(self, store: "Sessions") -> "ItemSetSessions":
        """The scan methods of a session store of this set's model, through the set."""
        return ItemSetSessions(self, store)

    def close(self):
        if getattr(self, "_h", None):
            self._L.sbr_item_set_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the sources of rows ----
    def _hist(self, user_ptr, item_ids, include_history, any_of, none_of) -> _ScanRows:
        up = np.ascontiguousarray(user_ptr, dtype=np.uint64)
        it = np.ascontiguousarray(item_ids, dtype=np.uint32)
        if it.size == 0:
            it = np.zeros(1, dtype=np.uint32)
        nu = max(len(up) - 1, 0)
        masks = _tag_masks(any_of, none_of, nu)

        def take(rows):
            sp = np.zeros(rows.size + 1, dtype=np.uint64)
            sp[1:] = np.cumsum((up[rows + 1] - up[rows]).astype(np.int64))
            si = np.concatenate([it[int(up[r]) : int(up[r + 1])] for r in rows]) if rows.size else np.zeros(0, np.uint32)
            return self._hist(sp, si, include_history, None if masks is None else masks[0][rows], None if masks is None else masks[1][rows])

        return _scan_rows(nu, masks, None, None, (up, it), take, user_ptr=up.ctypes.data, item_ids=it.ctypes.data,
                          flags=RECOMMEND_INCLUDE_HISTORY if include_history else 0)

    def _reps(self, reps, exclude, any_of, none_of) -> _ScanRows:
        reps = np.ascontiguousarray(reps, dtype=np.float32).reshape(-1, self.model.dim)
        nu = reps.shape[0]
        masks = _tag_masks(any_of, none_of, nu)
        ep, ei = _exclusion_csr(exclude, nu)
        buf = reps if nu else np.zeros((1, self.model.dim), dtype=np.float32)

        def take(rows):
            return self._reps(reps[rows], None if exclude is None else [exclude[int(r)] for r in rows],
                              None if masks is None else masks[0][rows], None if masks is None else masks[1][rows])

        return _scan_rows(nu, masks, ep, ei, buf, take, reps=buf.ctypes.data)

    def _store(self, store, slots, exclude, any_of, none_of, include_seen) -> _ScanRows:
        if include_seen and not store._seen:
            raise ValueError("include_seen: this store has no seen-item memory (sessions(capacity, remember=W))")
        sl = Sessions._slots(slots)
        masks = _tag_masks(any_of, none_of, sl.size)
        ep, ei = _exclusion_csr(exclude, sl.size)
        buf = sl if sl.size else np.zeros(1, dtype=np.uint32)

        def take(rows):
            return self._store(store, sl[rows], None if exclude is None else [exclude[int(r)] for r in rows],
                               None if masks is None else masks[0][rows], None if masks is None else masks[1][rows], include_seen)

        return _scan_rows(sl.size, masks, ep, ei, (store, buf), take, store=store._h.value, slots=buf.ctypes.data,
                          flags=RECOMMEND_INCLUDE_HISTORY if include_seen else 0)

    # ---- the families, over any source ----
    def _recommend(self, src: _ScanRows, k: int):
        items = np.zeros((src.n, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((src.n, max(int(k), 0)), dtype=np.float32)
        self._check(self._L.sbr_item_set_recommend(self._h, C.byref(src.desc), src.n, int(k) & 0xFFFFFFFF, _ptr(items), _ptr(scores)))
        return items, scores

    def _diverse(self, src: _ScanRows, k: int, pool: int, trade_off, metric):
        items = np.zeros((src.n, max(int(k), 0)), dtype=np.uint32)
        scores = np.zeros((src.n, max(int(k), 0)), dtype=np.float32)
        self._check(self._L.sbr_item_set_recommend_diverse(self._h, C.byref(src.desc), src.n, int(k) & 0xFFFFFFFF, int(pool) & 0xFFFFFFFF,
                                                           float(trade_off), _similar_metric(metric), _ptr(items), _ptr(scores)))
        return items, scores

    def _log_partition(self, src: _ScanRows, temperature) -> Partition:
        shift, mass, fb = _partition_outputs(src.n)
        self._check(self._L.sbr_item_set_log_partition(self._h, C.byref(src.desc), src.n, float(np.float32(temperature)), _ptr(shift),
                                                       _ptr(mass), C.byref(fb)))
        return Partition(temperature, shift, mass, fb.value)

    def _sampled(self, src: _ScanRows, k: int, temperature, seed, streams, log_prob: bool):
        sa, _keep = _sample_args(temperature, seed, streams, src.n)
        items, scores, keys = (np.zeros((src.n, max(int(k), 0)), dtype=dt) for dt in (np.uint32, np.float32, np.float32))
        self._check(self._L.sbr_item_set_recommend_sampled(self._h, C.byref(src.desc), src.n, int(k) & 0xFFFFFFFF, C.byref(sa), _ptr(items),
                                                           _ptr(scores), _ptr(keys)))
        if log_prob:  # the draws' propensities: the set's own log_partition of the same rows
            return items, scores, keys, self._log_partition(src, temperature).slate_log_prob(scores)
        return items, scores, keys

    def _above(self, src: _ScanRows, threshold, max_results, order, count_only, n=None):
        def call(*out):  # the set's own check raises; _above's then sees OK
            self._check((self._L.sbr_item_set_recommend_above if n is None else self._L.sbr_item_set_recommend_top)(
                self._h, C.byref(src.desc), src.n, *out))
            return int(Status.OK)

        return _above(call, src.n, threshold, max_results, order, count_only, n)

    def _capped(self, src: _ScanRows, k: int, cap: int, pool, exact: bool):
        ca, pool = _cap_args(k, cap, pool)
        items, scores = np.zeros((src.n, int(k)), dtype=np.uint32), np.zeros((src.n, int(k)), dtype=np.float32)
        flags_out = np.zeros(max(src.n, 1), dtype=np.uint8)
        self._check(self._L.sbr_item_set_recommend_capped(self._h, C.byref(src.desc), src.n, int(k), C.byref(ca), _ptr(items), _ptr(scores),
                                                          _ptr(flags_out)))
        complete = flags_out[: src.n].astype(bool)
        if exact and not complete.all():  # short rows are finished with the set's own recommend_top
            groups = getattr(self.model, "_groups", None)
            capped_complete(lambda rows, n: self._above(src.take(rows), None, None, "score", False, n), items, scores, complete,
                            self.model.item_groups() if groups is None else groups, int(cap), int(k), pool, max(self.size, 1))
        return items, scores, complete

    def _rank_targets(self, src: _ScanRows, target_ptr, target_items) -> np.ndarray:
        return _rank_targets_rows(self._L.sbr_item_set_rank_targets, self._h, self._check, src, target_ptr, target_items)

    # ---- histories: Model's methods of the same names ----
    def rank_targets(self, user_ptr, item_ids, target_ptr, target_items, include_history: bool = False, any_of=None,
                     none_of=None) -> np.ndarray:
        """``Model.rank_targets`` within the set (sbr_item_set_rank_targets): a target outside the set has rank num_items, the
        catalogue's."""
        return self._rank_targets(self._hist(user_ptr, item_ids, include_history, any_of, none_of), target_ptr, target_items)

    def recommend(self, user_ptr, item_ids, k: int, include_history: bool = False, any_of=None, none_of=None):
        """``Model.recommend`` within the set (sbr_item_set_recommend)."""
        return self._recommend(self._hist(user_ptr, item_ids, include_history, any_of, none_of), k)

    def recommend_sampled(self, user_ptr, item_ids, k: int, temperature: float = 1.0, seed: int = 0, streams=None,
                          include_history: bool = False, any_of=None, none_of=None, log_prob: bool = False):
        """``Model.recommend_sampled`` within the set: the same (seed, stream) draws what the model draws with the set's complement
        excluded.  ``log_prob=True`` goes through the set's own ``log_partition``."""
        return self._sampled(self._hist(user_ptr, item_ids, include_history, any_of, none_of), k, temperature, seed, streams, log_prob)

    def log_partition(self, user_ptr, item_ids, temperature: float = 1.0, include_history: bool = False, any_of=None,
                      none_of=None) -> Partition:
        """``Model.log_partition`` within the set; ``frac_bits`` is the model's."""
        return self._log_partition(self._hist(user_ptr, item_ids, include_history, any_of, none_of), temperature)

    def recommend_above(self, user_ptr, item_ids, threshold, include_history: bool = False, any_of=None, none_of=None,
                        max_results=None, order: str = "score") -> Above:
        """``Model.recommend_above`` within the set."""
        return self._above(self._hist(user_ptr, item_ids, include_history, any_of, none_of), threshold, max_results, order, False)

    def count_above(self, user_ptr, item_ids, threshold, include_history: bool = False, any_of=None, none_of=None) -> np.ndarray:
        return self._above(self._hist(user_ptr, item_ids, include_history, any_of, none_of), threshold, None, "id", True)

    def recommend_top(self, user_ptr, item_ids, n, include_history: bool = False, any_of=None, none_of=None, max_results=None,
                      order: str = "score") -> Above:
        """``Model.recommend_top`` within the set."""
        return self._above(self._hist(user_ptr, item_ids, include_history, any_of, none_of), None, max_results, order, False, n)

    def nth_score(self, user_ptr, item_ids, n, include_history: bool = False, any_of=None, none_of=None):
        return self._above(self._hist(user_ptr, item_ids, include_history, any_of, none_of), None, None, "id", True, n)

    def recommend_capped(self, user_ptr, item_ids, k: int, cap: int = 1, pool=None, include_history: bool = False, any_of=None,
                         none_of=None, exact: bool = True):
        """``Model.recommend_capped`` within the set; ``exact=True`` finishes short rows with the set's ``recommend_top``."""
        return self._capped(self._hist(user_ptr, item_ids, include_history, any_of, none_of), k, cap, pool, exact)

    def recommend_diverse(self, user_ptr, item_ids, k: int, pool: int, trade_off: float = 0.5, metric="cosine",
                          include_history: bool = False, any_of=None, none_of=None):
        """``Model.recommend_diverse`` within the set: the pool is the set's ``recommend`` row."""
        return self._diverse(self._hist(user_ptr, item_ids, include_history, any_of, none_of), k, pool, trade_off, metric)

    def _temporary_store(self, histories):
        """Model.rollout's temporary store: one slot per history, each history's last max_sequence_length items appended."""
        seqs = [np.asarray(h, dtype=np.uint32).ravel() for h in histories]
        if not seqs:
            raise ValueError("histories: at least one")
        T = int(self.model.hp.max_sequence_length)
        store = Sessions(self.model, len(seqs))
        try:
            slots = np.arange(len(seqs), dtype=np.uint32)
            store.append(slots, [s[-T:] if s.size > T else s for s in seqs])
        except BaseException:
            store.close()
            raise
        return store, slots, seqs

    def rollout(self, histories, steps: int, mode: str = "greedy", temperature: float = 1.0, seed: int = 0, streams=None,
                exclude_history: bool = True, any_of=None, none_of=None, allow_repeats: bool = False, log_prob: bool = False,
                final_state: bool = False) -> Rollout:
        """``Model.rollout`` within the set, DEFINED as it is: a temporary store of one slot per history, ``append`` of each
        history's last max_sequence_length items, and ``on(store).rollout`` of all slots with — ``exclude_history`` — each
        history's items as ``exclude``."""
        _rollout_args(steps, mode, temperature)
        store, slots, seqs = self._temporary_store(histories)
        try:
            return self.on(store).rollout(slots, steps, mode=mode, temperature=temperature, seed=seed, streams=streams,
                                          exclude=seqs if exclude_history else None, any_of=any_of, none_of=none_of,
                                          allow_repeats=allow_repeats, log_prob=log_prob, final_state=final_state)
        finally:
            store.close()

    def beam_search(self, histories, steps: int, width: int = 4, temperature: float = 1.0, exclude_history: bool = True, any_of=None,
                    none_of=None, allow_repeats: bool = False, partitions: bool = False) -> "Beams":
        """``Model.beam_search`` within the set, DEFINED as ``rollout``'s histories form is, through ``on(store).beam_search``."""
        _beam_args(steps, width, temperature)
        store, slots, seqs = self._temporary_store(histories)
        try:
            return self.on(store).beam_search(slots, steps, width=width, temperature=temperature, exclude=seqs if exclude_history else None,
                                              any_of=any_of, none_of=none_of, allow_repeats=allow_repeats, partitions=partitions)
        finally:
            store.close()

    # ---- representations ----
    def rank_targets_reps(self, reps, target_ptr, target_items, exclude=None, any_of=None, none_of=None) -> np.ndarray:
        return self._rank_targets(self._reps(reps, exclude, any_of, none_of), target_ptr, target_items)

    def recommend_reps(self, reps, k: int, exclude=None, any_of=None, none_of=None):
        return self._recommend(self._reps(reps, exclude, any_of, none_of), k)

    def recommend_sampled_reps(self, reps, k: int, temperature: float = 1.0, seed: int = 0, streams=None, exclude=None, any_of=None,
                               none_of=None, log_prob: bool = False):
        return self._sampled(self._reps(reps, exclude, any_of, none_of), k, temperature, seed, streams, log_prob)

    def log_partition_reps(self, reps, temperature: float = 1.0, exclude=None, any_of=None, none_of=None) -> Partition:
        return self._log_partition(self._reps(reps, exclude, any_of, none_of), temperature)

    def recommend_above_reps(self, reps, threshold, exclude=None, any_of=None, none_of=None, max_results=None,
                             order: str = "score") -> Above:
        return self._above(self._reps(reps, exclude, any_of, none_of), threshold, max_results, order, False)

    def count_above_reps(self, reps, threshold, exclude=None, any_of=None, none_of=None) -> np.ndarray:
        return self._above(self._reps(reps, exclude, any_of, none_of), threshold, None, "id", True)

    def recommend_top_reps(self, reps, n, exclude=None, any_of=None, none_of=None, max_results=None, order: str = "score") -> Above:
        return self._above(self._reps(reps, exclude, any_of, none_of), None, max_results, order, False, n)

    def nth_score_reps(self, reps, n, exclude=None, any_of=None, none_of=None):
        return self._above(self._reps(reps, exclude, any_of, none_of), None, None, "id", True, n)

    def recommend_capped_reps(self, reps, k: int, cap: int = 1, pool=None, exclude=None, any_of=None, none_of=None, exact: bool = True):
        return self._capped(self._reps(reps, exclude, any_of, none_of), k, cap, pool, exact)

    def recommend_diverse_reps(self, reps, k: int, pool: int, trade_off: float = 0.5, metric="cosine", exclude=None, any_of=None,
                               none_of=None):
        return self._diverse(self._reps(reps, exclude, any_of, none_of), k, pool, trade_off, metric)


class _ModelRows:
    """The three sources of rows as ``ItemSet`` names them, for a descriptor call on the model itself (no set)."""

    def __init__(self, model: "Model"):
        self.model = model

    _hist, _reps, _store = ItemSet._hist, ItemSet._reps, ItemSet._store


def _rank_targets_rows(fn, handle, check, src: _ScanRows, target_ptr, target_items) -> np.ndarray:
    """The eligible-ranks call ``fn`` (sbr_rank_targets_rows / sbr_item_set_rank_targets) over the rows ``src``: one u32 per
    target, in target order."""
    tp = np.ascontiguousarray(target_ptr, dtype=np.uint64)
    ti = np.ascontiguousarray(target_items, dtype=np.uint32)
    if tp.ndim != 1 or tp.size != src.n + 1:
        raise ValueError("one target range per row")
    nt = int(tp[-1] - tp[0])  # ti may hold a dummy entry where there is no target at all
    ranks = np.zeros(max(nt, 1), dtype=np.uint32)
    buf = ti if ti.size else np.zeros(1, dtype=np.uint32)
    check(fn(handle, C.byref(src.desc), src.n, _ptr(tp), _ptr(buf), _ptr(ranks)))
    return ranks[:nt]


class ItemSetSessions:
    """``ItemSet.on(store)``: the scan methods of ``Sessions`` under their names and keywords, restricted to the set.  The store
    must be current and of the set's model; its seen items are excluded as the store's own calls exclude them."""

    def __init__(self, item_set: ItemSet, store: "Sessions"):
        self.item_set, self.store = item_set, store

    def _src(self, slots, exclude, any_of, none_of, include_seen):
        return self.item_set._store(self.store, slots, exclude, any_of, none_of, include_seen)

    def recommend(self, slots, k: int, exclude=None, any_of=None, none_of=None, include_seen: bool = False):
        return self.item_set._recommend(self._src(slots, exclude, any_of, none_of, include_seen), k)

    def rank_targets(self, slots, targets, exclude=None, any_of=None, none_of=None, include_seen: bool = False) -> np.ndarray:
        """``Sessions.rank_targets`` within the set."""
        sl = Sessions._slots(slots)
        tp, ti = _items_csr(targets, sl.size)
        return self.item_set._rank_targets(self._src(sl, exclude, any_of, none_of, include_seen), tp, ti)

    def recommend_capped(self, slots, k: int, cap: int = 1, pool=None, exclude=None, any_of=None, none_of=None,
                         include_seen: bool = False, exact: bool = True):
        return self.item_set._capped(self._src(slots, exclude, any_of, none_of, include_seen), k, cap, pool, exact)

    def recommend_sampled(self, slots, k: int, temperature: float = 1.0, seed: int = 0, streams=None, exclude=None, any_of=None,
                          none_of=None, include_seen: bool = False, log_prob: bool = False):
        return self.item_set._sampled(self._src(slots, exclude, any_of, none_of, include_seen), k, temperature, seed, streams, log_prob)

    def log_partition(self, slots, temperature: float = 1.0, exclude=None, any_of=None, none_of=None,
                      include_seen: bool = False) -> Partition:
        return self.item_set._log_partition(self._src(slots, exclude, any_of, none_of, include_seen), temperature)

    def recommend_diverse(self, slots, k: int, pool: int, trade_off: float = 0.5, metric="cosine", exclude=None, any_of=None,
                          none_of=None):
        return self.item_set._diverse(self._src(slots, exclude, any_of, none_of, False), k, pool, trade_off, metric)

    def recommend_above(self, slots, threshold, exclude=None, any_of=None, none_of=None, include_seen: bool = False, max_results=None,
                        order: str = "score") -> Above:
        return self.item_set._above(self._src(slots, exclude, any_of, none_of, include_seen), threshold, max_results, order, False)

    def count_above(self, slots, threshold, exclude=None, any_of=None, none_of=None, include_seen: bool = False) -> np.ndarray:
        return self.item_set._above(self._src(slots, exclude, any_of, none_of, include_seen), threshold, None, "id", True)

    def recommend_top(self, slots, n, exclude=None, any_of=None, none_of=None, include_seen: bool = False, max_results=None,
                      order: str = "score") -> Above:
        return self.item_set._above(self._src(slots, exclude, any_of, none_of, include_seen), None, max_results, order, False, n)

    def nth_score(self, slots, n, exclude=None, any_of=None, none_of=None, include_seen: bool = False):
        return self.item_set._above(self._src(slots, exclude, any_of, none_of, include_seen), None, None, "id", True, n)

    def rollout(self, slots, steps: int, mode: str = "greedy", temperature: float = 1.0, seed: int = 0, streams=None, exclude=None,
                any_of=None, none_of=None, include_seen: bool = False, allow_repeats: bool = False, log_prob: bool = False,
                final_state: bool = False) -> Rollout:
        """``Sessions.rollout`` within the set (sbr_item_set_rollout): what the store's own call returns with every item outside
        the set added to each row's ``exclude``, bit for bit; ``frac_bits`` is the model's."""
        return self.store._rollout(self.item_set, slots, steps, mode, temperature, seed, streams, exclude, any_of, none_of, include_seen,
                                   allow_repeats, log_prob, final_state)

    def beam_search(self, slots, steps: int, width: int = 4, temperature: float = 1.0, exclude=None, any_of=None, none_of=None,
                    include_seen: bool = False, allow_repeats: bool = False, partitions: bool = False) -> Beams:
        """``Sessions.beam_search`` within the set (sbr_item_set_beam_search), under ``rollout``'s rule."""
        return self.store._beam_search(self.item_set, slots, steps, width, temperature, exclude, any_of, none_of, include_seen,
                                       allow_repeats, partitions)


def release_cached_memory() -> None:
    """Hand the engine's idle fit scratch (device and pinned-host blocks kept between fit calls) back to the driver."""
    _lib.load().sbr_release_cached_memory()
