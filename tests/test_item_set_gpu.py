"""GPU: item sets — every catalogue call restricted to a resident sub-table (sbr_item_set_*, ITEM SETS in include/sbr_hip.h).

The contract: a call through a set S returns, bit for bit, what the same call on the model returns with every item outside S added
to each row's exclusion list.  So every family is held three ways, all of them equality on ids, integers and f32 bits:

    numpy      the family's own statement (recommend_expect, filter_expect, sampled_expect, partition_expect, above_expect,
               top_expect, capped_expect, diverse_expect, seen_expect) over the oracle's scores with "outside S" joined to each row's
               excluded set
    exclusion  the model's own call with the complement of S appended to every exclusion list
    tags       the model's own call under a tag filter whose bit marks S

Shapes: test_sampled_gpu._core_case's — 1 000 items (32 tiles, the last ragged) x 130 rows (crosses the 128-row tile) — at d = 16
and d = 100 (stored as 128), SBR_CATALOGUE_GROUPS = 1 and 3, and |S| in {1, 31, 32, 33, every third item, all 1 000}: the 32-item
tile edge inside the set's own tiles.  Every third item of the table is one of three identical rows (i, i + 1, i + 2 for i = 0, 50,
100, ...), so tied scores fall inside and outside every S."""
import functools

import numpy as np
import pytest

from above_expect import above_expect
from capped_expect import capped_rows, ranking
from diverse_expect import DiverseExpectation
from filter_expect import allowed as tag_allowed
from filter_expect import equivalent_exclusions
from helpers import LOSS_HINGE, hparams
from partition_expect import frac_bits, partition_expect
from recommend_expect import NO_ITEM, topk_expectation
from sampled_expect import sampled_expect
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import NO_GROUP, Model
from sbr_rs_amd.errors import EngineError, PredictionError
from seen_expect import SeenModel
from test_sampled_gpu import _bits, _model, _oracle_of, _rep_scores
from top_expect import top_expect

pytestmark = pytest.mark.gpu

HOOK, FILL_HOOK, POISON_HOOK = "SBR_CATALOGUE_GROUPS", "SBR_ABOVE_FILL_BYTES", "SBR_TEST_POISON"
ITEMS, ROWS, T = 1000, 130, 8
S_BIT = np.uint32(1 << 31)  # the tag route's bit for "in S"; the case's own tags use bits 0 .. 3
DS, GROUPS = [16, 100], [1, 3]


def _force(monkeypatch, groups):
    monkeypatch.setenv(HOOK, str(groups))


@functools.lru_cache(maxsize=None)
def _case(d):
    """Parameters with planted ties, representation rows, caller lists, tags, groups and — computed once, read-only — the oracle's
    scores of every (row, item)."""
    rs = np.random.RandomState(100 + d)
    E = (rs.randn(ITEMS, d) * 0.3).astype(np.float32)
    b = (rs.randn(ITEMS) * 0.5).astype(np.float32)
    for i in range(0, ITEMS - 2, 50):
        E[i + 1] = E[i + 2] = E[i]
        b[i + 1] = b[i + 2] = b[i]
    reps = (rs.randn(ROWS, d) * 0.5).astype(np.float32)
    excl = [np.unique(rs.randint(0, ITEMS, rs.randint(0, 12))).astype(np.uint32) for _ in range(ROWS)]
    tags = rs.randint(0, 16, ITEMS).astype(np.uint32)
    groups = rs.randint(0, 8, ITEMS).astype(np.uint32)  # few groups: a pool of 16 under cap 1 leaves rows short
    groups[rs.rand(ITEMS) < 0.1] = NO_GROUP
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b)
    scores = _rep_scores(_oracle_of(g), ITEMS, reps)
    g.close()
    for a in (E, b, reps, tags, groups, scores):
        a.setflags(write=False)
    return E, b, reps, excl, tags, groups, scores


@functools.lru_cache(maxsize=None)
def _sets():
    """name -> sorted unique ids.  The small ones hold 50 and 52 and leave 51 out: a tie group that straddles the set."""
    perm = np.random.RandomState(5).permutation(ITEMS)
    perm = perm[~np.isin(perm, (50, 51, 52))]
    out = {"1": np.array([51])}
    for n in (31, 32, 33):
        out[str(n)] = np.sort(np.concatenate([[50, 52], perm[: n - 2]]))
    out["third"] = np.arange(0, ITEMS, 3)
    out["all"] = np.arange(ITEMS)
    return {k: v.astype(np.uint32) for k, v in out.items()}


SET_NAMES = ["1", "31", "32", "33", "third", "all"]


def _given(S):
    """the ids as a caller may give them: descending, with repeats"""
    return np.concatenate([S[::-1], S[:3]])


def _outside(S):
    return np.setdiff1d(np.arange(ITEMS, dtype=np.uint32), S).astype(np.uint32)


def _joined(excl, S, rows=ROWS):
    """each row's list with the complement of S appended"""
    out = _outside(S)
    return [np.concatenate([np.zeros(0, np.uint32) if excl is None else np.asarray(excl[u], np.uint32), out]).astype(np.uint32)
            for u in range(rows)]


def _tag_route(tags, S):
    t = tags.copy()
    t[S] |= S_BIT
    return t


def _topk_rows(scores, excl, k):
    rows = [topk_expectation(scores[u], excl[u], k) for u in range(len(scores))]
    return np.array([r[0] for r in rows], np.uint32).reshape(-1, k), np.array([r[1] for r in rows], np.float32).reshape(-1, k)


def _same_rows(got, want, what=""):
    """every array of a tuple result: integers equal, floats bit for bit"""
    assert len(got) == len(want), what
    for j, (a, w) in enumerate(zip(got, want)):
        a, w = np.asarray(a), np.asarray(w)
        assert a.shape == w.shape, (what, j, a.shape, w.shape)
        if a.dtype.kind == "f" and a.dtype.itemsize == 4:
            a, w = _bits(a), _bits(w)
        bad = np.argwhere(a != w)
        assert bad.size == 0, f"{what}: output {j}: {len(bad)} entries differ, first at {bad[0]}: {a[tuple(bad[0])]} vs {w[tuple(bad[0])]}"


def _same_above(got, want, what="", cuts=False):
    """an Above against (ptr, ids, scores[, cuts]) or another Above"""
    if not isinstance(want, tuple):
        want = (want.ptr, want.ids, want.scores) + ((want.cuts,) if cuts else ())
    _same_rows((got.ptr, got.ids, got.scores) + ((got.cuts,) if cuts else ()), want, what)


def _same_partition(got, want, what=""):
    if not isinstance(want, tuple):
        assert got.frac_bits == want.frac_bits, what
        want = (want.shift, want.mass)
    _same_rows((got.shift, got.mass), want, what)


def _thresholds(scores):
    """one bar per row between the rows' extremes, some ties at a score, a -inf and a +inf"""
    th = np.quantile(scores, 0.9, axis=1).astype(np.float32)
    th[::7] = scores[::7, 50]  # a score of the planted triple 50 / 51 / 52: ties at the bar, inside and outside the sets
    th[5], th[6] = -np.inf, np.inf
    return th


def _budgets(rows=ROWS):
    n = np.random.RandomState(3).randint(1, 40, rows).astype(np.uint64)
    n[0], n[1], n[2], n[3] = 0, 1, ITEMS + 5, 2000  # nothing, one, past the eligible items
    return n


# ------------------------------------------------------------------------------------------------
# the object
# ------------------------------------------------------------------------------------------------
def test_the_handle():
    E, b, reps, excl, tags, groups, scores = _case(16)
    g = _model(ITEMS, T, 16, ModelKind.EWMA, E, b)
    for name, S in _sets().items():
        s = g.item_set(_given(S))
        assert s.size == S.size == len(s) and np.array_equal(s.items, S) and s.items.dtype == np.uint32
        s.close()
        s.close()
    for bad in ([ITEMS], [0, 5, ITEMS + 7], [-1]):
        with pytest.raises(ValueError):
            g.item_set(bad)
    ids = np.array([3, ITEMS], np.uint32)  # the library's own check, under the Python layer's
    import ctypes as C

    h = C.c_void_p()
    assert g._L.sbr_item_set_create(g._h, ids.ctypes.data_as(C.c_void_p), 2, C.byref(h)) == Status.INVALID_ARGUMENT and not h.value
    s = g.item_set([4, 2])
    g.close()  # closes its live sets first
    assert s._h is None


# ------------------------------------------------------------------------------------------------
# top-k, with and without a filter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("d", DS)
def test_recommend(monkeypatch, d, groups):
    """k = 1, 10, 100 and 1 024 (past every |S| but one), every set; plain, with caller lists, and under a filter"""
    _force(monkeypatch, groups)
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    any_of = np.where(np.arange(ROWS) % 3 == 0, 0, 1 + np.arange(ROWS) % 7).astype(np.uint32)
    none_of = np.where(np.arange(ROWS) % 4 == 1, 8, 0).astype(np.uint32)
    for name in SET_NAMES:
        S = _sets()[name]
        s = g.item_set(_given(S))
        joined = _joined(excl, S)
        want = _topk_rows(scores, joined, 1024)
        for k in (1, 10, 100, 1024):
            got = s.recommend_reps(reps, k, exclude=excl)
            _same_rows(got, (want[0][:, :k], want[1][:, :k]), f"S={name} k={k}")
        _same_rows(s.recommend_reps(reps, 100, exclude=excl), g.recommend_reps(reps, 100, exclude=joined), f"S={name} exclusion route")
        _same_rows(s.recommend_reps(reps, 40), _topk_rows(scores, _joined(None, S), 40), f"S={name} no lists")
        # the filter: numpy, then both identities (the tag route needs the set's bit in the model's tags)
        fx = equivalent_exclusions(tags, any_of, none_of, ROWS, joined)
        got = s.recommend_reps(reps, 50, exclude=excl, any_of=any_of, none_of=none_of)
        _same_rows(got, _topk_rows(scores, fx, 50), f"S={name} filtered")
        _same_rows(got, g.recommend_reps(reps, 50, exclude=joined, any_of=any_of, none_of=none_of), f"S={name} filtered, exclusion route")
        g.set_item_tags(_tag_route(tags, S))
        _same_rows(s.recommend_reps(reps, 100, exclude=excl), g.recommend_reps(reps, 100, exclude=excl, any_of=int(S_BIT)), f"S={name} tag route")
        g.set_item_tags(tags)
        s.close()


def test_recommend_from_histories_and_wrappers():
    """the histories source (the history is the list; include_history), an LSTM's forward pass, and the model wrappers' item_set"""
    import sbr_rs_amd as sbr

    E, b, reps, excl, tags, grp, scores = _case(16)
    rs = np.random.RandomState(4)
    hists = [rs.randint(0, ITEMS, n).astype(np.uint32) for n in ([0, 1, 3, 8, 20] * 8)]
    ptr = np.zeros(len(hists) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(h) for h in hists])
    it = np.concatenate(hists).astype(np.uint32)
    for kind in (ModelKind.LSTM_NORMAL, ModelKind.EWMA):
        g = _model(ITEMS, T, 16, kind, E, b, tags)
        S = _sets()["third"]
        s = g.item_set(S)
        out = _outside(S)
        r = g.user_representations(ptr, it)
        for include in (False, True):
            lists = [np.concatenate([np.zeros(0, np.uint32) if include else h, out]) for h in hists]
            _same_rows(s.recommend(ptr, it, 30, include_history=include), g.recommend_reps(r, 30, exclude=lists), f"{kind.name} include={include}")
            _same_rows(s.recommend(ptr, it, 30, include_history=include, none_of=2),
                       g.recommend_reps(r, 30, exclude=lists, none_of=2), f"{kind.name} include={include} filtered")
        g.close()
    m = sbr.ewma.Hyperparameters.new(ITEMS, T).embedding_dim(16).build()
    w = m.item_set([5, 1, 9, 5])
    assert np.array_equal(w.items, [1, 5, 9])
    items, sc = w.recommend(hists, 5, exclude_history=False)
    assert items.shape == (len(hists), 5) and set(items[0].tolist()) == {1, 5, 9, int(NO_ITEM)}


# ------------------------------------------------------------------------------------------------
# sampled: the noise is the catalogue id's
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("d", DS)
def test_sampled(monkeypatch, d, groups):
    """two temperatures, explicit streams, with and without masks: the same (seed, stream) draws the same row through the set and
    through the plain call with the complement excluded — which fails if positions are hashed"""
    _force(monkeypatch, groups)
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    streams = (np.arange(ROWS, dtype=np.uint64) * 977 + 13) % 311  # repeats: two rows of one stream share their noise
    any_of = np.where(np.arange(ROWS) % 2 == 0, 0, 5).astype(np.uint32)
    for name in SET_NAMES:
        S = _sets()[name]
        s = g.item_set(S)
        joined = _joined(excl, S)
        for temp in (0.5, 4.0):
            want = sampled_expect(scores, joined, 100, temp, 77, streams)
            for k in (1, 10, 100):
                got = s.recommend_sampled_reps(reps, k, temperature=temp, seed=77, streams=streams, exclude=excl)
                _same_rows(got, tuple(w[:, :k] for w in want), f"S={name} T={temp} k={k}")
            _same_rows(s.recommend_sampled_reps(reps, 10, temperature=temp, seed=77, streams=streams, exclude=excl),
                       g.recommend_sampled_reps(reps, 10, temperature=temp, seed=77, streams=streams, exclude=joined), f"S={name} T={temp} exclusion route")
            fx = equivalent_exclusions(tags, any_of, 8, ROWS, joined)
            got = s.recommend_sampled_reps(reps, 10, temperature=temp, seed=78, streams=streams, exclude=excl, any_of=any_of, none_of=8)
            _same_rows(got, sampled_expect(scores, fx, 10, temp, 78, streams), f"S={name} T={temp} masks")
        # default streams (the row's index) and the propensities through the set's own partition
        got = s.recommend_sampled_reps(reps, 5, temperature=1.0, seed=3, exclude=excl, log_prob=True)
        ref = g.recommend_sampled_reps(reps, 5, temperature=1.0, seed=3, exclude=joined, log_prob=True)
        _same_rows(got[:3], ref[:3], f"S={name} default streams")
        assert np.array_equal(got[3], ref[3], equal_nan=True), f"S={name} log_prob"
        s.close()


# ------------------------------------------------------------------------------------------------
# log_partition: F is the model's
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("d", DS)
def test_log_partition(monkeypatch, d, groups):
    _force(monkeypatch, groups)
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    for name in SET_NAMES:
        S = _sets()[name]
        s = g.item_set(S)
        joined = _joined(excl, S)
        for temp in (0.5, 4.0):
            got = s.log_partition_reps(reps, temp, exclude=excl)
            assert got.frac_bits == frac_bits(ITEMS) == g.log_partition_reps(reps[:1], temp).frac_bits  # 40 here; the set's own |S| would give 40 too,
            _same_partition(got, partition_expect(scores, joined, temp), f"S={name} T={temp}")  # so the MASS is what holds F to the model's
            _same_partition(got, g.log_partition_reps(reps, temp, exclude=joined), f"S={name} T={temp} exclusion route")
            got = s.log_partition_reps(reps, temp, exclude=excl, any_of=6, none_of=1)
            _same_partition(got, partition_expect(scores, joined, temp, tags, 6, 1), f"S={name} T={temp} masks")
        s.close()


def test_log_partition_frac_bits_of_a_large_catalogue():
    """2^23 items: F = 63 - 24 = 39, where a set of 100 items on its own would take 40.  d = 16, one row; the mass through the set is
    the integer the contract states at the MODEL's F."""
    items = 1 << 23
    g = Model(hparams(items, 8, 16, int(ModelKind.EWMA), LOSS_HINGE, B=8))
    rep = (np.random.RandomState(1).randn(1, 16) * 0.5).astype(np.float32)
    S = np.arange(7, items, items // 100, dtype=np.uint32)[:100]
    s = g.item_set(S)
    got = s.log_partition_reps(rep, 1.0)
    assert got.frac_bits == 39 == frac_bits(items)
    sc = np.zeros((1, items), np.float32)
    sc[0, S] = g.predict(rep[0], S)
    from partition_expect import weights

    shift = np.float32((sc[0, S] * np.float32(1.0)).max())
    assert _bits(got.shift)[0] == _bits(shift) and int(got.mass[0]) == int(weights(sc[0, S], 1.0, shift, 39).sum(dtype=np.uint64))


# ------------------------------------------------------------------------------------------------
# above and top
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("d", DS)
def test_above_and_top(monkeypatch, d, groups):
    """both orders, SBR_ABOVE_FILL_BYTES forcing several fill ranges; budgets 0, 1 and past the eligible items"""
    _force(monkeypatch, groups)
    monkeypatch.setenv(FILL_HOOK, "4096")
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    th, n = _thresholds(scores), _budgets()
    for name in SET_NAMES:
        S = _sets()[name]
        s = g.item_set(S)
        joined = _joined(excl, S)
        allowed = np.array([tag_allowed(tags, 3, 4)] * ROWS)
        for order in ("score", "id"):
            got = s.recommend_above_reps(reps, th, exclude=excl, order=order)
            _same_above(got, above_expect(scores, th, joined, order=order), f"S={name} above {order}")
            got = s.recommend_top_reps(reps, n, exclude=excl, order=order)
            _same_above(got, top_expect(scores, n, joined, order=order), f"S={name} top {order}", cuts=True)
        _same_above(s.recommend_above_reps(reps, th, exclude=excl), g.recommend_above_reps(reps, th, exclude=joined), f"S={name} above, exclusion route")
        _same_above(s.recommend_top_reps(reps, n, exclude=excl), g.recommend_top_reps(reps, n, exclude=joined), f"S={name} top, exclusion route", cuts=True)
        _same_above(s.recommend_above_reps(reps, th, exclude=excl, any_of=3, none_of=4), above_expect(scores, th, joined, allowed), f"S={name} above masks")
        _same_above(s.recommend_top_reps(reps, n, exclude=excl, any_of=3, none_of=4), top_expect(scores, n, joined, allowed), f"S={name} top masks", cuts=True)
        assert np.array_equal(s.count_above_reps(reps, th, exclude=excl), g.count_above_reps(reps, th, exclude=joined))
        cuts, counts = s.nth_score_reps(reps, n, exclude=excl)
        want = top_expect(scores, n, joined)
        assert np.array_equal(_bits(cuts), _bits(want[3])) and np.array_equal(counts, np.diff(want[0]))
        with pytest.raises(ValueError, match="max_results"):
            s.recommend_above_reps(reps, -np.inf, max_results=S.size * ROWS - 1)
        s.close()


# ------------------------------------------------------------------------------------------------
# capped and diverse: the selections run on positions against the gathered words and the sub-table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("d", DS)
def test_capped(monkeypatch, d, groups):
    """groups straddle S; a small pool leaves rows short, which exact=True finishes with the set's own recommend_top"""
    _force(monkeypatch, groups)
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    g.set_item_groups(grp)
    k, cap, pool = 12, 1, 16
    for name in SET_NAMES:
        S = _sets()[name]
        s = g.item_set(S)
        joined = _joined(excl, S)
        ranks = [ranking(scores[u], joined[u]) for u in range(ROWS)]
        got = s.recommend_capped_reps(reps, k, cap=cap, pool=pool, exclude=excl, exact=False)
        want = capped_rows(ranks, grp, cap, k, pool)
        _same_rows(got, want, f"S={name} device rows")
        if name in ("third", "all"):
            assert not want[2].all()  # the pool of 16 leaves rows short
        _same_rows(s.recommend_capped_reps(reps, k, cap=cap, pool=pool, exclude=excl), capped_rows(ranks, grp, cap, k), f"S={name} exact")
        _same_rows(got, g.recommend_capped_reps(reps, k, cap=cap, pool=pool, exclude=joined, exact=False), f"S={name} exclusion route")
        ranks = [ranking(scores[u], joined[u], tag_allowed(tags, 0, 2)) for u in range(ROWS)]
        _same_rows(s.recommend_capped_reps(reps, k, cap=2, exclude=excl, none_of=2), capped_rows(ranks, grp, 2, k), f"S={name} masks, cap 2")
        s.close()


@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("d", DS)
def test_diverse(monkeypatch, d, groups):
    _force(monkeypatch, groups)
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    users = 24  # the numpy selection is slow
    for name in SET_NAMES:
        S = _sets()[name]
        s = g.item_set(S)
        joined = _joined(excl, S)
        pool_rows = _topk_rows(scores[:users], joined[:users], 40)
        for metric in ("cosine", "dot"):
            got = s.recommend_diverse_reps(reps[:users], 10, 40, trade_off=0.6, metric=metric, exclude=excl[:users])
            _same_rows(got, DiverseExpectation(E, metric).rows(pool_rows, 10, 0.6), f"S={name} {metric}")
        _same_rows(s.recommend_diverse_reps(reps, 10, 40, trade_off=0.3, exclude=excl),
                   g.recommend_diverse_reps(reps, 10, 40, trade_off=0.3, exclude=joined), f"S={name} exclusion route")
        _same_rows(s.recommend_diverse_reps(reps, 10, 40, trade_off=1.0, exclude=excl), s.recommend_reps(reps, 10, exclude=excl), f"S={name} trade_off=1")
        _same_rows(s.recommend_diverse_reps(reps, 10, 40, trade_off=0.3, exclude=excl, any_of=9),
                   g.recommend_diverse_reps(reps, 10, 40, trade_off=0.3, exclude=joined, any_of=9), f"S={name} masks")
        s.close()


# ------------------------------------------------------------------------------------------------
# sessions: the seen lists are built on the device and mapped to set positions there
# ------------------------------------------------------------------------------------------------
def _session_case(g, W, S):
    """slots 0 .. 7: seen items all inside S, all outside S, repeated, mixed, none, more than W (the ring wrapped); caller lists of
    0, 1, 63, 64, 65 and 150 entries mixing inside and outside ids; slot 6 has everything in S excluded"""
    rs = np.random.RandomState(W)
    inside, out = S, _outside(S)
    n = min(W, 8)
    appended = [rs.choice(inside, n), rs.choice(out, n) if out.size else rs.choice(inside, n), np.repeat(rs.choice(inside, 3), 3),
                rs.randint(0, ITEMS, n), np.zeros(0, np.int64), rs.randint(0, ITEMS, W + 5), rs.randint(0, ITEMS, 4), rs.randint(0, ITEMS, 2)]
    appended = [np.asarray(a, np.uint32) for a in appended]
    store = g.sessions(16, remember=W)
    seen = SeenModel(16, W)
    slots = np.arange(8, dtype=np.uint32)
    store.append(slots, appended)
    seen.append(slots, appended)
    lists = [rs.choice(ITEMS, n, replace=False).astype(np.uint32) for n in (0, 1, 63, 64, 65, 150)] + [S.copy(), rs.randint(0, ITEMS, 9).astype(np.uint32)]
    return store, seen, slots, lists


@pytest.mark.parametrize("W", [8, 100])
@pytest.mark.parametrize("name", ["33", "third"])
def test_sessions(monkeypatch, W, name):
    """W = 8 and W = 100: both forms of session_seen_lists_kernel ahead of subset_positions_kernel; every family through on(store)
    against numpy over the store's representations and against the store's own call with the complement excluded"""
    _force(monkeypatch, 3)
    monkeypatch.setenv(FILL_HOOK, "4096")
    d = 16
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    g.set_item_groups(grp)
    S = _sets()[name]
    s = g.item_set(S)
    store, seen, slots, lists = _session_case(g, W, S)
    on = s.on(store)
    sc = _rep_scores(_oracle_of(g), ITEMS, store.representations(slots))
    n = len(slots)
    out = _outside(S)
    for include_seen in (False, True):
        mine = [np.asarray(x, np.uint32) for x in lists] if include_seen else seen.excluded(slots, lists)
        joined = [np.concatenate([m, out]).astype(np.uint32) for m in mine]
        cl_joined = [np.concatenate([x, out]).astype(np.uint32) for x in lists]  # what the store's own call is given: it adds the seen items
        kw = dict(exclude=lists, include_seen=include_seen)
        ref = dict(exclude=cl_joined, include_seen=include_seen)
        what = f"W={W} S={name} include_seen={include_seen}"
        got = on.recommend(slots, 40, **kw)
        _same_rows(got, _topk_rows(sc, joined, 40), what)
        _same_rows(got, store.recommend(slots, 40, **ref), what + " exclusion route")
        assert np.all(got[0][6] == NO_ITEM)  # everything in S is excluded for slot 6
        if name == "33" and not include_seen:
            assert not np.isin(seen.seen([1])[0], S).any()  # slot 1's segment became all padding
        _same_rows(on.recommend(slots, 40, any_of=3, **kw), store.recommend(slots, 40, any_of=3, **ref), what + " filtered")
        streams = np.arange(n, dtype=np.uint64) + 1000
        got = on.recommend_sampled(slots, 10, temperature=0.7, seed=5, streams=streams, **kw)
        _same_rows(got, sampled_expect(sc, joined, 10, 0.7, 5, streams), what + " sampled")
        _same_rows(on.recommend_sampled(slots, 10, temperature=0.7, seed=5, **kw), store.recommend_sampled(slots, 10, temperature=0.7, seed=5, **ref),
                   what + " sampled, default streams are the slots")
        _same_partition(on.log_partition(slots, 0.7, **kw), partition_expect(sc, joined, 0.7), what + " partition")
        th = np.quantile(sc, 0.8, axis=1).astype(np.float32)
        for order in ("score", "id"):
            _same_above(on.recommend_above(slots, th, order=order, **kw), above_expect(sc, th, joined, order=order), what + f" above {order}")
        bud = np.array([0, 1, 5, 2000, 7, 33, 3, 9], np.uint64)
        _same_above(on.recommend_top(slots, bud, **kw), top_expect(sc, bud, joined), what + " top", cuts=True)
        assert np.array_equal(on.count_above(slots, th, **kw), store.count_above(slots, th, **ref))
        c0, c1 = on.nth_score(slots, bud, **kw), store.nth_score(slots, bud, **ref)
        assert np.array_equal(_bits(c0[0]), _bits(c1[0])) and np.array_equal(c0[1], c1[1])
        ranks = [ranking(sc[u], joined[u]) for u in range(n)]
        _same_rows(on.recommend_capped(slots, 6, cap=1, pool=8, **kw), capped_rows(ranks, grp, 1, 6), what + " capped, finished exactly")
        _same_rows(on.recommend_capped(slots, 6, cap=1, pool=8, exact=False, **kw), capped_rows(ranks, grp, 1, 6, 8), what + " capped, device rows")
    seen_joined = [np.concatenate([x, out]).astype(np.uint32) for x in lists]
    _same_rows(on.recommend_diverse(slots, 5, 20, trade_off=0.4, exclude=lists), store.recommend_diverse(slots, 5, 20, trade_off=0.4, exclude=seen_joined),
               f"W={W} S={name} diverse")
    plain = g.sessions(4)  # a store without memory: no seen lists, the caller's alone
    plain.append([0, 1], [[3, 6], [9]])
    _same_rows(s.on(plain).recommend([0, 1], 10, exclude=[[3], []]), plain.recommend([0, 1], 10, exclude=[np.concatenate([[3], out]), out]))
    with pytest.raises(ValueError):
        s.on(plain).recommend([0], 3, include_seen=True)


# ------------------------------------------------------------------------------------------------
# two launches
# ------------------------------------------------------------------------------------------------
def test_two_launches(monkeypatch):
    """8 192 + 40 rows x 300 items, d = 16, as test_recommend_among_two_launches: the sampled call's streams travel with the call's
    row index, the above call's CSR offsets run across the chunks"""
    items, d, nu = 300, 16, 8192 + 40
    rs = np.random.RandomState(8)
    E, b = (rs.randn(items, d) * 0.3).astype(np.float32), (rs.randn(items) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, b)
    base = (rs.randn(40, d) * 0.5).astype(np.float32)
    who = rs.randint(0, 40, nu)
    who[-40:] = np.arange(40)
    reps = base[who]
    S = np.sort(rs.choice(items, 100, replace=False)).astype(np.uint32)
    out = np.setdiff1d(np.arange(items), S).astype(np.uint32)
    s = g.item_set(S)
    sc = _rep_scores(_oracle_of(g), items, base)
    streams = np.arange(nu, dtype=np.uint64)[::-1].copy()
    got = s.recommend_sampled_reps(reps, 5, temperature=1.0, seed=11, streams=streams)
    want = sampled_expect(sc[who[-60:]], [out] * 60, 5, 1.0, 11, streams[-60:])  # the second launch's rows and the first's last
    _same_rows(tuple(x[-60:] for x in got), want, "sampled, the rows around the chunk edge")
    first = sampled_expect(sc[who[:20]], [out] * 20, 5, 1.0, 11, streams[:20])
    _same_rows(tuple(x[:20] for x in got), first, "sampled, the first rows")
    th = np.quantile(sc, 0.7, axis=1).astype(np.float32)[who]
    ab = s.recommend_above_reps(reps, th, order="id")
    w_ptr, w_ids, w_sc = above_expect(sc, np.quantile(sc, 0.7, axis=1).astype(np.float32), [out] * 40, order="id")
    rows = [(w_ids[int(w_ptr[u]): int(w_ptr[u + 1])], w_sc[int(w_ptr[u]): int(w_ptr[u + 1])]) for u in range(40)]
    assert np.array_equal(ab.counts, np.array([rows[w][0].size for w in who], np.uint64))
    for r in list(range(0, nu, 997)) + list(range(nu - 45, nu)):
        ids, scs = ab.row(r)
        assert np.array_equal(ids, rows[who[r]][0]) and np.array_equal(_bits(scs), _bits(rows[who[r]][1])), r


# ------------------------------------------------------------------------------------------------
# lifecycle
# ------------------------------------------------------------------------------------------------
def _every_call(s, reps):
    return [lambda: s.recommend_reps(reps, 3), lambda: s.recommend_sampled_reps(reps, 3), lambda: s.log_partition_reps(reps),
            lambda: s.recommend_above_reps(reps, 0.0), lambda: s.count_above_reps(reps, 0.0), lambda: s.recommend_top_reps(reps, 3),
            lambda: s.nth_score_reps(reps, 3), lambda: s.recommend_capped_reps(reps, 3), lambda: s.recommend_diverse_reps(reps, 3, 6)]


def test_staleness_and_refresh():
    """set_param makes the set stale and every call is refused; refresh() gives the new expectation; an open fit plan is refused"""
    d = 16
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    g.set_item_groups(grp)
    S = _sets()["33"]
    s = g.item_set(S)
    r = reps[:9]
    before = s.recommend_reps(r, 5)
    b2 = b.copy()
    b2[S[:5]] += 3.0
    g.set_param(Param.ITEM_BIAS, b2)
    for call in _every_call(s, r):
        with pytest.raises(ValueError) as e:
            call()
        assert isinstance(e.value, EngineError)
    store = g.sessions(4, remember=4)
    with pytest.raises(ValueError):
        s.on(store).recommend([0], 3)
    s.refresh()
    after = s.recommend_reps(r, 5)
    _same_rows(after, g.recommend_reps(r, 5, exclude=_joined(None, S, 9)), "after refresh")
    assert not np.array_equal(after[0], before[0])
    ptr, it = np.array([0, 3, 5], np.uint64), np.array([1, 2, 3, 4, 5], np.uint32)
    plan = g.fit_begin(ptr, it)
    for call in _every_call(s, r):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        s.refresh()
    with pytest.raises(ValueError):
        g.item_set([1, 2])
    plan.close()
    with pytest.raises(ValueError):  # the plan changed the generation
        s.recommend_reps(r, 5)
    s.refresh()
    s.recommend_reps(r, 5)


def test_tags_and_groups_need_no_refresh():
    d = 16
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    g.set_item_groups(grp)
    S = _sets()["third"]
    s = g.item_set(S)
    joined = _joined(None, S)
    tags2 = np.roll(tags, 17)
    grp2 = np.roll(grp, 29)
    _same_rows(s.recommend_reps(reps, 20, any_of=5), _topk_rows(scores, equivalent_exclusions(tags, 5, 0, ROWS, joined), 20), "the first tags")
    g.set_item_tags(tags2)
    _same_rows(s.recommend_reps(reps, 20, any_of=5), _topk_rows(scores, equivalent_exclusions(tags2, 5, 0, ROWS, joined), 20), "the new tags")
    ranks = [ranking(scores[u], joined[u]) for u in range(ROWS)]
    _same_rows(s.recommend_capped_reps(reps, 8, cap=1, exact=False), capped_rows(ranks, grp, 1, 8, 64), "the first groups")
    g.set_item_groups(grp2)
    _same_rows(s.recommend_capped_reps(reps, 8, cap=1, exact=False), capped_rows(ranks, grp2, 1, 8, 64), "the new groups")
    g.set_item_tags(None)
    with pytest.raises(ValueError):
        s.recommend_reps(reps, 5, any_of=1)
    g.set_item_groups(None)
    with pytest.raises(ValueError):
        s.recommend_capped_reps(reps, 5)


def test_refusals_non_finite_rows_and_the_empty_set():
    d = 16
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    g.set_item_groups(grp)
    other = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    S = _sets()["33"]
    s = g.item_set(S)
    with pytest.raises(ValueError):  # a store of another model
        s.on(other.sessions(4)).recommend([0], 3)
    # a non-finite row outside S is never read; inside S it fails the call, and the flag is clear for the next one
    E2 = E.copy()
    E2[51, 0] = np.nan
    g.set_param(Param.ITEM_EMBEDDING, E2)
    s.refresh()
    r = reps[:9]
    _same_rows(s.recommend_reps(r, 5), _topk_rows(scores[:9], _joined(None, S, 9), 5), "NaN outside S")
    with pytest.raises(PredictionError):
        g.recommend_reps(r, 5)
    E2 = E.copy()
    E2[50, 0] = np.nan
    g.set_param(Param.ITEM_EMBEDDING, E2)
    s.refresh()
    for call in _every_call(s, r)[:7]:
        with pytest.raises(PredictionError):
            call()
    g.set_param(Param.ITEM_EMBEDDING, E)
    s.refresh()
    _same_rows(s.recommend_reps(r, 5), _topk_rows(scores[:9], _joined(None, S, 9), 5), "the flag is clear again")
    # the empty set: every call answers as the plain call does for a row that may see nothing
    e = g.item_set([])
    assert e.size == 0 and e.items.size == 0
    everything = [np.arange(ITEMS, dtype=np.uint32)] * 9
    _same_rows(e.recommend_reps(r, 4), g.recommend_reps(r, 4, exclude=everything), "empty recommend")
    _same_rows(e.recommend_sampled_reps(r, 4), g.recommend_sampled_reps(r, 4, exclude=everything), "empty sampled")
    _same_partition(e.log_partition_reps(r), g.log_partition_reps(r, exclude=everything), "empty partition")
    _same_above(e.recommend_above_reps(r, -np.inf), g.recommend_above_reps(r, -np.inf, exclude=everything), "empty above")
    bud = np.array([0, 1, 2, 3, 0, 9, 1, 1, 5], np.uint64)
    _same_above(e.recommend_top_reps(r, bud), g.recommend_top_reps(r, bud, exclude=everything), "empty top", cuts=True)
    _same_rows(e.recommend_capped_reps(r, 4), g.recommend_capped_reps(r, 4, exclude=everything), "empty capped")
    _same_rows(e.recommend_diverse_reps(r, 4, 8), g.recommend_diverse_reps(r, 4, 8, exclude=everything), "empty diverse")
    store = g.sessions(4, remember=4)
    store.append([0], [[1, 2]])
    _same_rows(e.on(store).recommend([0, 1], 3), store.recommend([0, 1], 3, exclude=everything[:2]), "empty, a store")
    e.refresh()


# ------------------------------------------------------------------------------------------------
# poisoned scratch: one reduced pass of every family
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0xFF, 0x7F, 0x80], ids=lambda p: f"poison{p:02X}")
def test_on_poisoned_scratch(monkeypatch, pattern):
    """SBR_TEST_POISON as tests/test_poisoned_scratch_gpu.py sets it (that module's fixture proves the hook is live): every arena
    carve and cached block is filled with the byte first.  The set is created under the hook too — its sub-table is persistent
    memory the gather writes in full — and every family is held to numpy."""
    monkeypatch.setenv(POISON_HOOK, str(pattern))
    _force(monkeypatch, 3)
    monkeypatch.setenv(FILL_HOOK, "4096")
    d = 100
    E, b, reps, excl, tags, grp, scores = _case(d)
    g = _model(ITEMS, T, d, ModelKind.EWMA, E, b, tags)
    g.set_item_groups(grp)
    S = _sets()["third"]
    s = g.item_set(_given(S))
    joined = _joined(excl, S)
    fx = equivalent_exclusions(tags, 3, 4, ROWS, joined)
    allowed = np.array([tag_allowed(tags, 3, 4)] * ROWS)
    th, n = _thresholds(scores), _budgets()
    for _ in range(2):  # the second pass meets what the first left in the arena
        _same_rows(s.recommend_reps(reps, 20, exclude=excl, any_of=3, none_of=4), _topk_rows(scores, fx, 20), "recommend")
        _same_rows(s.recommend_sampled_reps(reps, 10, temperature=0.5, seed=9, exclude=excl, any_of=3, none_of=4), sampled_expect(scores, fx, 10, 0.5, 9), "sampled")
        _same_partition(s.log_partition_reps(reps, 0.5, exclude=excl, any_of=3, none_of=4), partition_expect(scores, joined, 0.5, tags, 3, 4), "partition")
        _same_above(s.recommend_above_reps(reps, th, exclude=excl, any_of=3, none_of=4), above_expect(scores, th, joined, allowed), "above")
        _same_above(s.recommend_top_reps(reps, n, exclude=excl, any_of=3, none_of=4), top_expect(scores, n, joined, allowed), "top", cuts=True)
        ranks = [ranking(scores[u], joined[u], allowed[u]) for u in range(ROWS)]
        _same_rows(s.recommend_capped_reps(reps, 8, cap=1, pool=12, exclude=excl, any_of=3, none_of=4, exact=False), capped_rows(ranks, grp, 1, 8, 12), "capped")
        _same_rows(s.recommend_diverse_reps(reps[:12], 6, 20, trade_off=0.5, exclude=excl[:12]),
                   DiverseExpectation(E, "cosine").rows(_topk_rows(scores[:12], joined[:12], 20), 6, 0.5), "diverse")
    store, seen, slots, lists = _session_case(g, 8, S)
    sc = _rep_scores(_oracle_of(g), ITEMS, store.representations(slots))
    out = _outside(S)
    sj = [np.concatenate([m, out]).astype(np.uint32) for m in seen.excluded(slots, lists)]
    _same_rows(s.on(store).recommend(slots, 20, exclude=lists), _topk_rows(sc, sj, 20), "a store")
