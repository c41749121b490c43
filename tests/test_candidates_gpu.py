"""GPU: sbr_recommend_among[_reps], sbr_score_candidates[_reps] and sbr_user_representations (sbr_catalogue.hip) against the
oracle's user_representation and predict (candidates_expect.py) and against the engine's own single-user calls.  Every comparison
is equality of item ids and of score bits."""
import ctypes as C

import numpy as np
import pytest

from candidates_expect import AmongExpectation, oracle_candidate_scores, planted_params, planted_subset
from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM, topk_expectation
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, PredictionError

pytestmark = pytest.mark.gpu

KINDS = [ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA]
PAIRS_PER_LAUNCH = 1 << 22  # candidate_pairs_cap (sbr_kernels.h)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    gi, gs = got
    wi, ws = want
    assert gi.shape == wi.shape, (gi.shape, wi.shape)
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{len(bad)} items differ; first at {bad[0]}: {gi[tuple(bad[0])]} vs {wi[tuple(bad[0])]}"
    assert np.array_equal(_bits(gs), _bits(ws))


def _same_lists(got, want):
    assert len(got) == len(want)
    for u, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"user {u}"


def _pair(items, T, d, kind, E=None, bias=None, oracle=True):
    hp = hparams(items, T, d, int(kind), LOSS_HINGE, B=8)
    g, o = Model(hp), OracleModel(hp) if oracle else None
    for m in (g, o):
        if m is None:
            continue
        if E is not None:
            m.set_param(Param.ITEM_EMBEDDING, E)
        if bias is not None:
            m.set_param(Param.ITEM_BIAS, bias)
    return g, o


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, np.uint32) for x in lists]) if len(lists) else np.zeros(0, np.uint32)
    return ptr, flat.astype(np.uint32)


_SHAPES = [(1, 300), (16, 1500), (64, 900), (100, 2000), (128, 700), (256, 3000)]


# ---- 1. recommend_among against the expectation -------------------------------------------------------------------------------
@pytest.mark.parametrize("d,items", _SHAPES)
def test_recommend_among_matches_expectation(d, items):
    T, nu = 12, 24
    kind = KINDS[(d + items) % 3]
    E, bias, tied = planted_params(items, d, d + items)
    g, o = _pair(items, T, d, kind, E, bias)
    ptr, it = synthetic_interactions(nu, items, 3 * T, seed=d, min_len=0, zipf=True)
    want = AmongExpectation.from_histories(o, items, ptr, it)
    reps = np.array([o.user_representation(h) for h in want.hists], np.float32)
    rs = np.random.RandomState(d)
    for n in (1, 31, 32, 33, items // 3, items):
        S = planted_subset(items, n, tied, n)
        if 2 < n < items:  # ties inside the set, tied items outside it, and a tied item below the set's lowest one
            assert np.intersect1d(S, tied).size >= 2 and np.setdiff1d(tied, S).size >= 1
        for k in sorted({1, 10, min(1024, n), min(1024, n + 3)}):
            _same(g.recommend_among(ptr, it, k, S), want.rows(S, k, exclude=want.hists))
            _same(g.recommend_among(ptr, it, k, S, include_history=True), want.rows(S, k))
            _same(g.recommend_among_reps(reps, k, S), want.rows(S, k))
            if k - 1 <= n:  # caller's lists (unsorted, duplicates, ids outside S too) that leave k - 1 eligible items of S
                excl = []
                for _ in range(nu):
                    keep = rs.choice(S, k - 1, replace=False)
                    ex = np.concatenate([np.setdiff1d(S, keep), np.setdiff1d(rs.randint(0, items, 5), keep)])
                    ex = np.concatenate([ex, ex[:7]])
                    rs.shuffle(ex)
                    excl.append(ex.astype(np.uint32))
                xi, xs = g.recommend_among_reps(reps, k, S, exclude=excl)
                _same((xi, xs), want.rows(S, k, exclude=excl))
                assert np.all(xi[:, k - 1] == NO_ITEM) and np.all(xi[:, : k - 1] != NO_ITEM)
    # the planted ties resolve to the lower id AMONG S (item 0, the lowest of the catalogue's tied items, is outside it): every
    # row — the whole set fits one — holds the set's tied items in ascending order
    S = planted_subset(items, items // 3, tied, 5)
    inside = np.intersect1d(S, tied)
    gi, gs = g.recommend_among_reps(reps, S.size, S)
    for row, sc in zip(gi.tolist(), gs):
        pos = [row.index(int(t)) for t in inside]
        assert pos == sorted(pos) and np.unique(_bits(sc[pos])).size == 1


# ---- 2. identities without the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,items", [(16, 1500), (100, 2000), (256, 3000)])
def test_recommend_among_identities(d, items):
    T, nu = 12, 40
    E, bias, tied = planted_params(items, d, d)
    g, _ = _pair(items, T, d, KINDS[d % 3], E, bias, oracle=False)
    ptr, it = synthetic_interactions(nu, items, 3 * T, seed=d + 1, min_len=0, zipf=True)
    everything = np.arange(items, dtype=np.uint32)
    for k in (1, 100, min(1024, items)):
        for inc in (False, True):
            _same(g.recommend_among(ptr, it, k, everything, include_history=inc), g.recommend(ptr, it, k, include_history=inc))
    reps = g.user_representations(ptr, it)
    rs = np.random.RandomState(d)
    S = planted_subset(items, items // 3, tied, 3)
    outside = np.setdiff1d(everything, S).astype(np.uint32)
    excl = [rs.randint(0, items, 30).astype(np.uint32) for _ in range(nu)]
    for k in (10, min(1024, S.size)):
        _same(g.recommend_among_reps(reps, k, S), g.recommend_reps(reps, k, exclude=[outside] * nu))
        _same(g.recommend_among_reps(reps, k, S, exclude=excl), g.recommend_reps(reps, k, exclude=[np.concatenate([outside, e]) for e in excl]))
        messy = np.concatenate([S, S[:50], S[-3:]])
        rs.shuffle(messy)
        _same(g.recommend_among_reps(reps, k, messy, exclude=excl), g.recommend_among_reps(reps, k, np.unique(S), exclude=excl))
        _same(g.recommend_among(ptr, it, k, messy), g.recommend_among(ptr, it, k, np.unique(S)))


# ---- 3. non-finite locality ---------------------------------------------------------------------------------------------------
def test_recommend_among_scores_only_the_subset():
    items, d, k, bad = 500, 32, 10, 123
    E, bias, tied = planted_params(items, d, 3)
    E[bad] = 3e19
    g, _ = _pair(items, 8, d, ModelKind.EWMA, E, bias, oracle=False)
    clean = E.copy()
    clean[bad] = 0.0
    c, _ = _pair(items, 8, d, ModelKind.EWMA, clean, bias, oracle=False)
    reps = np.full((6, d), 1e19, np.float32)  # 3e19 * 1e19 overflows within two steps of the chain; 0.3 * 1e19 is far from it
    reps[3] = -1e19
    everything = np.arange(items, dtype=np.uint32)
    S = np.setdiff1d(everything, [bad]).astype(np.uint32)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_reps(reps, k)
    _same(g.recommend_among_reps(reps, k, S), c.recommend_among_reps(reps, k, S))  # the row outside S is never read
    _same(g.recommend_among_reps(reps, k, S[::3]), c.recommend_reps(reps, k, exclude=[np.setdiff1d(everything, S[::3])] * 6))
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_among_reps(reps, k, everything)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_among_reps(reps, k, [bad])
    # ... and the flag does not outlive the call
    _same(g.recommend_among_reps(reps, k, S), c.recommend_among_reps(reps, k, S))
    # from histories: an EWMA state that holds the huge row itself
    hists = [[4, 9, bad], [bad], [7, bad, bad]]
    ptr, it = _csr(hists)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend(ptr, it, k)
    gi, gs = g.recommend_among(ptr, it, k, S)
    assert np.all(np.isfinite(gs)) and bad not in gi and np.all(gi != NO_ITEM)
    _same((gi, gs), g.recommend_among_reps(g.user_representations(ptr, it), k, S, exclude=hists))
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_among(ptr, it, k, everything)


# ---- 4. several item ranges and full lists --------------------------------------------------------------------------------------
_MONOTONE = {}


def _monotone_case(direction):
    """The 60 000-item monotone table of test_similar_items_long_ranges_full_lists (d = 32, E[i] = (1e-3 * (i + 1), 0, ...), or the
    ramp reversed), a zero bias, 160 users whose representations are rows of the table: the score of item i is E[q][0] * E[i][0],
    strictly monotone in the id, so under the ascending ramp every scanned score is a candidate.  Scores computed once."""
    if direction not in _MONOTONE:
        items, d = 60_000, 32
        E = np.zeros((items, d), np.float32)
        ramp = np.arange(1, items + 1, dtype=np.float64) * 1e-3
        E[:, 0] = (ramp if direction > 0 else ramp[::-1]).astype(np.float32)
        bias = np.zeros(items, np.float32)
        o = OracleModel(hparams(items, 8, d, int(ModelKind.EWMA), LOSS_HINGE))
        o.set_param(Param.ITEM_EMBEDDING, E)
        o.set_param(Param.ITEM_BIAS, bias)
        reps = E[np.random.RandomState(6).randint(0, items, 160)]
        S = np.arange(0, items, 3, dtype=np.uint32)
        _MONOTONE[direction] = (E, bias, reps, S, AmongExpectation(o, items, reps).rows(S, 1024))
    return _MONOTONE[direction]


@pytest.mark.parametrize("groups", ["1", "3"])
@pytest.mark.parametrize("direction", [1, -1])
def test_recommend_among_long_ranges_full_lists(direction, groups, monkeypatch):
    """One long item range and three (SBR_CATALOGUE_GROUPS) over S = every third item, k = 1024: full lists, staging merges, the
    merge of ranges — all sized from |S|."""
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", groups)
    E, bias, reps, S, want = _monotone_case(direction)
    g, _ = _pair(E.shape[0], 8, E.shape[1], ModelKind.EWMA, E, bias, oracle=False)
    got = g.recommend_among_reps(reps, 1024, S)
    _same(got, want)
    top = S[::-1][:1024] if direction > 0 else S[:1024]
    for j in (0, 77, 159):
        assert got[0][j].tolist() == top.tolist()


# ---- 5. two launches ------------------------------------------------------------------------------------------------------------
def test_recommend_among_two_launches():
    """8 192 + 40 users: the second launch's rows (c0 != 0) land where they belong."""
    items, d, k, nu = 300, 16, 10, 8192 + 40
    E, bias, tied = planted_params(items, d, 8)
    g, o = _pair(items, 8, d, ModelKind.LSTM_NORMAL, E, bias)
    S = planted_subset(items, 100, tied, 2)
    rs = np.random.RandomState(9)
    pool = [rs.randint(0, items, n) for n in (0, 1, 5, 8, 13) * 8]  # 40 histories
    who = rs.randint(0, len(pool), nu)
    who[-40:] = np.arange(40)
    ptr, it = _csr([pool[w] for w in who])
    pptr, pit = _csr(pool)
    want = AmongExpectation.from_histories(o, items, pptr, pit).rows(S, k, exclude=pool)
    got = g.recommend_among(ptr, it, k, S)
    _same(got, (want[0][who], want[1][who]))
    _same(g.recommend_among_reps(g.user_representations(ptr, it), k, S, exclude=[pool[w] for w in who]), got)


# ---- 6. score_candidates against the oracle and predict -------------------------------------------------------------------------
def _candidate_lists(items, nu, seed):
    """list lengths 0, 1, 63, 64, 65 (the wave edge), 1 000 and random ones; unsorted, with duplicates"""
    rs = np.random.RandomState(seed)
    lens = [0, 1, 63, 64, 65, 1000, 0, 127, 129] + rs.randint(0, 200, nu - 9).tolist()
    return [rs.randint(0, items, n).astype(np.uint32) for n in lens]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 16, 32, 64, 100, 128, 256])
def test_score_candidates_matches_oracle_and_predict(kind, d):
    items, T, nu = 700, 12, 40
    E, bias, _ = planted_params(items, d, d)
    g, o = _pair(items, T, d, kind, E, bias)
    ptr, it = synthetic_interactions(nu, items, 3 * T, seed=d, min_len=0, zipf=True)
    hists = [it[int(ptr[u]): int(ptr[u + 1])] for u in range(nu)]
    cands = _candidate_lists(items, nu, d)
    assert any(np.unique(c).size < c.size for c in cands)
    cp, ci = _csr(cands)
    got = g.score_candidates(ptr, it, cp, ci)
    _same_lists(got, oracle_candidate_scores(o, hists, cands))
    _same_lists(got, [g.predict(g.user_representation(h), c) if len(c) else np.zeros(0, np.float32) for h, c in zip(hists, cands)])
    reps = g.user_representations(ptr, it)
    _same_lists(g.score_candidates_reps(reps, cp, ci), got)
    # pointers that do not start at zero: the scores of the lists they cover, from out_scores[0] on
    _same_lists(g.score_candidates_reps(reps[5:], cp[5:], ci), got[5:])


def test_score_candidates_wrappers_and_rerank():
    import sbr_rs_amd as sbr

    items, d, T, nu = 400, 24, 8, 12
    E, bias, _ = planted_params(items, d, 4)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    w = sbr.ewma.ImplicitEWMAModel(g)
    rs = np.random.RandomState(1)
    hists = [rs.randint(0, items, n) for n in rs.randint(0, 15, nu)]
    cands = _candidate_lists(items, nu, 2)
    want = oracle_candidate_scores(o, hists, cands)
    _same_lists(w.score_candidates(hists, cands), want)
    assert np.array_equal(_bits(w.user_representations(hists)), _bits(np.array([o.user_representation(np.asarray(h, np.uint32)) for h in hists])))
    for k in (None, 5):
        for (ri, rsc), c, s in zip(w.rerank(hists, cands, k), cands, want):
            full = np.full(items, -np.inf, np.float32)
            full[c] = s  # duplicates carry the same score
            n = np.unique(c).size if k is None else min(k, np.unique(c).size)
            ei, es = topk_expectation(full, np.setdiff1d(np.arange(items), c), n)
            assert np.array_equal(ri, ei) and np.array_equal(_bits(rsc), _bits(es))
    S = planted_subset(items, 90, np.arange(0, 42, 2, dtype=np.uint32), 1)
    ptr, it = _csr(hists)
    _same(w.recommend(hists, 7, among=S), g.recommend_among(ptr, it, 7, S))
    _same(w.recommend(hists, 7, exclude_history=False, among=S), g.recommend_among(ptr, it, 7, S, include_history=True))
    _same(w.recommend(hists, 7), g.recommend(ptr, it, 7))


# ---- 7. pair-cap crossing -----------------------------------------------------------------------------------------------------
def _integer_model(items, d, seed):
    """E, b and representations with integer entries in -2 .. 2: every product and partial sum is exact, so a float32 loop over k
    is the chain's result whatever the order — these tests are about the carving of the pair list, not the chain."""
    rs = np.random.RandomState(seed)
    E = rs.randint(-2, 3, (items, d)).astype(np.float32)
    bias = rs.randint(-2, 3, items).astype(np.float32)
    g, _ = _pair(items, 8, d, ModelKind.EWMA, E, bias, oracle=False)
    return g, E, bias, rs


def _integer_scores(E, bias, reps, cp, ci):
    user = np.repeat(np.arange(len(cp) - 1), np.diff(cp.astype(np.int64)))
    acc = np.zeros(ci.size, np.float32)
    for k in range(E.shape[1]):
        acc = acc + reps[user, k] * E[ci, k]
    return bias[ci] + acc


def test_score_candidates_crosses_the_pair_cap():
    items, d = 300, 16
    g, E, bias, rs = _integer_model(items, d, 12)
    lens = [2_000_000, 2_194_000, 600, 0, 2_704]  # the third user's list straddles the cap; cap + 3 000 pairs in all
    assert sum(lens) == PAIRS_PER_LAUNCH + 3000 and sum(lens[:2]) < PAIRS_PER_LAUNCH < sum(lens[:3])
    reps = rs.randint(-2, 3, (len(lens), d)).astype(np.float32)
    cp = np.zeros(len(lens) + 1, np.uint64)
    cp[1:] = np.cumsum(lens)
    ci = rs.randint(0, items, sum(lens)).astype(np.uint32)
    got = np.concatenate(g.score_candidates_reps(reps, cp, ci))
    assert np.array_equal(_bits(got), _bits(_integer_scores(E, bias, reps, cp, ci)))


def test_score_candidates_two_user_chunks():
    items, d, nu = 300, 16, 8192 + 40
    g, E, bias, rs = _integer_model(items, d, 13)
    reps = rs.randint(-2, 3, (nu, d)).astype(np.float32)
    cp = np.arange(0, 3 * nu + 1, 3, dtype=np.uint64)
    ci = rs.randint(0, items, 3 * nu).astype(np.uint32)
    got = np.concatenate(g.score_candidates_reps(reps, cp, ci))
    assert np.array_equal(_bits(got), _bits(_integer_scores(E, bias, reps, cp, ci)))


# ---- 8. user_representations ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [16, 100, 256])
def test_user_representations_match_single_calls(kind, d):
    items, T = 300, 8
    g, _ = _pair(items, T, d, kind, oracle=False)
    rs = np.random.RandomState(d)
    hists = [rs.randint(0, items, n).astype(np.uint32) for n in (0, 1, T, T + 5, 3, 0, T + 5, 1, T - 1, 2 * T)]
    ptr, it = _csr(hists)
    got = g.user_representations(ptr, it)
    assert got.shape == (len(hists), d)
    assert np.array_equal(_bits(got), _bits(np.array([g.user_representation(h) for h in hists])))
    assert np.array_equal(_bits(got[0]), _bits(g.user_representation(np.zeros(1, np.uint32))))  # empty = item 0
    assert g.user_representations(np.zeros(1, np.uint64), np.zeros(0, np.uint32)).shape == (0, d)  # no users: a no-op


def test_user_representations_two_launches():
    items, T, d, nu = 300, 8, 16, 8192 + 40
    g, _ = _pair(items, T, d, ModelKind.LSTM_NORMAL, oracle=False)
    rs = np.random.RandomState(3)
    pool = [rs.randint(0, items, n).astype(np.uint32) for n in (0, 1, T, T + 5, 4) * 8]
    single = np.array([g.user_representation(h) for h in pool])
    who = rs.randint(0, len(pool), nu)
    who[-40:] = np.arange(40)
    ptr, it = _csr([pool[w] for w in who])
    assert np.array_equal(_bits(g.user_representations(ptr, it)), _bits(single[who]))


# ---- 9. errors --------------------------------------------------------------------------------------------------------------------
def test_candidates_errors():
    items, d, k, nu = 500, 32, 10, 6
    E, bias, tied = planted_params(items, d, 3)
    g, _ = _pair(items, 8, d, ModelKind.LSTM_NORMAL, E, bias, oracle=False)
    ptr, it = synthetic_interactions(nu, items, 12, seed=1, min_len=1)
    reps = g.user_representations(ptr, it)
    S = np.arange(0, items, 2, dtype=np.uint32)
    cands = [np.arange(5, dtype=np.uint32)] * nu
    cp, ci = _csr(cands)
    bad_ptr = cp.copy()
    bad_ptr[2] = bad_ptr[3] + 1
    bad_it = it.copy()
    bad_it[3] = items
    bad_ci = ci.copy()
    bad_ci[7] = items
    calls = [
        lambda: g.recommend_among(ptr, it, k, [3, items]), lambda: g.recommend_among_reps(reps, k, [items]),
        lambda: g.recommend_among(ptr, it, 0, S), lambda: g.recommend_among(ptr, it, 1025, S), lambda: g.recommend_among_reps(reps, 0, S),
        lambda: g.recommend_among(ptr, bad_it, k, S), lambda: g.recommend_among_reps(reps, k, S, exclude=[[items]] + [[]] * (nu - 1)),
        lambda: g.score_candidates(ptr, it, bad_ptr, ci), lambda: g.score_candidates_reps(reps, bad_ptr, ci),
        lambda: g.score_candidates(ptr, it, cp, bad_ci), lambda: g.score_candidates_reps(reps, cp, bad_ci),
        lambda: g.score_candidates(ptr, bad_it, cp, ci), lambda: g.user_representations(ptr, bad_it),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT, i
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    L, h = g._L, g._h
    out_i = np.zeros((nu, k), np.uint32)
    out_s = np.zeros(ci.size, np.float32)
    assert L.sbr_recommend_among(h, vp(ptr), vp(it), nu, k, 2, vp(S), S.size, vp(out_i), None) == Status.INVALID_ARGUMENT  # unknown flag
    assert L.sbr_recommend_among(h, vp(ptr), vp(it), nu, k, 0, None, 5, vp(out_i), None) == Status.INVALID_ARGUMENT
    assert L.sbr_score_candidates(h, vp(ptr), vp(it), nu, vp(cp), None, vp(out_s)) == Status.INVALID_ARGUMENT  # lists without items
    assert L.sbr_score_candidates_reps(h, vp(reps), nu, vp(cp), None, vp(out_s)) == Status.INVALID_ARGUMENT
    # scores are optional for recommend_among
    assert L.sbr_recommend_among(h, vp(ptr), vp(it), nu, k, 0, vp(S), S.size, vp(out_i), None) == Status.OK
    assert np.array_equal(out_i, g.recommend_among(ptr, it, k, S)[0])
    assert L.sbr_recommend_among_reps(h, vp(reps), nu, k, None, None, vp(S), S.size, vp(out_i), None) == Status.OK
    assert np.array_equal(out_i, g.recommend_among_reps(reps, k, S)[0])
    # an empty set: rows of padding; no pairs, no users: no-ops
    ei, es = g.recommend_among(ptr, it, k, [])
    assert np.all(ei == NO_ITEM) and np.all(np.isneginf(es)) and ei.shape == (nu, k)
    ei, es = g.recommend_among_reps(reps, k, np.zeros(0, np.uint32))
    assert np.all(ei == NO_ITEM) and np.all(np.isneginf(es))
    zero = np.zeros(nu + 1, np.uint64)
    assert L.sbr_score_candidates(h, vp(ptr), vp(it), nu, vp(zero), None, None) == Status.OK
    assert all(x.size == 0 for x in g.score_candidates_reps(reps, zero, np.zeros(0, np.uint32)))
    # a non-finite score raises, and the flag does not outlive the call
    big = E.copy()
    big[123] = 3e19
    b, _ = _pair(items, 8, d, ModelKind.LSTM_NORMAL, big, bias, oracle=False)
    huge = np.full((nu, d), 1e19, np.float32)
    with_bad = [np.array([1, 2, 123, 4], np.uint32)] + cands[1:]
    wp, wi = _csr(with_bad)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        b.score_candidates_reps(huge, wp, wi)
    _same_lists(b.score_candidates_reps(huge, cp, ci), [b.predict(huge[u], cands[u]) for u in range(nu)])


# ---- 10. reads parameters only --------------------------------------------------------------------------------------------------
def test_candidates_read_parameters_only():
    items, d, k = 900, 64, 50
    rs = np.random.RandomState(2)
    g = Model(hparams(items, 8, d, int(ModelKind.LSTM_NORMAL), LOSS_HINGE, B=8))
    g.set_param(Param.ITEM_BIAS, rs.randn(items).astype(np.float32))
    hists = [rs.randint(0, items, 6) for _ in range(30)]
    ptr = np.arange(0, 6 * 31, 6, dtype=np.uint64)
    it = np.concatenate(hists).astype(np.uint32)

    def snapshot():
        return [g.get_param(p).copy() for p in Param if g.param_count(p)], g.recommend(ptr, it, k)

    before, rec_before = snapshot()
    S = np.arange(0, items, 4, dtype=np.uint32)
    cp, ci = _csr([rs.randint(0, items, 70) for _ in range(30)])
    reps = g.user_representations(ptr, it)
    g.score_candidates(ptr, it, cp, ci)
    g.score_candidates_reps(reps, cp, ci)
    g.recommend_among(ptr, it, k, S)
    g.recommend_among_reps(reps, k, S)
    after, rec_after = snapshot()
    assert len(before) == len(after) and len(before) >= 6
    for a, b in zip(before, after):
        assert np.array_equal(_bits(a), _bits(b))
    _same(rec_after, rec_before)
