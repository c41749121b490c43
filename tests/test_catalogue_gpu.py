"""GPU: the catalogue scan (sbr_catalogue.hip: rank_gemm_kernel behind mrr_score, topk_gemm_kernel + topk_merge_kernel behind
recommend) on the paths the host's item-range split keeps test-sized shapes away from: several 32-item tiles per range (the LDS
double buffer, the packed rank counters), lists that fill (the live threshold and its id tie-break, staging overflow and the
re-offer loop, entries pushed past k), exclusion under load, and the host's chunking over users.

Which path a shape reaches is decided by the number of item ranges, so the tests force it with the library's test hook
SBR_CATALOGUE_GROUPS=n: the ranges are then ceil(items / n) items rounded up to whole 32-item tiles (`_range_len`), under the
launchers' hard limits.  Everything is compared bit for bit (items, ranks, score bits) with one of two references:

  * the oracle (user_representation + predict over every item, mrr_score), then recommend_expect.topk_expectation;
  * designed scores through recommend_reps: d = 16, reps[u] = (x_u, 0, ...), E[i] = (y_i, 0, ...), all values small integers
    times a power of two, so b[i] + x_u * y_i is exact in f32 whatever the order of operations; the expectation is numpy in
    float64, and `_designed_scores` asserts that it equals its own f32 cast."""
import functools

import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleError, OracleModel
from recommend_expect import NO_ITEM, topk_expectation
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import PredictionError

pytestmark = pytest.mark.gpu

KINDS = [ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA]
HOOK = "SBR_CATALOGUE_GROUPS"


def _force(monkeypatch, groups):
    if groups is None:
        monkeypatch.delenv(HOOK, raising=False)
    else:
        monkeypatch.setenv(HOOK, str(groups))


def _range_len(items, groups):
    """Items per range of a scan forced to `groups` ranges (split_items: whole 32-item tiles)."""
    groups = max(1, min(groups, (items + 31) // 32))
    return ((items + groups - 1) // groups + 31) // 32 * 32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    gi, gs = got
    wi, ws = want
    assert gi.shape == wi.shape, (what, gi.shape, wi.shape)
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: {len(bad)} items differ; first at {bad[0]}: {gi[tuple(bad[0])]} vs {wi[tuple(bad[0])]}"
    bad = np.argwhere(_bits(gs) != _bits(ws))
    assert bad.size == 0, f"{what}: {len(bad)} score bits differ; first at {bad[0]}"


def _pair(items, T, d, kind, E, bias):
    hp = hparams(items, T, d, int(kind), LOSS_HINGE, B=8)
    g, o = Model(hp), OracleModel(hp)
    for m in (g, o):
        m.set_param(Param.ITEM_EMBEDDING, E)
        m.set_param(Param.ITEM_BIAS, bias)
    return g, o


def _heavy_tie_params(items, d, seed):
    """E rows drawn from 50 distinct rows (the r-th with weight 1 / (r + 1)) and biases from 4 values: 200 score classes, the
    largest of several hundred items at 5 000 items, so the k-th score is almost always shared and the id decides."""
    rs = np.random.RandomState(seed)
    rows = (rs.randn(50, d) * 0.3).astype(np.float32)
    p = 1.0 / np.arange(1, 51)
    E = rows[rs.choice(50, size=items, p=p / p.sum())]
    bias = np.array([-0.5, 0.0, 0.25, 0.5], np.float32)[rs.randint(0, 4, items)]
    return np.ascontiguousarray(E), bias


def _histories(ptr, it):
    ptr = np.asarray(ptr, dtype=np.int64)
    return [np.asarray(it[ptr[u]: ptr[u + 1]], dtype=np.uint32) for u in range(len(ptr) - 1)]


def _oracle_scores(o, items, hists):
    """[users, items] f32: the oracle's score of every item for every history."""
    all_items = np.arange(items, dtype=np.uint32)
    return np.array([o.predict(o.user_representation(h), all_items) for h in hists], np.float32).reshape(len(hists), items)


def _expect(scores, excl, k):
    """topk_expectation of every row of scores; excl: one list per row, or None."""
    rows = [topk_expectation(scores[u], () if excl is None else excl[u], k) for u in range(len(scores))]
    return (np.array([r[0] for r in rows], np.uint32).reshape(-1, k), np.array([r[1] for r in rows], np.float32).reshape(-1, k))


def _csr(hists):
    ptr = np.zeros(len(hists) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(h) for h in hists])
    it = np.concatenate([np.asarray(h, np.uint32) for h in hists] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return ptr, it


# ------------------------------------------------------------------------------------------------
# recommend: long ranges, heavy ties, against the oracle
# ------------------------------------------------------------------------------------------------
LONG_ITEMS, LONG_USERS, LONG_T = 5007, 130, 12
LONG_KS = (1, 31, 32, 33, 100, 1000, 1024)


@functools.lru_cache(maxsize=None)
def _long_case(kind, d):
    """Parameters, histories and the oracle's scores of the long-range test, shared by its forced group counts."""
    E, bias = _heavy_tie_params(LONG_ITEMS, d, 100 + d)
    hp = hparams(LONG_ITEMS, LONG_T, d, int(kind), LOSS_HINGE, B=8)
    o = OracleModel(hp)
    o.set_param(Param.ITEM_EMBEDDING, E)
    o.set_param(Param.ITEM_BIAS, bias)
    ptr, it = synthetic_interactions(LONG_USERS, LONG_ITEMS, 3 * LONG_T, seed=d, min_len=0, zipf=True)
    hists = _histories(ptr, it)
    return hp, E, bias, ptr, it, hists, _oracle_scores(o, LONG_ITEMS, hists)


@pytest.mark.parametrize("groups", [1, 3, None])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 16, 64, 100, 256])
def test_recommend_long_ranges_heavy_ties(monkeypatch, groups, kind, d):
    """topk_gemm_kernel with a full list: the live threshold (thS, thI) and its id tie-break, staging buffers that overflow and
    the re-offer loop, list entries pushed past k, at every width class (d = 1 and 100 zero-padded, 256 with its own launch
    bounds).  Forced to 1 range: 1 x 5 024 items = 157 tiles per workgroup; to 3: 3 x 1 696 = 53 tiles; unset: the split of the
    day.  Every range holds at least k + 64 eligible items for every user (asserted), so every list fills and then drops
    entries; the largest score classes have hundreds of items, so the threshold is tied most of the time.  130 users: the
    second user tile holds two users (its waves 1-3 are empty).  All users against the oracle, history excluded and included."""
    _force(monkeypatch, groups)
    hp, E, bias, ptr, it, hists, scores = _long_case(kind, d)
    if groups is not None:
        per = _range_len(LONG_ITEMS, groups)
        assert per >= 3 * 32 and (LONG_ITEMS + per - 1) // per == groups
        longest = max(len(h) for h in hists)
        assert LONG_ITEMS - (groups - 1) * per - longest >= max(LONG_KS) + 64  # the last, shortest range
    assert min(len(h) for h in hists) == 0
    _, cnt = np.unique(scores[0], return_counts=True)
    assert cnt.max() >= 200  # heavy ties
    g = Model(hp)
    g.set_param(Param.ITEM_EMBEDDING, E)
    g.set_param(Param.ITEM_BIAS, bias)
    uniq = [np.unique(h) for h in hists]
    for k in LONG_KS:
        _same(g.recommend(ptr, it, k), _expect(scores, uniq, k), f"k={k} excluded")
        _same(g.recommend(ptr, it, k, include_history=True), _expect(scores, None, k), f"k={k} included")


# ------------------------------------------------------------------------------------------------
# recommend_reps: designed scores
# ------------------------------------------------------------------------------------------------
def _designed_model(y, b):
    """d = 16 model whose score of item i for the representation (x, 0, ...) is b[i] + x * y[i]."""
    items = len(y)
    E = np.zeros((items, 16), np.float32)
    E[:, 0] = y
    g = Model(hparams(items, 8, 16, int(ModelKind.EWMA), LOSS_HINGE, B=8))
    g.set_param(Param.ITEM_EMBEDDING, E)
    g.set_param(Param.ITEM_BIAS, np.asarray(b, np.float32))
    return g


def _designed_scores(x, y, b):
    """float64 b + x * y for one user; asserts that product and sum are f32 values (no rounding anywhere)."""
    p = np.float64(x) * np.asarray(y, np.float64)
    s = np.asarray(b, np.float64) + p
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p) and np.array_equal(s.astype(np.float32).astype(np.float64), s)
    s32 = np.asarray(b, np.float32) + np.float32(x) * np.asarray(y, np.float32)  # the same in f32 arithmetic
    assert np.array_equal(_bits(s32), _bits(s.astype(np.float32)))
    return s.astype(np.float32)


def _reps(xs):
    r = np.zeros((len(xs), 16), np.float32)
    r[:, 0] = xs
    return r


def _designed_expect(xs, y, b, k, excl=None):
    """Expectation per user; users without exclusions that share x share the row."""
    cache, ri, rs = {}, [], []
    for u, x in enumerate(xs):
        key = float(x)
        if excl is not None and len(excl[u]):
            row = topk_expectation(_designed_scores(x, y, b), excl[u], k)
        else:
            if key not in cache:
                cache[key] = topk_expectation(_designed_scores(x, y, b), (), k)
            row = cache[key]
        ri.append(row[0])
        rs.append(row[1])
    return np.array(ri, np.uint32).reshape(-1, k), np.array(rs, np.float32).reshape(-1, k)


DES_ITEMS, DES_USERS = 200_000, 300
S = 2.0 ** -10


def _design(name):
    ids = np.arange(DES_ITEMS, dtype=np.float64)
    u = np.arange(DES_USERS)
    if name == "equal":          # every score 0.25 whatever x: the id alone orders the catalogue
        return (1 + u % 4) * S, np.zeros(DES_ITEMS), np.full(DES_ITEMS, 0.25)
    if name == "ascending":      # every item beats the threshold: a merge per 32 items, every list entry moves every time
        return (1 + u % 4) * S, ids, np.zeros(DES_ITEMS)
    if name == "descending":     # after the first k items nothing beats the threshold
        return -(1.0 + u % 4) * S, ids, np.zeros(DES_ITEMS)
    if name == "sawtooth":       # period 33: runs of equal scores straddle the 32-item tiles
        return (1 + u % 4) * S, ids % 33, np.zeros(DES_ITEMS)
    if name == "flips":          # neighbouring users of one wave want opposite ends; user 77 has x = 0: bias only
        x = np.where(u % 2 == 0, 1.0, -1.0) * (1 + u % 3) * S
        x[77] = 0.0
        return x, ids, (np.arange(DES_ITEMS) % 7) * 0.125
    raise ValueError(name)


@pytest.mark.parametrize("groups", [1, None])
@pytest.mark.parametrize("name", ["equal", "ascending", "descending", "sawtooth", "flips"])
def test_recommend_designed_scores(monkeypatch, groups, name):
    """topk_gemm_kernel's merging at its extremes, 300 users x 200 000 items, d = 16, k = 10, 100, 1024.  Forced to 1 range:
    1 x 200 000 items = 6 250 tiles per workgroup (unset: the split of the day, 8 ranges at k = 1024).  Designed scores: all
    equal; ascending in the id (worst-case merging); descending; a sawtooth of period 33 (ties that straddle tiles); per-user
    sign flips, so the lanes of one wave take opposite branches, with one bias-only user."""
    _force(monkeypatch, groups)
    x, y, b = _design(name)
    g = _designed_model(y, b)
    want = _designed_expect(x, y, b, 1024)
    if name == "equal":
        assert np.array_equal(want[0][5], np.arange(1024))
    if name == "flips":
        assert x[77] == 0.0 and x[76] * x[78] > 0 > x[76] * x[75]
    for k in (10, 100, 1024):
        _same(g.recommend_reps(_reps(x), k), (want[0][:, :k], want[1][:, :k]), f"{name} k={k}")


def test_recommend_exclusion_under_load(monkeypatch):
    """The exclusion search inside merge_staged with full staging buffers, forced to 1 range of 20 000 items (625 tiles),
    k = 100, designed monotone scores (even users want the high ids, odd users the low ones).  Five kinds of user side by side,
    so the lanes of one wave take different branches: one excludes its 5 000 best items (whole staging buffers of excluded
    candidates: ne == 0), one excludes everything (a row of padding), one leaves k - 1 items, one passes an unsorted list with
    duplicates, one excludes nothing."""
    _force(monkeypatch, 1)
    items, k, users = 20_000, 100, 70
    ids = np.arange(items, dtype=np.float64)
    u = np.arange(users)
    x = np.where(u % 2 == 0, 1.0, -1.0) * (1 + u % 3) * S
    b = (np.arange(items) % 5) * 0.25
    rs = np.random.RandomState(11)
    excl = []
    for i in range(users):
        best_first = np.arange(items - 1, -1, -1) if x[i] > 0 else np.arange(items)
        kind = i % 5
        if kind == 0:
            e = best_first[:5000]
        elif kind == 1:
            e = np.arange(items)
        elif kind == 2:
            e = rs.permutation(items)[: items - (k - 1)]
        elif kind == 3:
            e = np.concatenate([best_first[:40:2], best_first[:40:2], rs.randint(0, items, 300)])
            rs.shuffle(e)
        else:
            e = np.zeros(0, np.int64)
        excl.append(e.astype(np.uint32))
    g = _designed_model(ids, b)
    want = _designed_expect(x, ids, b, k, excl)
    assert np.all(want[0][1] == NO_ITEM) and np.all(np.isneginf(want[1][1]))
    assert want[0][2][k - 2] != NO_ITEM and want[0][2][k - 1] == NO_ITEM
    assert not set(want[0][0].tolist()) & set(excl[0].tolist())
    _same(g.recommend_reps(_reps(x), k, exclude=excl), want)


# ------------------------------------------------------------------------------------------------
# extreme magnitudes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, None])
@pytest.mark.parametrize("case", ["subnormal_products", "subnormal_biases", "negative_zero", "near_flt_max"])
def test_recommend_extreme_magnitudes(monkeypatch, groups, case):
    """recommend, predict and the oracle agree bit for bit where f32 runs out: products in the subnormal range (E and the EWMA
    state around 2^-70), subnormal biases, scores that are -0.0 (a -0.0 bias plus negative products that underflow; -0.0 ties
    with +0.0 and the id decides), and scores near FLT_MAX that stay finite.  The f32 MFMA chain must keep subnormals as the
    scalar fma of predict and of the oracle does.  700 items, d = 16, 40 users, k = 50; forced to 1 range of
    704 items = 22 tiles."""
    _force(monkeypatch, groups)
    items, d, T, k = 700, 16, 8, 50
    rs = np.random.RandomState(3)
    if case == "subnormal_products":
        E = (rs.randint(-64, 65, (items, d)) * 2.0 ** -76).astype(np.float32)
        bias = np.zeros(items, np.float32)
    elif case == "subnormal_biases":
        E = (rs.randint(-64, 65, (items, d)) * 2.0 ** -76).astype(np.float32)
        bias = (rs.randint(-50, 51, items) * 2.0 ** -149).astype(np.float32)
    elif case == "negative_zero":
        E = (rs.randint(-3, 4, (items, d)) * 2.0 ** -100).astype(np.float32)
        bias = np.where(rs.rand(items) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    else:
        E = (rs.randn(items, d) * 2.0 ** 58).astype(np.float32)
        bias = (rs.randn(items) * 1e38).clip(-3e38, 3e38).astype(np.float32)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(40, items, 2 * T, seed=4, min_len=1)
    hists = _histories(ptr, it)
    scores = _oracle_scores(o, items, hists)
    assert np.all(np.isfinite(scores))
    tiny = np.float32(2.0 ** -126)
    if case in ("subnormal_products", "subnormal_biases"):
        assert np.mean((scores != 0) & (np.abs(scores) < tiny)) > 0.9  # the scores themselves are subnormal
    if case == "negative_zero":
        assert np.all(scores == 0) and 0.02 < np.mean(np.signbit(scores)) < 0.98
    if case == "near_flt_max":
        assert np.abs(scores).max() > 1e38
    all_items = np.arange(items, dtype=np.uint32)
    for u in (0, 17, 39):
        rep_o, rep_g = o.user_representation(hists[u]), g.user_representation(hists[u])
        assert np.array_equal(_bits(rep_o), _bits(rep_g))
        assert np.array_equal(_bits(g.predict(rep_g, all_items)), _bits(scores[u])), "predict differs from the oracle"
    _same(g.recommend(ptr, it, k), _expect(scores, [np.unique(h) for h in hists], k), case)
    _same(g.recommend(ptr, it, k, include_history=True), _expect(scores, None, k), case)


def test_recommend_overflow_in_last_step(monkeypatch):
    """A score whose chain is finite after 15 of its 16 steps and overflows in the last one fails the call with
    InvalidPredictionValue: in recommend_reps (1 range and the split of the day), in predict, and in the oracle.  Without
    that item every score is finite (below 2^128) and the calls succeed."""
    items, d, k = 500, 16, 10
    E = np.full((items, d), 2.0 ** 60, np.float32)
    E[:, 0] = (np.arange(items) % 9) * 2.0 ** 56
    bias = np.zeros(items, np.float32)
    reps = np.full((3, d), 2.0 ** 63, np.float32)
    all_items = np.arange(items, dtype=np.uint32)
    g, o = _pair(items, 8, d, ModelKind.EWMA, E, bias)
    want = _expect(np.array([o.predict(r, all_items) for r in reps]), None, k)
    for groups in (1, None):
        _force(monkeypatch, groups)
        _same(g.recommend_reps(reps, k), want)
    E[321, :] = 2.0 ** 60
    E[321, d - 1] = 2.0 ** 65  # 15 x 2^123, then + 2^128
    partial = np.float32(0)
    for j in range(d - 1):
        partial = np.float32(partial + np.float32(reps[0, j]) * np.float32(E[321, j]))
    assert np.isfinite(partial)
    g, o = _pair(items, 8, d, ModelKind.EWMA, E, bias)
    for groups in (1, None):
        _force(monkeypatch, groups)
        with pytest.raises(PredictionError.InvalidPredictionValue):
            g.recommend_reps(reps, k)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.predict(reps[0], all_items)
    with pytest.raises(OracleError) as e:
        o.predict(reps[0], all_items)
    assert e.value.status == Status.INVALID_PREDICTION


# ------------------------------------------------------------------------------------------------
# small and odd shapes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("items", [1, 5, 31, 32, 33])
def test_recommend_tiny_catalogues(monkeypatch, items):
    """Catalogues of at most two tiles with k = 1, 10, 1024 (k > items: rows padded with (NO_ITEM, -inf)); forced group counts
    1 and 2 (2 is cut to the number of tiles) and unset.  LSTM, d = 16, 20 users."""
    d, T = 16, 6
    E, bias = _heavy_tie_params(items, d, items)
    g, o = _pair(items, T, d, ModelKind.LSTM_NORMAL, E, bias)
    ptr, it = synthetic_interactions(20, items, 4, seed=items, min_len=0)
    hists = _histories(ptr, it)
    scores = _oracle_scores(o, items, hists)
    uniq = [np.unique(h) for h in hists]
    for groups in (1, 2, None):
        _force(monkeypatch, groups)
        for k in (1, 10, 1024):
            got = g.recommend(ptr, it, k)
            _same(got, _expect(scores, uniq, k), f"groups={groups} k={k}")
            assert np.all(got[0][:, items:] == NO_ITEM)
            _same(g.recommend(ptr, it, k, include_history=True), _expect(scores, None, k), f"groups={groups} k={k} included")


@pytest.mark.parametrize("users", [1, 127, 128, 129, 257])
def test_recommend_user_tile_edges(monkeypatch, users):
    """User counts around the 128-user tile (the last tile holds 1, 127, 128 users) forced to 1 range of 2 016 items = 63 tiles,
    k = 33 and 200, EWMA, d = 64, heavy ties."""
    _force(monkeypatch, 1)
    items, d, T = 2003, 64, 10
    E, bias = _heavy_tie_params(items, d, users)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(users, items, 2 * T, seed=users, min_len=0)
    hists = _histories(ptr, it)
    scores = _oracle_scores(o, items, hists)
    for k in (33, 200):
        _same(g.recommend(ptr, it, k), _expect(scores, [np.unique(h) for h in hists], k), f"k={k}")


@pytest.mark.parametrize("k,groups", [(683, 7), (683, 8), (1023, 7), (1023, 8), (1024, 8), (1024, 7)])
def test_recommend_merge_sizes(monkeypatch, k, groups):
    """topk_merge_kernel's sort sizes: groups * k a non-power-of-two below TK_MERGE_MAX = 8 192 (683 x 7, 683 x 8, 1 023 x 7,
    1 023 x 8 = 8 184) and exactly 8 192 (1 024 x 8).  9 200 items forced to 7 ranges of 1 344 and 8 of 1 152 items (the last holds 1 136): each range
    holds more than k eligible items (asserted), so every list reaches the merge full.  LSTM coupled, d = 16, 130 users."""
    _force(monkeypatch, groups)
    items, d, T = 9200, 16, 8
    per = _range_len(items, groups)
    assert (items + per - 1) // per == groups and groups * k <= 8192
    E, bias = _heavy_tie_params(items, d, k)
    g, o = _pair(items, T, d, ModelKind.LSTM_COUPLED, E, bias)
    ptr, it = synthetic_interactions(130, items, 2 * T, seed=k, min_len=0)
    hists = _histories(ptr, it)
    assert items - (groups - 1) * per - max(len(h) for h in hists) > k
    scores = _oracle_scores(o, items, hists)
    _same(g.recommend(ptr, it, k), _expect(scores, [np.unique(h) for h in hists], k))


# ------------------------------------------------------------------------------------------------
# the host's chunking over users
# ------------------------------------------------------------------------------------------------
def test_recommend_two_chunks_k1024():
    """sbr_recommend and sbr_recommend_reps cut at recommend_users_cap = 4 096 users for k = 1024: 4 096 + 130 users give two
    launches, the second writing at out + 4 096 k.  1 100 items, EWMA, d = 16.  (a) recommend, every user against the oracle;
    (b) recommend_reps with designed representations distinct per user (user u's best item is u % 1 100)."""
    users, items, d, T, k = 4096 + 130, 1100, 16, 8, 1024
    E, bias = _heavy_tie_params(items, d, 21)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(users, items, 2 * T, seed=22, min_len=0)
    hists = _histories(ptr, it)
    scores = _oracle_scores(o, items, hists)
    _same(g.recommend(ptr, it, k), _expect(scores, [np.unique(h) for h in hists], k), "recommend")
    # (b) s[u][i] = x_u * i with x_u = (u - users / 2) 2^-12: distinct per user, the sign changes in the middle
    ids = np.arange(items, dtype=np.float64)
    x = (np.arange(users) - users // 2) * 2.0 ** -12
    gd = _designed_model(ids, np.zeros(items))
    got = gd.recommend_reps(_reps(x), k)
    want = _designed_expect(x, ids, np.zeros(items), k)
    _same(got, want, "recommend_reps")
    assert len(np.unique(got[1][:, 1])) >= users - 1  # the rows are distinct: a misplaced chunk cannot go unseen


def test_recommend_two_chunks_k100():
    """sbr_recommend cuts at 8 192 users below k = 257: 8 192 + 200 users, k = 100, 700 items, LSTM, d = 16, every user against
    the oracle."""
    users, items, d, T, k = 8192 + 200, 700, 16, 6, 100
    E, bias = _heavy_tie_params(items, d, 31)
    g, o = _pair(items, T, d, ModelKind.LSTM_NORMAL, E, bias)
    ptr, it = synthetic_interactions(users, items, 2 * T, seed=32, min_len=0)
    hists = _histories(ptr, it)
    scores = _oracle_scores(o, items, hists)
    _same(g.recommend(ptr, it, k), _expect(scores, [np.unique(h) for h in hists], k))


def test_mrr_two_chunks_with_unranked_users():
    """sbr_mrr_score cuts at 8 192 RANKED users: 9 800 users of whom every 7th has fewer than two interactions leave 8 400
    ranked, so the second launch writes ranks + 8 192 and the MRR sums across both.  600 items, EWMA, d = 16: ranks, their
    count and the MRR bits against the oracle."""
    users, items, d, T = 9800, 600, 16, 8
    E, bias = _heavy_tie_params(items, d, 41)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(users, items, 2 * T, seed=42, min_len=2)
    hists = _histories(ptr, it)
    for u in range(0, users, 7):
        hists[u] = hists[u][: (u // 7) % 2]  # 0 or 1 interactions: not ranked
    ptr, it = _csr(hists)
    mg, rg = g.mrr_score(ptr, it)
    mo, ro = o.mrr_score(ptr, it)
    assert ro.size == users - len(range(0, users, 7)) == 8400
    assert rg.size == ro.size and np.array_equal(rg, ro)
    assert _bits(mg) == _bits(mo)
    assert len(np.unique(ro[8192:])) > 20


def test_chunks_by_forward_rows():
    """Both scans also cut a launch at 2^22 forward rows: T = 600 and 7 100 users with histories of 601..620 items are
    4.26 M rows, two launches of fewer than 8 192 users.  EWMA, d = 16, 300 items: mrr_score (ranks, MRR bits) and recommend
    (k = 10) against the oracle."""
    users, items, d, T, k = 7100, 300, 16, 600, 10
    E, bias = _heavy_tie_params(items, d, 51)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(users, items, T + 20, seed=52, min_len=T + 1)
    assert users * T > 2 ** 22 and users < 8192
    mg, rg = g.mrr_score(ptr, it)
    mo, ro = o.mrr_score(ptr, it)
    assert rg.size == users and np.array_equal(rg, ro) and _bits(mg) == _bits(mo)
    hists = _histories(ptr, it)
    scores = _oracle_scores(o, items, hists)
    _same(g.recommend(ptr, it, k), _expect(scores, [np.unique(h) for h in hists], k))


# ------------------------------------------------------------------------------------------------
# mrr_score: several tiles per range
# ------------------------------------------------------------------------------------------------
def _mrr_same(g, o, ptr, it, min_ranked):
    mg, rg = g.mrr_score(ptr, it)
    mo, ro = o.mrr_score(ptr, it)
    assert rg.shape == ro.shape and ro.size >= min_ranked
    bad = np.flatnonzero(rg != ro)
    assert bad.size == 0, f"{bad.size} ranks differ; first: user {bad[0]}: {rg[bad[0]]} vs {ro[bad[0]]}"
    assert _bits(mg) == _bits(mo)
    return ro


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("kind,d,items,users", [
    (ModelKind.EWMA, 128, 5003, 700),
    (ModelKind.LSTM_NORMAL, 32, 1683, 180),
    (ModelKind.LSTM_COUPLED, 256, 999, 37),
    (ModelKind.EWMA, 16, 70, 300),
    (ModelKind.LSTM_NORMAL, 64, 2500, 130),
    (ModelKind.EWMA, 100, 1500, 129),      # zero-padded width
])
def test_mrr_multi_tile_ranges(monkeypatch, groups, kind, d, items, users):
    """rank_gemm_kernel's tile loop run more than once: the fetch of tile + 1 during the MFMA chain, the stage into the other
    LDS half, counters that grow past 1.  The shapes of test_mrr_gemm_ranks_bit_exact plus d = 64 and a padded width, forced
    to 1 range (157, 53, 32, 3, 79, 47 tiles) and to 3 ranges (a third of that each, 1 tile at 70 items).  Heavy ties: many
    items share the test item's score, which `>=` counts and `>` would not (asserted on the oracle's scores)."""
    _force(monkeypatch, groups)
    T = 24
    E, bias = _heavy_tie_params(items, d, d)
    g, o = _pair(items, T, d, kind, E, bias)
    ptr, it = synthetic_interactions(users, items, 3 * T, seed=77, min_len=1, zipf=True)
    assert _range_len(items, groups) >= 64 or items == 70
    if items >= 500:  # the test item's score is shared with other items for most users (70 items: too few per score class)
        all_items = np.arange(items, dtype=np.uint32)
        ranked = [h for h in _histories(ptr, it) if len(h) >= 2][:30]
        shared = [np.sum(s == s[h[-1]]) >= 3 for h in ranked for s in [o.predict(o.user_representation(h[:-1]), all_items)]]
        assert np.mean(shared) > 0.5
    _mrr_same(g, o, ptr, it, users // 2)


def test_mrr_natural_multi_tile():
    """Several tiles per range WITHOUT the hook: 700 users x 100 003 items, d = 32 is 6 user tiles, so the split wants 768
    workgroups per user tile's share (4 608 / 6) and cuts 626 ranges of 160 items = 5 tiles.  Should the split change, the
    forced cases above keep the path."""
    items, d, T, users = 100_003, 32, 12, 700
    E, bias = _heavy_tie_params(items, d, 5)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(users, items, 2 * T, seed=6, min_len=1, zipf=True)
    _mrr_same(g, o, ptr, it, users // 2)


@pytest.mark.parametrize("users", [127, 128, 129, 257])
def test_mrr_edges(monkeypatch, users):
    """mrr_score forced to 1 range of 1 216 items = 38 tiles with: all scores equal (rank = items - distinct history items, or
    items where the test item is in the history); test items inside the history; histories longer than T with duplicates; user
    counts around the 128-user tile.  LSTM, d = 32."""
    _force(monkeypatch, 1)
    items, d, T = 1201, 32, 8
    E = np.tile(np.linspace(-1, 1, d, dtype=np.float32), (items, 1))
    bias = np.full(items, 0.25, np.float32)
    g, o = _pair(items, T, d, ModelKind.LSTM_NORMAL, E, bias)
    rs = np.random.RandomState(users)
    hists = []
    for u in range(users):
        h = rs.randint(0, items, rs.randint(2, 3 * T))
        if u % 3 == 0:
            h[-1] = h[0]                 # the test item is in the history
        if u % 3 == 1 and len(h) > 4:
            h[1:-1:2] = h[0]             # duplicates
            if h[-1] == h[0]:
                h[-1] = (h[0] + 1) % items
        hists.append(h.astype(np.uint32))
    ptr, it = _csr(hists)
    ro = _mrr_same(g, o, ptr, it, users)
    for u, h in enumerate(hists):
        assert ro[u] == (items if h[-1] in h[:-1] else items - len(np.unique(h[:-1])))
    # and with heavy-tie parameters
    E, bias = _heavy_tie_params(items, d, users)
    g, o = _pair(items, T, d, ModelKind.LSTM_NORMAL, E, bias)
    _mrr_same(g, o, ptr, it, users)


def test_mrr_counter_width(monkeypatch):
    """rank_gemm_kernel packs two 16-bit counters per register, so launch_rank may give a range at most 65 535 tiles.  Forced to
    1 range, 65 535 * 32 + 33 = 2 097 153 items must still be cut in two (65 535 tiles + 2), and with every item scoring at or
    above the test item every lane of the first range counts to exactly 65 535: one more and it would carry into its
    neighbour.  d = 16, EWMA, E = 0, bias 1 everywhere but 0 at the three test items; 3 users."""
    _force(monkeypatch, 1)
    items, d, T = 65535 * 32 + 33, 16, 4
    E = np.zeros((items, d), np.float32)
    bias = np.ones(items, np.float32)
    tests = [5, 1_000_000, items - 1]
    bias[tests] = 0.0
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    hists = [np.array(h, np.uint32) for h in ([9, 70_000, 9, tests[0]], [3, tests[1]], [9, 70_000, 9, tests[2]])]
    ptr, it = _csr(hists)
    ro = _mrr_same(g, o, ptr, it, 3)
    assert ro.tolist() == [items - 2, items - 1, items - 2]


def test_mrr_no_ranked_user():
    """No user with two interactions: the reference divides an empty sum by zero (evaluation.rs:47), the oracle returns NaN and
    no ranks (tests/test_oracle.py pins it), and so does the engine."""
    hp = hparams(50, 8, 16, int(ModelKind.EWMA), LOSS_HINGE, B=4)
    g, o = Model(hp), OracleModel(hp)
    for hists in ([], [[3]], [[3], [], [7]]):
        ptr, it = _csr([np.array(h, np.uint32) for h in hists])
        mg, rg = g.mrr_score(ptr, it)
        mo, ro = o.mrr_score(ptr, it)
        assert rg.size == ro.size == 0 and np.isnan(mg) and np.isnan(mo)


def test_rank_family_launch_counts():
    """The launches each catalogue call reports in the RANK family of the timing ledger (timing_read()["RANK"][1]; the read
    resets it): every tools/time_*.py "kernel time" is the event bracket these counts label.  One call each, all single-chunk:
    EWMA, d = 16, 300 items, 40 users with histories of 3..6 items, k = 5, pool = 8, an item subset of 50, 8 query items, item
    tags set, a session store of capacity 40 without memory and one with remember = 4.  The scan's own kernels count (top-k:
    the GEMM and the merge, plus the sub-table gather and the id translation of recommend_among, the norms and the query rows of
    similar_items, the selection of recommend_diverse, the seen-list build of a store with memory, the id translation of the
    store's audience); mrr_score reports its scan as one."""
    users, items, d, T, k, pool = 40, 300, 16, 8, 5, 8
    rs = np.random.RandomState(7)
    E, bias = _heavy_tie_params(items, d, 3)
    hp = hparams(items, T, d, int(ModelKind.EWMA), LOSS_HINGE, B=8)
    m = Model(hp)
    m.set_param(Param.ITEM_EMBEDDING, E)
    m.set_param(Param.ITEM_BIAS, bias)
    m.set_item_tags(rs.randint(1, 8, items).astype(np.uint32))
    hists = [rs.randint(0, items, rs.randint(3, 7)).astype(np.uint32) for _ in range(users)]
    ptr, it = _csr(hists)
    reps = m.user_representations(ptr, it)
    among = rs.choice(items, 50, replace=False).astype(np.uint32)
    queries = rs.randint(0, items, 8).astype(np.uint32)
    one_ptr = np.arange(users + 1, dtype=np.uint64)  # one candidate / one target per user
    one_item = rs.randint(0, items, users).astype(np.uint32)
    slots = np.arange(users, dtype=np.uint32)
    plain, memory = m.sessions(users), m.sessions(users, remember=4)
    plain.append(slots, hists)
    memory.append(slots, hists)
    calls = [
        ("mrr_score", 1, lambda: m.mrr_score(ptr, it)),
        ("recommend", 2, lambda: m.recommend(ptr, it, k)),
        ("recommend with masks", 2, lambda: m.recommend(ptr, it, k, any_of=3, none_of=4)),
        ("recommend_reps", 2, lambda: m.recommend_reps(reps, k)),
        ("recommend_diverse", 3, lambda: m.recommend_diverse(ptr, it, k, pool)),
        ("recommend_among", 4, lambda: m.recommend_among(ptr, it, k, among)),
        ("similar_items", 4, lambda: m.similar_items(queries, k)),
        ("similar_items with masks", 4, lambda: m.similar_items(queries, k, any_of=3, none_of=4)),
        ("score_candidates", 1, lambda: m.score_candidates(ptr, it, one_ptr, one_item)),
        ("user_representations", 1, lambda: m.user_representations(ptr, it)),
        ("rank_targets", 3, lambda: m.rank_targets(ptr, it, one_ptr, one_item)),
        ("audience_reps", 2, lambda: m.audience_reps(reps, queries, k)),
        ("Sessions.recommend, no memory", 2, lambda: plain.recommend(slots, k)),
        ("Sessions.recommend, memory", 3, lambda: memory.recommend(slots, k)),
        ("Sessions.recommend, memory, include_seen", 2, lambda: memory.recommend(slots, k, include_seen=True)),
        ("Sessions.recommend_diverse, memory", 4, lambda: memory.recommend_diverse(slots, k, pool)),
        ("Sessions.audience", 3, lambda: plain.audience(queries, k)),
    ]
    m.timing_enable(True)
    m.timing_read()
    got = {}
    for what, _, call in calls:
        call()
        got[what] = int(m.timing_read()["RANK"][1])
    m.timing_enable(False)
    print(got)
    assert got == {what: n for what, n, _ in calls}
