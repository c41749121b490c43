"""GPU: sbr_recommend_diverse / _reps / sbr_sessions_recommend_diverse (greedy MMR re-ranking of recommend's pool,
diverse_select_kernel in sbr_catalogue.hip) against the contract evaluated with the oracle's chain (diverse_expect.py).  Items and
score bits must be equal."""
import ctypes as C

import numpy as np
import pytest

from diverse_expect import DiverseExpectation, clustered_case, pool_from_histories, pool_from_reps
from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, PredictionError

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    gi, gs = got
    wi, ws = want
    assert gi.shape == wi.shape, (what, gi.shape, wi.shape)
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: {len(bad)} items differ; first at {bad[0]}: {gi[tuple(bad[0])]} vs {wi[tuple(bad[0])]}"
    assert np.array_equal(_bits(gs), _bits(ws)), what


def _pair(items, T, d, kind, E=None, bias=None):
    hp = hparams(items, T, d, int(kind), LOSS_HINGE, B=8)
    g, o = Model(hp), OracleModel(hp)
    for m in (g, o):
        if E is not None:
            m.set_param(Param.ITEM_EMBEDDING, E)
        if bias is not None:
            m.set_param(Param.ITEM_BIAS, bias)
    return g, o


def _planted(items, d, seed):
    """0.3 * randn with 20 copies of row 0 (exact ties), a zero row, a doubled and a negated row; biases on a 0.1 grid (score
    ties)."""
    rs = np.random.RandomState(seed)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    E[rs.choice(np.arange(10, items), 20, replace=False)] = E[0]
    E[5] = 0.0
    E[7] = 2.0 * E[3]
    E[9] = -E[3]
    bias = np.round(rs.randn(items) * 0.5, 1).astype(np.float32)
    return E, bias


def _max_pool(d):
    sd = 16 if d <= 16 else 32 if d <= 32 else 64 if d <= 64 else 128 if d <= 128 else 256
    return min(1024, 32768 // sd)


_SHAPES = [(1, 1300), (16, 1500), (32, 2000), (64, 900), (100, 700), (128, 600), (256, 1100)]
_USERS = 70


@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("d,items", _SHAPES)
def test_matches_expectation(d, items, metric, kind):
    T = 8
    E, bias = _planted(items, d, d + items)
    g, o = _pair(items, T, d, kind, E, bias)
    assert g.diverse_max_pool() == _max_pool(d)
    want = DiverseExpectation(E, metric)
    ptr, it = synthetic_interactions(_USERS, items, 3 * T, seed=d, min_len=0, zipf=True)
    reps = g.user_representations(ptr, it)
    rs = np.random.RandomState(d)
    excl = [rs.randint(0, items, rs.randint(0, 30)) for _ in range(_USERS)]
    excl[0] = np.delete(np.arange(items), 17)            # n == 1
    excl[1] = np.arange(5, items)[::-1]                   # n == 5: below k from 10 on
    excl[2] = np.arange(40, items)                        # n == 40: below the pool from 64 on
    for k, pool in ((1, 1), (10, 10), (10, 64), (33, 65), (20, _max_pool(d))):
        pools = {"masked": pool_from_histories(o, items, ptr, it, pool),
                 "kept": pool_from_histories(o, items, ptr, it, pool, include_history=True),
                 "reps": pool_from_reps(o, items, reps, pool, excl)}
        for t in (0.0, 0.3, 1.0):
            what = f"k={k} pool={pool} trade_off={t}"
            _same(g.recommend_diverse(ptr, it, k, pool, t, metric), want.rows(pools["masked"], k, t), what + " masked")
            _same(g.recommend_diverse(ptr, it, k, pool, t, metric, include_history=True), want.rows(pools["kept"], k, t), what + " kept")
            got = g.recommend_diverse_reps(reps, k, pool, t, metric, exclude=excl)
            _same(got, want.rows(pools["reps"], k, t), what + " reps")
            assert got[0][0, 0] == 17 and np.all(got[0][0, 1:] == NO_ITEM) and np.all(np.isneginf(got[1][0, 1:]))
            assert np.all(got[0][1, min(k, 5):] == NO_ITEM) and np.all(got[0][1, : min(k, 5)] != NO_ITEM)


@pytest.mark.parametrize("d,pool", [(128, 256), (256, 128), (16, 1024), (32, 1024), (64, 512)])
def test_pool_at_the_lds_limit(d, pool):
    items, k = 1500, pool // 2
    E, bias = _planted(items, d, d)
    g, o = _pair(items, 8, d, ModelKind.EWMA, E, bias)
    assert g.diverse_max_pool() == pool
    reps = (np.random.RandomState(d + 1).randn(9, d) * 0.5).astype(np.float32)
    for metric in ("cosine", "dot"):
        _same(g.recommend_diverse_reps(reps, k, pool, 0.3, metric), DiverseExpectation(E, metric).rows(pool_from_reps(o, items, reps, pool), k, 0.3), metric)
    with pytest.raises(EngineError) as e:
        g.recommend_diverse_reps(reps, k, pool + 1, 0.3)
    assert e.value.status == Status.INVALID_ARGUMENT
    oi, osc = np.full((9, k), 7, np.uint32), np.full((9, k), 7.0, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert g._L.sbr_recommend_diverse_reps(g._h, vp(reps), 9, k, pool + 1, 0.3, 0, None, None, vp(oi), vp(osc)) == Status.INVALID_ARGUMENT
    assert np.all(oi == 7) and np.all(osc == 7.0)


def test_ties_and_degenerate_rows():
    items, d = 300, 16
    rs = np.random.RandomState(3)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    bias = np.round(rs.randn(items) * 0.5, 1).astype(np.float32)
    E[10:20] = E[10]          # exact duplicates with one bias: every score, and every similarity to and from them, ties
    bias[10:20] = 2.0
    E[5] = 0.0                # r = 0: similarity 0 both ways
    bias[5] = 2.0
    E[7] = -E[10]             # the negated row
    bias[7] = 2.0
    g, o = _pair(items, 8, d, ModelKind.EWMA, E, bias)
    reps = (rs.randn(30, d) * 0.2).astype(np.float32)
    for metric in ("cosine", "dot"):
        want = DiverseExpectation(E, metric)
        for k, pool, t in ((12, 12, 0.5), (12, 40, 0.0), (25, 64, 0.3), (12, 40, 1.0)):
            got = g.recommend_diverse_reps(reps, k, pool, t, metric)
            _same(got, want.rows(pool_from_reps(o, items, reps, pool), k, t), f"{metric} {k} {pool} {t}")
            for row in got[0]:  # of the duplicates a row holds, the lower id was picked first
                dup = [int(i) for i in row if 10 <= i < 20]
                assert dup == sorted(dup)
    # identical rows and one bias: every score and every similarity ties, so the picks are the pool in its order, the ids ascending
    flat = np.tile(np.linspace(-1, 1, d, dtype=np.float32), (items, 1))
    g2, o2 = _pair(items, 8, d, ModelKind.EWMA, flat, np.full(items, 0.25, np.float32))
    for metric in ("cosine", "dot"):
        gi, gs = g2.recommend_diverse_reps(reps, 10, 64, 0.3, metric, exclude=[[0, 3]] * len(reps))
        assert all(r.tolist() == [1, 2, 4, 5, 6, 7, 8, 9, 10, 11] for r in gi)
        _same((gi, gs), DiverseExpectation(flat, metric).rows(pool_from_reps(o2, items, reps, 64, [[0, 3]] * len(reps)), 10, 0.3))
    # a catalogue with fewer items than k
    E3, b3 = (rs.randn(12, d) * 0.3).astype(np.float32), np.zeros(12, np.float32)
    g3, o3 = _pair(12, 8, d, ModelKind.LSTM_NORMAL, E3, b3)
    ptr, it = synthetic_interactions(20, 12, 4, seed=1, min_len=0)
    got = g3.recommend_diverse(ptr, it, 16, 32, 0.3, include_history=True)
    _same(got, DiverseExpectation(E3, "cosine").rows(pool_from_histories(o3, 12, ptr, it, 32, include_history=True), 16, 0.3))
    assert np.all(got[0][:, 12:] == NO_ITEM) and np.all(np.sort(got[0][:, :12], axis=1) == np.arange(12))


def test_identities():
    items, d, T, k = 1200, 100, 8, 20
    E, bias = _planted(items, d, 11)
    g, _ = _pair(items, T, d, ModelKind.LSTM_NORMAL, E, bias)
    ptr, it = synthetic_interactions(_USERS, items, 2 * T, seed=4, min_len=0)
    hists = [it[int(ptr[u]): int(ptr[u + 1])] for u in range(_USERS)]
    reps = g.user_representations(ptr, it)
    plain = g.recommend(ptr, it, k)
    for metric in ("cosine", "dot"):
        _same(g.recommend_diverse(ptr, it, k, 80, 1.0, metric), plain, "trade_off 1")
        _same(g.recommend_diverse_reps(reps, k, 80, 1.0, metric), g.recommend_reps(reps, k), "trade_off 1, reps")
        for t in (0.0, 0.4):
            pi, ps = g.recommend_diverse(ptr, it, k, k, t, metric)
            order = np.argsort(pi, axis=1, kind="stable")
            porder = np.argsort(plain[0], axis=1, kind="stable")
            _same((np.take_along_axis(pi, order, 1), np.take_along_axis(ps, order, 1)),
                  (np.take_along_axis(plain[0], porder, 1), np.take_along_axis(plain[1], porder, 1)), "pool == k")
            _same(g.recommend_diverse(ptr, it, k, 80, t, metric), g.recommend_diverse_reps(reps, k, 80, t, metric, exclude=hists), "histories vs reps")
    # a session store's rows in place: 70 shuffled slots of a larger store, every seventh left empty
    store = g.sessions(_USERS + 9)
    slots = np.random.RandomState(5).permutation(_USERS + 9)[:_USERS].astype(np.uint32)
    filled = [h if u % 7 else h[:0] for u, h in enumerate(hists)]
    store.append(slots, [h[:T] for h in filled])
    sreps = store.representations(slots)
    for metric in ("cosine", "dot"):
        _same(store.recommend_diverse(slots, k, 80, 0.3, metric, exclude=filled), g.recommend_diverse_reps(sreps, k, 80, 0.3, metric, exclude=filled), "sessions")
    _same(store.recommend_diverse(slots, k, 80, 1.0), store.recommend(slots, k), "sessions, trade_off 1")
    # the lstm / ewma wrapper: pool = min(4 k, the largest)
    import sbr_rs_amd as sbr

    w = sbr.lstm.ImplicitLSTMModel(g)
    _same(w.recommend_diverse(hists, k, trade_off=0.3), g.recommend_diverse(ptr, it, k, 4 * k, 0.3))
    _same(w.recommend_diverse(hists, 100, trade_off=0.3, exclude_history=False), g.recommend_diverse(ptr, it, 100, 256, 0.3, include_history=True))
    with pytest.raises(EngineError) as e:
        w.recommend_diverse(hists, 300)  # min(4 k, 256) < k: the C call's error
    assert e.value.status == Status.INVALID_ARGUMENT


@pytest.mark.parametrize("d", [16, 100, 128, 256])
def test_diversity_changes_the_list(d):
    """The clustered table (diverse_expect.clustered_case; tests/test_diverse_cpu.py holds the expectation to its condition at these
    widths): at least 36 of 40 rows differ from recommend's, the distinct clusters per row go from one to two, and the device's
    rows are the expectation's."""
    E, bias, reps = clustered_case(d, 0)
    items = E.shape[0]
    g, o = _pair(items, 8, d, ModelKind.EWMA, E, bias)
    got = g.recommend_diverse_reps(reps, 10, 64, 0.3, "cosine")
    plain = g.recommend_reps(reps, 10)
    assert int(np.count_nonzero(np.any(got[0] != plain[0], axis=1))) >= 36
    before, after = (float(np.mean([len(set((r % 12).tolist())) for r in rows])) for rows in (plain[0], got[0]))
    assert 1.0 <= before <= 1.1 and after >= 2.0, (before, after)
    _same(got, DiverseExpectation(E, "cosine").rows(pool_from_reps(o, items, reps, 64), 10, 0.3))


def test_two_chunks():
    """recommend's scan cuts at 8 192 users while the pool is at most 256: 8 192 + 200 users, the second launch's rows (c0 != 0)
    against the same users run alone."""
    users, items, d, T = 8192 + 200, 700, 16, 6
    E, bias = _planted(items, d, 31)
    g, _ = _pair(items, T, d, ModelKind.LSTM_NORMAL, E, bias)
    ptr, it = synthetic_interactions(users, items, 2 * T, seed=32, min_len=0)
    gi, gs = g.recommend_diverse(ptr, it, 10, 64, 0.3)
    p64 = np.asarray(ptr, dtype=np.int64)
    for lo, hi in ((8192, users), (0, 150)):
        alone = g.recommend_diverse(ptr[lo: hi + 1] - ptr[lo], it[p64[lo]: p64[hi]], 10, 64, 0.3)
        _same((gi[lo:hi], gs[lo:hi]), alone, f"users {lo}..{hi}")
    assert len(np.unique(gi[8192:], axis=0)) > 100  # the rows are distinct: a misplaced chunk cannot go unseen


def test_errors_and_flag():
    items, d, k, pool = 500, 32, 10, 40
    E, bias = _planted(items, d, 3)
    rs = np.random.RandomState(1)
    reps = (rs.randn(12, d) * 0.5).astype(np.float32)
    reps[:, 0] = 0.0
    ptr, it = synthetic_interactions(12, items, 10, seed=1)
    g, o = _pair(items, 8, d, ModelKind.LSTM_NORMAL, E, bias)
    params = lambda m: [m.get_param(p).copy() for p in Param if m.param_count(p)]  # noqa: E731
    before = params(g)
    bad_it = it.copy()
    bad_it[5] = items
    for call in (lambda: g.recommend_diverse_reps(reps, 0, pool), lambda: g.recommend_diverse_reps(reps, k, k - 1),
                 lambda: g.recommend_diverse_reps(reps, k, g.diverse_max_pool() + 1), lambda: g.recommend_diverse_reps(reps, k, pool, -0.01),
                 lambda: g.recommend_diverse_reps(reps, k, pool, 1.01), lambda: g.recommend_diverse_reps(reps, k, pool, float("nan")),
                 lambda: g.recommend_diverse_reps(reps, k, pool, 0.5, metric=2), lambda: g.recommend_diverse(ptr, it, k, pool, 0.5, metric=2),
                 lambda: g.recommend_diverse(ptr, it, 0, pool), lambda: g.recommend_diverse(ptr, it, k, 5), lambda: g.recommend_diverse(ptr, bad_it, k, pool),
                 lambda: g.recommend_diverse_reps(reps, k, pool, exclude=[[items]] + [[]] * 11)):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    up, ids = np.ascontiguousarray(ptr, np.uint64), np.ascontiguousarray(it, np.uint32)
    out = np.zeros((12, k), np.uint32)
    assert g._L.sbr_recommend_diverse(g._h, vp(up), vp(ids), 12, k, pool, 0.5, 0, 2, vp(out), None) == Status.INVALID_ARGUMENT  # an unknown flag
    assert g._L.sbr_recommend_diverse(g._h, vp(up), vp(ids), 12, k, pool, 0.5, 0, 0, vp(out), None) == Status.OK  # scores are optional
    assert np.array_equal(out, g.recommend_diverse(ptr, it, k, pool, 0.5)[0])
    ei, es = g.recommend_diverse_reps(np.zeros((0, d), np.float32), k, pool)
    assert ei.shape == (0, k) and es.shape == (0, k)
    # a row whose squared norm overflows (2e19 in a column where every representation is zero: its score is its bias, finite) ...
    big = E.copy()
    big[123] = 0.0
    big[123, 0] = 2e19
    for where, b123 in (("outside", -100.0), ("inside", 100.0)):
        b2 = bias.copy()
        b2[123] = b123
        g2, o2 = _pair(items, 8, d, ModelKind.LSTM_NORMAL, big, b2)
        if where == "outside":  # ... outside every pool does not matter
            for metric in ("cosine", "dot"):
                got = g2.recommend_diverse_reps(reps, k, pool, 0.3, metric)
                assert 123 not in got[0]
            calm = big.copy()  # the expectation's table: the row is in no pool, and the oracle refuses its squared norm
            calm[123] = 0.0
            _same(g2.recommend_diverse_reps(reps, k, pool, 0.3), DiverseExpectation(calm, "cosine").rows(pool_from_reps(o2, items, reps, pool), k, 0.3))
        else:  # ... inside a pool fails the cosine call, and the call after it is not marked by it
            snap = params(g2)
            with pytest.raises(PredictionError.InvalidPredictionValue):
                g2.recommend_diverse_reps(reps, k, pool, 0.3)
            ok = g2.recommend_diverse_reps(reps, k, pool, 0.3, exclude=[[123]] * 12)
            assert 123 not in ok[0] and np.all(ok[0] != NO_ITEM)
            assert np.all(g2.recommend_diverse_reps(reps, k, pool, 0.3, "dot")[0][:, 0] == 123)  # its dot products are finite
            for a, b in zip(snap, params(g2)):
                assert np.array_equal(_bits(a), _bits(b))
    for a, b in zip(before, params(g)):
        assert np.array_equal(_bits(a), _bits(b))
    # a store is refused while it is stale
    store = g.sessions(4)
    store.append([0, 1], [[1, 2], [3]])
    assert store.recommend_diverse([0, 1], k, pool)[0].shape == (2, k)
    g.set_param(Param.ITEM_BIAS, bias)
    with pytest.raises(EngineError) as e:
        store.recommend_diverse([0, 1], k, pool)
    assert e.value.status == Status.INVALID_ARGUMENT
    store.reset()
    assert store.recommend_diverse([0, 1], k, pool)[0].shape == (2, k)
