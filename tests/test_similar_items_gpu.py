"""GPU: sbr_similar_items (exact top-k cosine / dot-product neighbours of catalogue items, sbr_catalogue.hip) against the
contract's formulas evaluated with the oracle's chain (similar_expect.py).  Items and score bits must be equal."""
import ctypes as C

import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams
from recommend_expect import NO_ITEM
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, PredictionError
from similar_expect import SimilarExpectation

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    gi, gs = got
    wi, ws = want
    assert gi.shape == wi.shape, (gi.shape, wi.shape)
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{len(bad)} items differ; first at {bad[0]}: {gi[tuple(bad[0])]} vs {wi[tuple(bad[0])]}"
    assert np.array_equal(_bits(gs), _bits(ws))


def _model(E, kind=ModelKind.EWMA, bias=None):
    items, d = E.shape
    g = Model(hparams(items, 8, d, int(kind), LOSS_HINGE, B=8))
    g.set_param(Param.ITEM_EMBEDDING, E)
    if bias is not None:
        g.set_param(Param.ITEM_BIAS, bias)
    return g


def _planted_table(items, d, seed):
    """0.3 * randn with, all in one table: 20 rows copied from row 0 (exact ties, lower id first), row 5 zero, row 7 = 2 x row 3
    (cosine 1 with it, or a rounding away), row 9 = -row 3."""
    rs = np.random.RandomState(seed)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    E[rs.choice(np.arange(10, items), 20, replace=False)] = E[0]
    E[5] = 0.0
    E[7] = 2.0 * E[3]
    E[9] = -E[3]
    return E


def _queries(items, seed, n=40):
    """n queries that include 0, 3, 5, items - 1 and a repeated id"""
    rs = np.random.RandomState(seed)
    return np.concatenate([[0, 3, 5, items - 1, 3], rs.randint(0, items, n - 5)]).astype(np.uint32)


_SHAPES = [(1, 300), (16, 1500), (32, 5000), (64, 900), (100, 2000), (128, 700), (256, 3000)]


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("d,items", _SHAPES)
def test_similar_items_matches_expectation(d, items, metric):
    E = _planted_table(items, d, d + items)
    g = _model(E)
    want = SimilarExpectation(E, metric)
    q = _queries(items, d)
    for k in (1, 10, 100, min(1024, items)):
        _same(g.similar_items(q, k, metric=metric), want.rows(q, k))
    if metric == "cosine":  # the planted rows do what the contract says
        gi, gs = g.similar_items(q, 10)
        assert np.all(gs[2] == 0.0) and gi[2].tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]  # the zero row: every score a tie at 0
        i3, s3 = g.similar_items([3], min(1024, items))
        s3 = dict(zip(i3[0].tolist(), s3[0].tolist()))
        assert abs(s3[7] - 1.0) < 1e-6
        if 5 in s3:
            assert s3[5] == 0.0
        if 9 in s3:
            assert abs(s3[9] + 1.0) < 1e-6


@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA])
def test_similar_items_on_both_models(kind):
    """The item table is shared code: one LSTM and one EWMA model through the public wrappers."""
    import sbr_rs_amd as sbr

    items, d, k = 700, 24, 20
    E = _planted_table(items, d, 11)
    g = _model(E, kind)
    w = (sbr.lstm.ImplicitLSTMModel if kind == ModelKind.LSTM_NORMAL else sbr.ewma.ImplicitEWMAModel)(g)
    q = _queries(items, 2)
    for metric in ("cosine", "dot"):
        _same(w.similar_items(q, k, metric=metric), SimilarExpectation(E, metric).rows(q, k))


def test_similar_items_self_exclusion_and_padding():
    items, d, k = 400, 16, 10
    E = _planted_table(items, d, 1)
    g = _model(E)
    want = SimilarExpectation(E, "cosine")
    q = _queries(items, 3)
    gi, gs = g.similar_items(q, k)
    _same((gi, gs), want.rows(q, k))
    for j, qq in enumerate(q):
        assert int(qq) not in gi[j].tolist()
    inc = g.similar_items(q, k, include_self=True)
    _same(inc, want.rows(q, k, include_self=True))
    # per-query exclusion lists: unsorted, with duplicates, and leaving 3 eligible items (the query is not one of them)
    rs = np.random.RandomState(4)
    excl = []
    for qq in q:
        keep = rs.choice(np.setdiff1d(np.arange(items), [qq]), 3, replace=False)
        ex = np.setdiff1d(np.arange(items), np.concatenate([keep, [qq]]))
        ex = np.concatenate([ex, ex[:17]])
        rs.shuffle(ex)
        excl.append(ex.astype(np.uint32))
    for self_too in (False, True):
        xi, xs = g.similar_items(q, k, include_self=self_too, exclude=excl)
        _same((xi, xs), want.rows(q, k, include_self=self_too, exclude=excl))
        n = 4 if self_too else 3
        assert np.all(xi[:, n:] == NO_ITEM) and np.all(np.isneginf(xs[:, n:])) and np.all(xi[:, :n] != NO_ITEM)
    # an empty query list is a no-op
    ei, es = g.similar_items(np.zeros(0, np.uint32), k)
    assert ei.shape == (0, k) and es.shape == (0, k)


_MONOTONE = {}


def _monotone_case(direction):
    """60 000 items, d = 32, E[i] = (1e-3 * (i + 1), 0, ...) (ascending) — under the dot metric the score of item i is
    E[q][0] * E[i][0], strictly increasing in the id for every query (neighbouring entries differ by at least 1.6e-5 relative, far
    above an f32 rounding), so every scanned score is a candidate.  Descending: E[i] = (1e-3 * (items - i), 0, ...), the same
    values in the other order, so almost no score is (a sign flip of every row would leave the product of two rows, and so the
    order, as it was).  The expectation is computed once per direction."""
    if direction not in _MONOTONE:
        items, d = 60_000, 32
        E = np.zeros((items, d), np.float32)
        ramp = np.arange(1, items + 1, dtype=np.float64) * 1e-3
        E[:, 0] = (ramp if direction > 0 else ramp[::-1]).astype(np.float32)
        q = np.random.RandomState(6).randint(0, items, 160).astype(np.uint32)
        _MONOTONE[direction] = (E, q, SimilarExpectation(E, "dot").rows(q, 1024))
    return _MONOTONE[direction]


@pytest.mark.parametrize("groups", ["1", "3"])
@pytest.mark.parametrize("direction", [1, -1])
def test_similar_items_long_ranges_full_lists(direction, groups, monkeypatch):
    """One long item range and three (SBR_CATALOGUE_GROUPS), k = 1024: full lists, staging merges, the merge of ranges."""
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", groups)
    E, q, want = _monotone_case(direction)
    g = _model(E)
    got = g.similar_items(q, 1024, metric="dot")
    _same(got, want)
    top = np.arange(E.shape[0] - 1, E.shape[0] - 1026, -1) if direction > 0 else np.arange(1025)
    for j in (0, 77, 159):
        assert got[0][j].tolist() == [i for i in top.tolist() if i != int(q[j])][:1024]


def test_similar_items_two_chunks():
    """8 192 + 40 queries: the second launch's queries (c0 != 0) land in the right rows."""
    items, d, k = 300, 16, 10
    E = _planted_table(items, d, 8)
    g = _model(E)
    q = np.random.RandomState(9).randint(0, items, 8192 + 40).astype(np.uint32)
    _same(g.similar_items(q, k), SimilarExpectation(E, "cosine").rows(q, k))


@pytest.mark.parametrize("d,items", [(16, 1500), (100, 2000), (256, 3000)])
def test_similar_items_dot_equals_recommend_reps(d, items):
    """No oracle: on a model whose bias is zero, the dot metric with the query included is recommend_reps of the query rows."""
    E = _planted_table(items, d, 5)
    g = _model(E, bias=np.zeros(items, np.float32))
    q = _queries(items, 7)
    for k in (1, 100, min(1024, items)):
        _same(g.similar_items(q, k, metric="dot", include_self=True), g.recommend_reps(E[q], k))


def test_similar_items_errors():
    items, d, k = 500, 32, 10
    E = _planted_table(items, d, 3)
    q = _queries(items, 1)
    # a row whose squared norm overflows: the cosine of anything is undefined
    big = E.copy()
    big[123] = 3e19
    g = _model(big)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.similar_items(q, k)
    # two rows whose dot product overflows, one of them a query
    two = E.copy()
    two[200] = 0.0
    two[300] = 0.0
    two[200, 0] = two[300, 0] = 1e20
    g = _model(two)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.similar_items(np.array([4, 200], np.uint32), k, metric="dot")
    # ... and the flag does not outlive the call: queries that meet only finite products get their answer
    _same(g.similar_items(q, k, metric="dot"), SimilarExpectation(two, "dot").rows(q, k))
    g = _model(E)
    for kwargs in (dict(query_items=[items], k=k), dict(query_items=q, k=0), dict(query_items=q, k=1025),
                   dict(query_items=q, k=k, metric=2), dict(query_items=q, k=k, exclude=[[items]] + [[]] * (len(q) - 1))):
        with pytest.raises(EngineError) as e:
            g.similar_items(**kwargs)
        assert e.value.status == Status.INVALID_ARGUMENT
    out = np.zeros((len(q), k), np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert g._L.sbr_similar_items(g._h, vp(q), len(q), k, 0, 2, None, None, vp(out), None) == Status.INVALID_ARGUMENT
    assert g._L.sbr_similar_items(g._h, vp(q), len(q), k, 0, 0, None, None, vp(out), None) == Status.OK  # scores are optional
    assert np.array_equal(out, g.similar_items(q, k)[0])
    with pytest.raises(ValueError):
        g.similar_items(q, k, metric="euclid")


def test_similar_items_reads_parameters_only():
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
    for metric in ("cosine", "dot"):
        g.similar_items(_queries(items, 5), k, metric=metric)
    after, rec_after = snapshot()
    assert len(before) == len(after) and len(before) >= 6
    for a, b in zip(before, after):
        assert np.array_equal(_bits(a), _bits(b))
    _same(rec_after, rec_before)
