"""CPU: the five calls of the candidates family (user_representations, score_candidates[_reps], recommend_among[_reps]) exist
at every layer, refuse to run without a device (no CPU fallback), and the expectation the GPU tests use orders items as a float64
brute force restricted to the item set does."""
import ctypes as C
import os

import numpy as np
import pytest

from candidates_expect import AmongExpectation, planted_subset
from helpers import LOSS_HINGE, hparams
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ModelKind, Param

SYMBOLS = ["sbr_user_representations", "sbr_score_candidates", "sbr_score_candidates_reps", "sbr_recommend_among",
           "sbr_recommend_among_reps"]


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def test_candidates_symbols_declared_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sbr_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.DECLARED_SYMBOLS
        assert hasattr(L, name)
        assert f"sbr_status {name}(sbr_model* m" in header
    assert L.sbr_abi_version() == _lib.ABI_VERSION


def test_candidates_on_both_models_and_engine():
    import inspect

    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine

    for mod in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel):
        for name in ("user_representations", "score_candidates", "rerank", "recommend"):
            assert callable(getattr(mod, name))
        p = inspect.signature(mod.recommend).parameters
        assert p["among"].default is None and p["exclude_history"].default is True  # today's call is unchanged
        assert "host" in mod.rerank.__doc__
    for name in ("user_representations", "score_candidates", "score_candidates_reps", "recommend_among", "recommend_among_reps"):
        assert callable(getattr(engine.Model, name))


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device behaviour")
def test_candidates_without_device_fail_loudly():
    import sbr_rs_amd as sbr
    from sbr_rs_amd._abi import Status
    from sbr_rs_amd.errors import EngineError

    def model():  # a model cannot exist without a device: every path to the five calls ends here
        return sbr.ewma.Hyperparameters.new(50, 8).embedding_dim(16).build()

    hists, cands = [[1, 2, 3], [4]], [[5, 6], [7]]
    reps = np.zeros((2, 16), np.float32)
    cp = np.array([0, 2, 3], np.uint64)
    ci = np.array([5, 6, 7], np.uint32)
    calls = [lambda: model().user_representations(hists), lambda: model().score_candidates(hists, cands), lambda: model().rerank(hists, cands, 1),
             lambda: model().recommend(hists, 5, among=[1, 2, 3]), lambda: model().params.score_candidates_reps(reps, cp, ci),
             lambda: model().params.recommend_among_reps(reps, 5, [1, 2, 3])]
    for call in calls:
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.NO_DEVICE
    # no model, no answer: the entry points compute nothing on the host
    L = _lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    up = np.array([0, 3, 4], np.uint64)
    it = np.array([1, 2, 3, 4], np.uint32)
    out = np.zeros(64, np.float32)
    oi = np.zeros(16, np.uint32)
    assert L.sbr_user_representations(None, vp(up), vp(it), 2, vp(out)) == Status.INVALID_ARGUMENT
    assert L.sbr_score_candidates(None, vp(up), vp(it), 2, vp(cp), vp(ci), vp(out)) == Status.INVALID_ARGUMENT
    assert L.sbr_score_candidates_reps(None, vp(reps), 2, vp(cp), vp(ci), vp(out)) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_among(None, vp(up), vp(it), 2, 5, 0, vp(ci), 3, vp(oi), None) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_among_reps(None, vp(reps), 2, 5, None, None, vp(ci), 3, vp(oi), None) == Status.INVALID_ARGUMENT


@pytest.mark.parametrize("d,items", [(8, 300), (32, 500), (100, 400)])
def test_expectation_orders_as_float64_brute_force(d, items):
    """Well-separated data: where no two of a user's best k + 1 scores among S are closer than 1e-5, the f32 chain's error cannot
    change the order a float64 computation restricted to S gives (the rule of the similar_items expectation's test)."""
    rs = np.random.RandomState(d)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    bias = (rs.randn(items) * 0.5).astype(np.float32)
    o = OracleModel(hparams(items, 8, d, int(ModelKind.EWMA), LOSS_HINGE))
    o.set_param(Param.ITEM_EMBEDDING, E)
    o.set_param(Param.ITEM_BIAS, bias)
    reps = (rs.randn(6, d) * 0.3).astype(np.float32)
    want = AmongExpectation(o, items, reps)
    k = 20
    compared = 0
    for n in (25, items // 3, items):
        S = planted_subset(items, n, np.arange(0, 42, 2, dtype=np.uint32), n)
        excl = [rs.choice(S, 3, replace=False) for _ in reps]
        gi, gs = want.rows(S, k, exclude=excl)
        for u, r in enumerate(reps):
            s64 = bias.astype(np.float64) + E.astype(np.float64) @ r.astype(np.float64)
            ids = np.setdiff1d(S.astype(np.int64), excl[u])
            order = ids[np.lexsort((ids, -s64[ids]))]
            if np.all(np.abs(np.diff(s64[order][: k + 1])) > 1e-5):
                assert gi[u].tolist() == order[:k].tolist()
                compared += 1
            real = gi[u] != NO_ITEM
            assert np.allclose(gs[u][real], s64[gi[u][real]], rtol=0, atol=1e-5)
            assert set(gi[u][real].tolist()) <= set(ids.tolist())
    assert compared >= 9  # of 18 rows
    # fewer eligible items than k: padding
    pi, ps = want.rows(S[:5], k)
    assert np.all(pi[:, 5:] == NO_ITEM) and np.all(np.isneginf(ps[:, 5:])) and np.all(pi[:, :5] != NO_ITEM)
