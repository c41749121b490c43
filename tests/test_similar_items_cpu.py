"""CPU: the similar_items surface exists at every layer, refuses to run without a device (no CPU fallback), and the expectation
the GPU tests use orders items as a float64 brute force does."""
import os

import numpy as np
import pytest

from recommend_expect import NO_ITEM
from sbr_rs_amd import _lib
from similar_expect import SimilarExpectation


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def test_similar_items_symbol_declared_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    L = _lib.load()
    assert "sbr_similar_items" in _lib.DECLARED_SYMBOLS
    assert hasattr(L, "sbr_similar_items")
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sbr_hip.h")).read()
    for name in ("SBR_SIMILAR_COSINE 0u", "SBR_SIMILAR_DOT 1u", "SBR_SIMILAR_INCLUDE_SELF 1u"):
        assert "#define " + name in header


def test_similar_items_on_both_models_and_engine():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine

    for mod in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel):
        assert callable(getattr(mod, "similar_items"))
    assert callable(engine.Model.similar_items)
    assert (engine.SIMILAR_COSINE, engine.SIMILAR_DOT, engine.SIMILAR_INCLUDE_SELF) == (0, 1, 1)


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device behaviour")
def test_similar_items_without_device_fails_loudly():
    import ctypes as C

    import sbr_rs_amd as sbr
    from sbr_rs_amd._abi import Status
    from sbr_rs_amd.errors import EngineError

    with pytest.raises(EngineError) as e:
        sbr.ewma.Hyperparameters.new(50, 8).embedding_dim(16).build().similar_items([1, 2, 3], 5)
    assert e.value.status == Status.NO_DEVICE
    # no model, no answer: the entry point computes nothing on the host
    q = np.array([1], np.uint32)
    out = np.zeros(5, np.uint32)
    L = _lib.load()
    assert L.sbr_similar_items(None, q.ctypes.data_as(C.c_void_p), 1, 5, 0, 0, None, None, out.ctypes.data_as(C.c_void_p), None) == Status.INVALID_ARGUMENT


@pytest.mark.parametrize("d,items", [(8, 300), (32, 500), (100, 400)])
def test_expectation_orders_as_float64_brute_force(d, items):
    """Well-separated data: where no two of a query's best k + 1 scores are closer than 1e-5, the f32 chain's 6e-7 cannot change
    the order a float64 computation gives."""
    rs = np.random.RandomState(d)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    E[5] = 0.0
    queries = [0, 3, 5, items - 1, 3]
    k = 20
    E64 = E.astype(np.float64)
    n = np.sqrt((E64 * E64).sum(1))
    rn = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)
    compared = 0
    for metric in ("cosine", "dot"):
        want = SimilarExpectation(E, metric)
        items_got, scores_got = want.rows(queries, k)
        for j, q in enumerate(queries):
            s64 = (E64 @ E64[q]) * (rn * rn[q] if metric == "cosine" else 1.0)
            ids = np.array([i for i in range(items) if i != q])
            order = ids[np.lexsort((ids, -s64[ids]))]
            gaps = np.abs(np.diff(s64[order][: k + 1]))
            if np.all(gaps > 1e-5):
                assert items_got[j].tolist() == order[:k].tolist()
                compared += 1
            assert np.allclose(scores_got[j], s64[items_got[j]], rtol=0, atol=2e-6 if metric == "cosine" else 1e-5)
    assert compared >= 6  # of 10 rows; the zero row's two are all ties
    # the zero row: similarity 0 with everything, ids ascending; a duplicate pair ties to the lower id
    zi, zs = SimilarExpectation(E, "cosine").rows([5], 4)
    assert zi[0].tolist() == [0, 1, 2, 3] and np.all(zs == 0.0)
    E[11] = E[2]
    di, _ = SimilarExpectation(E, "cosine").rows([20], items + 3)
    row = di[0].tolist()
    assert row.index(2) + 1 == row.index(11) and row[-4:] == [NO_ITEM] * 4 and 20 not in row
