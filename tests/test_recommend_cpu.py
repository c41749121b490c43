"""CPU: the top-k recommendation surface exists at every layer, refuses to run without a device (no CPU fallback), and the
numpy expectation the GPU tests use agrees with a brute-force sort."""
import functools
import os

import numpy as np
import pytest

from recommend_expect import NO_ITEM, topk_expectation
from sbr_rs_amd import _lib


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def test_recommend_symbols_declared_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    L = _lib.load()
    for name in ("sbr_recommend", "sbr_recommend_reps"):
        assert name in _lib.DECLARED_SYMBOLS
        assert hasattr(L, name)


def test_recommend_on_both_models_and_engine():
    import sbr_rs_amd as sbr
    from sbr_rs_amd.engine import Model

    for mod in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel):
        assert callable(getattr(mod, "recommend"))
    assert callable(Model.recommend) and callable(Model.recommend_reps)


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device behaviour")
def test_recommend_without_device_fails_loudly():
    import ctypes as C

    import sbr_rs_amd as sbr
    from sbr_rs_amd._abi import Status
    from sbr_rs_amd.errors import EngineError

    with pytest.raises(EngineError) as e:
        sbr.lstm.Hyperparameters.new(50, 8).embedding_dim(16).build().recommend([[1, 2, 3]], 5)
    assert e.value.status == Status.NO_DEVICE
    # no model, no answer: the entry points compute nothing on the host
    out = np.zeros(5, np.uint32)
    ptr = np.array([0, 0], np.uint64)
    L = _lib.load()
    assert L.sbr_recommend(None, ptr.ctypes.data_as(C.c_void_p), None, 1, 5, 0, out.ctypes.data_as(C.c_void_p), None) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_reps(None, None, 1, 5, None, None, out.ctypes.data_as(C.c_void_p), None) == Status.INVALID_ARGUMENT


def _brute(scores, excluded, k):
    ex = set(int(x) for x in excluded)

    def cmp(a, b):  # (score desc, id asc); -0.0 == +0.0
        if scores[a] != scores[b]:
            return -1 if scores[a] > scores[b] else 1
        return -1 if a < b else 1

    order = sorted((i for i in range(len(scores)) if i not in ex), key=functools.cmp_to_key(cmp))[:k]
    items = [int(i) for i in order] + [NO_ITEM] * (k - len(order))
    sc = [float(scores[i]) for i in order] + [-np.inf] * (k - len(order))
    return np.array(items, np.uint32), np.array(sc, np.float32)


@pytest.mark.parametrize("seed", range(12))
def test_expectation_matches_brute_force(seed):
    rs = np.random.RandomState(seed)
    n = int(rs.randint(1, 60))
    scores = np.round(rs.randn(n), 1).astype(np.float32)  # many exact ties
    scores[rs.rand(n) < 0.2] = 0.0
    scores[rs.rand(n) < 0.2] = -0.0
    excluded = rs.randint(0, n, rs.randint(0, n + 1))
    for k in (1, 3, n, n + 5):
        ei, es = topk_expectation(scores, excluded, k)
        bi, bs = _brute(scores, excluded, k)
        assert np.array_equal(ei, bi)
        assert np.array_equal(es, bs)  # -0.0 == +0.0 here; the bits are those of the chosen items' scores


def test_expectation_all_ties_and_padding():
    scores = np.full(10, 0.5, np.float32)
    items, sc = topk_expectation(scores, [0, 3, 3], 9)
    assert items.tolist() == [1, 2, 4, 5, 6, 7, 8, 9, NO_ITEM]
    assert sc[-1] == -np.inf and np.all(sc[:-1] == 0.5)
