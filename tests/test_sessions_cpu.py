"""CPU: the session store's calls exist at every layer — declared in include/sbr_hip.h, exported by the library, bound by the
loader, wrapped by engine.Sessions, reachable from both models and the C++ header — and refuse to run without a device (no CPU
fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sbr_rs_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sbr_sessions_create", "sbr_sessions_destroy", "sbr_sessions_capacity", "sbr_sessions_reset", "sbr_sessions_reset_all",
           "sbr_sessions_append", "sbr_sessions_lengths", "sbr_sessions_representations", "sbr_sessions_get_state",
           "sbr_sessions_set_state", "sbr_sessions_recommend", "sbr_sessions_score_candidates"]


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    return _lib.load()


def test_sessions_symbols_declared_exported_and_bound():
    L = _library()
    header = open(os.path.join(ROOT, "include", "sbr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "typedef struct sbr_sessions sbr_sessions;" in code
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.DECLARED_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None, name  # the loader gave it a signature
    assert L.sbr_sessions_destroy.restype is None
    assert L.sbr_abi_version() == _abi.ABI_VERSION


def test_sessions_source_is_part_of_the_build():
    from sbr_rs_amd import build

    assert "sbr_sessions.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "sbr_sessions.hip"))
    assert callable(build.build_sessions_tests)


def test_sessions_on_both_models_engine_and_cpp_header():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine

    for mod in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel, engine.Model):
        assert callable(getattr(mod, "sessions"))
    for name in ("append", "representations", "recommend", "score_candidates", "lengths", "reset", "state", "set_state", "close"):
        assert callable(getattr(engine.Sessions, name)), name
    hpp = open(os.path.join(ROOT, "include", "sbr.hpp")).read()
    assert "class Sessions" in hpp and "Sessions sessions(std::size_t capacity) const" in hpp


def test_items_argument_forms():
    from sbr_rs_amd.engine import _items_csr

    ptr, ids = _items_csr([[1, 2], [], [3]], 3)
    assert ptr.tolist() == [0, 2, 2, 3] and ids.tolist() == [1, 2, 3] and ptr.dtype == np.uint64 and ids.dtype == np.uint32
    ptr, ids = _items_csr((np.array([0, 1, 3]), np.array([7, 8, 9])), 2)
    assert ptr.tolist() == [0, 1, 3] and ids.tolist() == [7, 8, 9]
    ptr, ids = _items_csr([[], []], 2)
    assert ptr.tolist() == [0, 0, 0] and ids.size == 1  # never an empty buffer
    with pytest.raises(ValueError):
        _items_csr([[1]], 2)
    with pytest.raises(ValueError):
        _items_csr((np.array([0, 1]), np.array([7])), 2)


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device behaviour")
def test_sessions_without_device_fail_loudly():
    import sbr_rs_amd as sbr
    from sbr_rs_amd._abi import Status
    from sbr_rs_amd.errors import EngineError

    # a store needs a model and a model cannot exist without a device: the path to every call ends here
    for build in (lambda: sbr.ewma.Hyperparameters.new(50, 8).embedding_dim(16).build(),
                  lambda: sbr.lstm.Hyperparameters.new(50, 8).embedding_dim(16).build()):
        with pytest.raises(EngineError) as e:
            build().sessions(4)
        assert e.value.status == Status.NO_DEVICE
    # no model, no store, no answer: the entry points compute nothing on the host
    L = _library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = C.c_void_p()
    assert L.sbr_sessions_create(None, 4, C.byref(h)) == Status.INVALID_ARGUMENT and not h.value
    sl = np.array([0, 1], np.uint32)
    ptr = np.array([0, 1, 2], np.uint64)
    ids = np.array([1, 2], np.uint32)
    out = np.zeros(64, np.float32)
    oi = np.zeros(16, np.uint32)
    n64 = np.zeros(2, np.uint64)
    assert L.sbr_sessions_append(None, vp(sl), 2, vp(ptr), vp(ids)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_representations(None, vp(sl), 2, vp(out)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_recommend(None, vp(sl), 2, 5, None, None, 0, vp(oi), None) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_score_candidates(None, vp(sl), 2, vp(ptr), vp(ids), vp(out)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_lengths(None, vp(sl), 2, vp(n64)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_get_state(None, vp(sl), 2, vp(out), None, vp(n64)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_set_state(None, vp(sl), 2, vp(out), None, vp(n64)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_reset(None, vp(sl), 2) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_reset_all(None) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_capacity(None, n64.ctypes.data_as(C.POINTER(C.c_uint64))) == Status.INVALID_ARGUMENT
    L.sbr_sessions_destroy(None)  # a null store is ignored
