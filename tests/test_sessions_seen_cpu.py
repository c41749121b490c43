"""CPU: the seen-item memory of the session store exists at every layer — declared in include/sbr_hip.h, exported by the library,
bound by the loader, wrapped by engine.Sessions, reachable from both models and the C++ header — the ABI version agrees in the
header, the library and the loader, and the plain-Python model of the memory (tests/seen_expect.py) follows the rules it is the
reference for."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from seen_expect import SeenModel
from sbr_rs_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sbr_sessions_create_seen", "sbr_sessions_seen_capacity", "sbr_sessions_get_seen", "sbr_sessions_set_seen"]


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbr_hip.h")).read(), flags=re.S)


def test_seen_symbols_declared_exported_and_bound():
    L = _library()
    code = _header()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.DECLARED_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert re.search(r"#define\s+SBR_SESSIONS_MAX_SEEN\s+1024u", code)


def test_abi_version_agrees_in_header_library_and_loader():
    L = _library()
    m = re.search(r"#define\s+SBR_ABI_VERSION\s+(\d+)u", _header())
    assert m, "the header states the version"
    assert int(m.group(1)) == L.sbr_abi_version() == _abi.ABI_VERSION == 13


def test_python_and_cpp_surfaces():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import build, engine

    for mod in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel, engine.Model):
        p = inspect.signature(mod.sessions).parameters
        assert "remember" in p and p["remember"].default == 0, mod
    assert isinstance(engine.Sessions.seen_capacity, property)
    for name in ("seen", "set_seen"):
        assert callable(getattr(engine.Sessions, name)), name
    p = inspect.signature(engine.Sessions.recommend).parameters
    assert p["include_seen"].default is False
    assert "include_seen" not in inspect.signature(engine.Sessions.recommend_diverse).parameters  # the diverse calls always exclude
    hpp = open(os.path.join(ROOT, "include", "sbr.hpp")).read()
    for text in ("Sessions sessions(std::size_t capacity, std::size_t seen_capacity) const", "std::size_t seen_capacity() const",
                 "Seen seen(const std::vector<std::uint32_t>& slots) const", "void set_seen(", "bool include_seen = false",
                 "sbr_sessions_create_seen(", "sbr_sessions_get_seen(", "sbr_sessions_set_seen("):
        assert text in hpp, text
    assert callable(build.build_sessions_seen_tests)
    assert os.path.exists(build.SESSIONS_SEEN_SRC)


def test_include_seen_without_memory_raises():
    from sbr_rs_amd.engine import Sessions

    st = Sessions.__new__(Sessions)  # no device here: the refusal comes before any call into the library
    st._seen = 0
    st._h = None
    with pytest.raises(ValueError):
        st.recommend([0], 5, include_seen=True)


def test_remember_out_of_range_raises_before_the_library():
    from sbr_rs_amd.engine import Sessions

    for w in (-1, 1025):
        with pytest.raises(ValueError):
            Sessions(None, 4, remember=w)


def test_null_store_is_refused():
    L = _library()
    from sbr_rs_amd._abi import Status

    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = C.c_void_p()
    assert L.sbr_sessions_create_seen(None, 4, 8, C.byref(h)) == Status.INVALID_ARGUMENT and not h.value
    sl, ptr, ids = np.array([0, 1], np.uint32), np.array([0, 1, 2], np.uint64), np.array([1, 2], np.uint32)
    w = C.c_uint32()
    assert L.sbr_sessions_seen_capacity(None, C.byref(w)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_get_seen(None, vp(sl), 2, vp(ptr), vp(ids)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_set_seen(None, vp(sl), 2, vp(ptr), vp(ids)) == Status.INVALID_ARGUMENT


# ---- the ring model's own unit cases ------------------------------------------------------------------------------------------
def lists(model, slots):
    return [a.tolist() for a in model.seen(slots)]


def test_model_wraps_and_keeps_append_order():
    s = SeenModel(3, 4)
    s.append([0, 2], [[1, 2, 3], [9]])
    s.append([0], [[4, 5]])  # five items into a memory of four: the oldest goes
    assert lists(s, [0, 1, 2]) == [[2, 3, 4, 5], [], [9]]
    for x in (6, 7, 8, 9, 10):
        s.append([0], [[x]])
    assert lists(s, [0]) == [[7, 8, 9, 10]]


def test_model_more_than_w_in_one_call_keeps_the_last_w():
    s = SeenModel(2, 3)
    s.append([1], [list(range(10))])  # 3 W + 1
    assert lists(s, [1]) == [[7, 8, 9]]
    s.append([1], [[]])
    assert lists(s, [1]) == [[7, 8, 9]]


def test_model_keeps_duplicates():
    s = SeenModel(1, 5)
    s.append([0], [[4] * 7])
    assert lists(s, [0]) == [[4] * 5]
    s.append([0], [[2, 4]])
    assert lists(s, [0]) == [[4, 4, 4, 2, 4]]


def test_model_reset_set_state_and_set_seen():
    s = SeenModel(4, 3)
    s.append([0, 1, 2], [[1], [2, 3], [4, 5, 6, 7]])
    s.reset([1])
    assert lists(s, [0, 1, 2]) == [[1], [], [5, 6, 7]]
    s.set_state([2])
    assert lists(s, [2]) == [[]]
    s.set_seen([2, 3], [[5, 6, 7, 8, 9], [1]])  # the last W of the given list
    assert lists(s, [2, 3]) == [[7, 8, 9], [1]]
    s.append([2], [[3]])
    assert lists(s, [2]) == [[8, 9, 3]]
    s.reset()
    assert lists(s, [0, 1, 2, 3]) == [[], [], [], []]
    assert [a.tolist() for a in s.excluded([0], [[5, 5]])] == [[5, 5]]
    with pytest.raises(ValueError):
        s.append([0, 0], [[1], [2]])
    with pytest.raises(ValueError):
        s.seen([4])
