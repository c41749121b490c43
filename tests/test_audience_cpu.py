"""CPU: the audience scan (which rows for this item) exists at every layer — declared in include/sbr_hip.h, exported by the library,
bound by the loader, wrapped by engine.Model / engine.Sessions, reachable from both models and the C++ header — its argument
refusals come before any call into the library, and the plain-numpy reference of its rows (tests/audience_expect.py) agrees with a
sort written from the definition, ties and signed zeros included."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import audience_expect as ae
from seen_expect import SeenModel
from sbr_rs_amd import _abi, _lib
from sbr_rs_amd._abi import Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sbr_audience_reps", "sbr_audience", "sbr_sessions_audience"]


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    return _lib.load()


def test_audience_symbols_declared_exported_and_bound():
    L = _library()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbr_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.DECLARED_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    # additions only: the ABI version stays what it was
    m = re.search(r"#define\s+SBR_ABI_VERSION\s+(\d+)u", code)
    assert int(m.group(1)) == L.sbr_abi_version() == _abi.ABI_VERSION == 13


def test_python_and_cpp_surfaces():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import build, engine

    p = inspect.signature(engine.Sessions.audience).parameters
    assert list(p) == ["self", "items", "k", "slots", "exclude", "include_seen"]
    assert p["slots"].default is None and p["exclude"].default is None and p["include_seen"].default is False
    p = inspect.signature(engine.Model.audience_reps).parameters
    assert list(p) == ["self", "reps", "items", "k", "exclude"] and p["exclude"].default is None
    for cls in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel):
        p = inspect.signature(cls.audience).parameters
        assert list(p) == ["self", "interactions_or_histories", "items", "k", "exclude_history"], cls
        assert p["exclude_history"].default is True
    hpp = open(os.path.join(ROOT, "include", "sbr.hpp")).read()
    for text in ("Result<Recommendations, PredictionError> audience(const std::vector<std::uint32_t>& items, std::size_t k,",
                 "Result<Recommendations, PredictionError> audience_reps(const std::vector<float>& reps, const std::vector<ItemId>& items,",
                 "Result<Recommendations, PredictionError> audience(const data::CompressedInteractions& histories,",
                 "sbr_sessions_audience(", "sbr_audience_reps(", "sbr_audience("):
        assert text in hpp, text
    assert callable(build.build_audience_tests) and os.path.exists(build.AUDIENCE_SRC)
    assert os.path.exists(os.path.join(ROOT, "tools", "time_audience.py"))


def _store_without_library(seen):
    from sbr_rs_amd.engine import Sessions

    class NoLibrary:  # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    st = Sessions.__new__(Sessions)
    st._seen, st._h, st._L = seen, None, NoLibrary()
    return st


def test_include_seen_without_memory_raises_before_the_library():
    with pytest.raises(ValueError):
        _store_without_library(0).audience([1, 2], 5, include_seen=True)


def test_k_out_of_range_and_duplicate_slots_are_refused():
    st = _store_without_library(8)
    for k in (0, -1, 1025):
        with pytest.raises(ValueError):
            st.audience([1, 2], k)
    with pytest.raises(ValueError):
        st.audience([1, 2], 5, slots=[3, 4, 3])
    with pytest.raises(ValueError):
        st.audience([1, 2], 5, exclude=[[1]])  # one list per query
    # the C entry points refuse before they touch anything: no model, no store, no answer
    L = _library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(10, 7, np.uint32)
    q = np.array([1, 2], np.uint32)
    ptr = np.array([0, 0], np.uint64)
    reps = np.zeros(16, np.float32)
    assert L.sbr_audience_reps(None, vp(reps), 1, vp(q), 2, 5, None, None, vp(out), None) == Status.INVALID_ARGUMENT
    assert L.sbr_audience(None, vp(ptr), None, 1, vp(q), 2, 5, 0, vp(out), None) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_audience(None, vp(q), 2, 5, None, 0, None, None, 0, vp(out), None) == Status.INVALID_ARGUMENT
    assert np.all(out == 7)


# ---- the reference against the definition -------------------------------------------------------------------------------------
def _tied_scores(rs, nq, ns):
    """scores from a handful of values, so that most pairs tie, with both zeros among them"""
    values = np.array([0.0, -0.0, 1.5, -2.25, 1.5, 3.0e-39, -0.0], dtype=np.float32)  # a denormal too
    return values[rs.randint(0, values.size, size=(nq, ns))].view(np.uint32)


@pytest.mark.parametrize("seed", range(4))
def test_expectation_agrees_with_brute_force_on_ties(seed):
    rs = np.random.RandomState(seed)
    nq, ns = 7, 23
    bits = _tied_scores(rs, nq, ns)
    ids = rs.permutation(100)[:ns].astype(np.uint32)  # ids in no order: the tie rule is about ids, not positions
    exclude = [rs.choice(ids, size=rs.randint(0, 6), replace=False) for _ in range(nq)]
    for k in (1, 5, ns, ns + 4):
        for ex in (None, exclude):
            got = ae.expected_rows(bits, ids, k, ex)
            want = ae.brute_force_rows(bits, ids, k, ex)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, ex is None)


def test_signed_zeros_tie_and_keep_their_bits():
    neg, pos = np.float32(-0.0).view(np.uint32), np.float32(0.0).view(np.uint32)
    bits = np.array([[pos, neg, pos, neg]], dtype=np.uint32)
    rows, out = ae.expected_rows(bits, [9, 3, 5, 7], 4)
    assert rows.tolist() == [[3, 5, 7, 9]]
    assert out.tolist() == [[neg, pos, neg, pos]]
    rows, out = ae.expected_rows(bits, [9, 3, 5, 7], 6, exclude=[[5, 1000]])
    assert rows.tolist() == [[3, 7, 9, ae.NO_ROW, ae.NO_ROW, ae.NO_ROW]]
    assert out[0, 3:].view(np.float32).tolist() == [-np.inf] * 3


def test_seen_rule_last_w_repeats_once_and_candidates_only():
    s = SeenModel(6, 3)
    s.append([0, 1, 2, 4], [[5, 6, 7, 8], [7, 7, 7], [], [8, 5]])  # slot 0 forgot item 5; slot 1 holds 7 three times
    got = ae.seen_excluded(s, [0, 1, 2, 3], [5, 7, 8, 7])
    assert got == [set(), {0, 1}, {0}, {0, 1}]  # slot 4 holds 5 and 8 but is no candidate
    assert ae.unite(got, [[2], [], [1], []]) == [{2}, {0, 1}, {0, 1}, {0, 1}]
    assert ae.unite(None, got) is got and ae.unite(got, None) is got


def test_cpp_program_builds_without_a_device():
    from sbr_rs_amd import build as hip_build

    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_audience_tests(verbose=False))
