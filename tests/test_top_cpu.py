"""CPU: the budget form of the scans (the exact best n of a row, any n) exists at every layer — declared in include/sbr_hip.h,
exported by the library, bound by the loader, wrapped by engine.Model / engine.Sessions, reachable from both models and the C++
header — its argument refusals come before any call into the library, and the numpy restatement the GPU tests compare against
(tests/top_expect.py) agrees with a selection written from the definition on heavily tied scores.  No device is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from sbr_rs_amd import _abi, _lib, engine, lstm
from sbr_rs_amd._abi import Status
from top_expect import key_of, top_expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sbr_recommend_top", "sbr_recommend_top_reps", "sbr_sessions_recommend_top", "sbr_audience_top_reps", "sbr_audience_top",
           "sbr_sessions_audience_top"]


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    return _lib.load()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_top_symbols_declared_exported_and_bound():
    L = _library()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbr_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.DECLARED_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
        # the sibling's list with out_cuts added: one argument more
        assert len(fn.argtypes) == len(getattr(L, name.replace("_top", "_above")).argtypes) + 1, name
    m = re.search(r"#define\s+SBR_ABI_VERSION\s+(\d+)u", code)
    assert int(m.group(1)) == L.sbr_abi_version() == _abi.ABI_VERSION == 13  # additions only


def _params(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_python_and_cpp_surfaces():
    from sbr_rs_amd import build

    E = inspect.Parameter.empty
    assert _params(engine.Model.recommend_top) == {"user_ptr": E, "item_ids": E, "n": E, "include_history": False, "any_of": None,
                                                   "none_of": None, "max_results": None, "order": "score"}
    assert _params(engine.Model.recommend_top_reps) == {"reps": E, "n": E, "exclude": None, "any_of": None, "none_of": None,
                                                        "max_results": None, "order": "score"}
    assert _params(engine.Model.audience_top) == {"user_ptr": E, "item_ids": E, "items": E, "n": E, "include_history": False,
                                                  "max_results": None, "order": "score"}
    assert _params(engine.Model.audience_top_reps) == {"reps": E, "items": E, "n": E, "exclude": None, "max_results": None, "order": "score"}
    assert _params(engine.Sessions.recommend_top) == {"slots": E, "n": E, "exclude": None, "any_of": None, "none_of": None,
                                                      "include_seen": False, "max_results": None, "order": "score"}
    assert _params(engine.Sessions.audience_top) == {"items": E, "n": E, "slots": None, "exclude": None, "include_seen": False,
                                                     "max_results": None, "order": "score"}
    # an nth_score form beside each, with the same leading arguments and neither max_results nor order
    for owner, name, nth in ((engine.Model, "recommend_top", "nth_score"), (engine.Model, "recommend_top_reps", "nth_score_reps"),
                             (engine.Model, "audience_top", "nth_audience_score"), (engine.Model, "audience_top_reps", "nth_audience_score_reps"),
                             (engine.Sessions, "recommend_top", "nth_score"), (engine.Sessions, "audience_top", "nth_audience_score")):
        full = _params(getattr(owner, name))
        assert _params(getattr(owner, nth)) == {k: v for k, v in full.items() if k not in ("max_results", "order")}, nth
    M = lstm._ImplicitSequenceModel
    assert _params(M.recommend_top) == {"interactions_or_histories": E, "n": E, "exclude_history": True, "any_of": None, "none_of": None,
                                        "max_results": None, "order": "score"}
    assert _params(M.audience_top) == {"interactions_or_histories": E, "items": E, "n": E, "exclude_history": True, "max_results": None,
                                       "order": "score"}
    assert _params(M.recommend_top_reps) == _params(engine.Model.recommend_top_reps)
    assert _params(M.audience_top_reps) == _params(engine.Model.audience_top_reps)
    for name in ("nth_score", "nth_score_reps", "nth_audience_score", "nth_audience_score_reps"):
        assert callable(getattr(M, name))
    # the result object: the existing Above, `cuts` None unless a *_top call set it
    a = engine.Above(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    assert a.cuts is None and engine.Above(a.ptr, a.ids, a.scores, "id", np.zeros(0, np.float32)).cuts is not None
    hpp = open(os.path.join(ROOT, "include", "sbr.hpp")).read()
    for text in ("Result<Above, PredictionError> recommend_top(const data::CompressedInteractions& interactions, const std::vector<std::uint64_t>& n,",
                 "Result<Above, PredictionError> recommend_top_reps(const std::vector<float>& reps, const std::vector<std::uint64_t>& n,",
                 "Result<Above, PredictionError> audience_top(const data::CompressedInteractions& histories, const std::vector<ItemId>& items,",
                 "Result<Above, PredictionError> audience_top_reps(const std::vector<float>& reps, const std::vector<ItemId>& items,",
                 "Result<Above, PredictionError> recommend_top(const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& n,",
                 "Result<Above, PredictionError> audience_top(const std::vector<std::uint32_t>& items, const std::vector<std::uint64_t>& n,",
                 "std::vector<float> cuts;", "sbr_recommend_top(", "sbr_recommend_top_reps(", "sbr_sessions_recommend_top(",
                 "sbr_audience_top_reps(", "sbr_audience_top(", "sbr_sessions_audience_top("):
        assert text in hpp, text
    assert callable(build.build_top_tests) and os.path.exists(build.TOP_SRC)


class NoLibrary:  # any call into the library fails the test
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def _store_without_library(seen):
    st = engine.Sessions.__new__(engine.Sessions)
    st._seen, st._h, st._L = seen, None, NoLibrary()
    return st


def _model_without_library(dim=4):
    m = engine.Model.__new__(engine.Model)
    m._h, m._L, m.dim = None, NoLibrary(), dim
    return m


def test_refusals_come_before_the_library():
    from sbr_rs_amd.engine import _top_budgets

    assert _top_budgets(5, 3).tolist() == [5, 5, 5] and _top_budgets(5, 3).dtype == np.uint64
    assert _top_budgets([0, 1 << 40, 7], 3).tolist() == [0, 1 << 40, 7]
    assert _top_budgets(np.array([2.0, 3.0]), 2).tolist() == [2, 3]
    assert _top_budgets(1, 0).size == 1  # a valid pointer for an empty call
    assert _top_budgets(2.0 ** 63, 1).tolist() == [1 << 63] and _top_budgets(np.uint64(2 ** 64 - 1), 1).tolist() == [2 ** 64 - 1]
    for bad, rows in ((-1, 3), ([1, -2, 3], 3), (np.nan, 2), ([1.0, np.nan], 2), (1.5, 2), (np.inf, 2), ([1, 2], 3), ("7", 1), (1e30, 2),
                      (2.0 ** 64, 1), ([1.0, 2.0 ** 64], 2), (2 ** 64, 1)):
        with pytest.raises(ValueError):
            _top_budgets(bad, rows)
    m = _model_without_library()
    reps = np.zeros((3, 4), np.float32)
    ptr, it = np.array([0, 1, 2, 3], np.uint64), np.array([1, 2, 3], np.uint32)
    for bad in (-1, [1, 2], np.nan, [1, -1, 1]):
        with pytest.raises(ValueError):
            m.recommend_top_reps(reps, bad)
        with pytest.raises(ValueError):
            m.nth_score_reps(reps, bad)
        with pytest.raises(ValueError):
            m.recommend_top(ptr, it, bad)
        with pytest.raises(ValueError):
            m.audience_top_reps(reps, [1, 2, 3], bad)
        with pytest.raises(ValueError):
            m.audience_top(ptr, it, [1, 2, 3], bad)
    with pytest.raises(ValueError):
        m.recommend_top_reps(reps, 5, order="rank")
    with pytest.raises(ValueError):
        m.recommend_top_reps(reps, 5, max_results=-1)
    with pytest.raises(ValueError):
        m.recommend_top_reps(reps, 5, exclude=[[1]])  # one list per row
    with pytest.raises(ValueError):
        _store_without_library(0).recommend_top([1, 2], 5, include_seen=True)
    with pytest.raises(ValueError):
        _store_without_library(0).audience_top([1, 2], 5, include_seen=True)
    st = _store_without_library(8)
    with pytest.raises(ValueError):
        st.audience_top([1, 2], 5, slots=[3, 4, 3])
    with pytest.raises(ValueError):
        st.audience_top([1, 2], [5, 6, 7])
    with pytest.raises(ValueError):
        st.nth_audience_score([1, 2], -5)
    # the C entry points refuse before they touch anything: no model, no store, no answer
    L = _library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = np.array([3, 3], np.uint64)
    cuts, counts, total = np.full(2, 7, np.float32), np.full(2, 7, np.uint64), C.c_uint64(7)
    q = np.array([1, 2], np.uint32)
    uptr = np.array([0, 0, 0], np.uint64)
    reps2 = np.zeros(32, np.float32)
    tail = (vp(cuts), vp(counts), C.byref(total), 0, None, None)
    assert L.sbr_recommend_top(None, vp(uptr), None, 2, vp(n), 0, None, None, *tail) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_top_reps(None, vp(reps2), 2, vp(n), None, None, None, None, *tail) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_recommend_top(None, vp(q), 2, vp(n), None, None, 0, None, None, *tail) == Status.INVALID_ARGUMENT
    assert L.sbr_audience_top_reps(None, vp(reps2), 2, vp(q), 2, vp(n), None, None, *tail) == Status.INVALID_ARGUMENT
    assert L.sbr_audience_top(None, vp(uptr), None, 2, vp(q), 2, vp(n), 0, *tail) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_audience_top(None, vp(q), 2, vp(n), None, 0, None, None, 0, *tail) == Status.INVALID_ARGUMENT
    assert np.all(cuts == 7) and np.all(counts == 7) and total.value == 7


# ---- the expectation against the definition -------------------------------------------------------------------------------------
def test_key_map_is_monotone_and_zeros_tie():
    fmax = np.finfo(np.float32).max
    tiny = np.float32(1e-45)  # the smallest denormal
    v = np.array([-fmax, -3.5, -1.0, -1e-30, -tiny, 0.0, tiny, 3e-39, 1e-30, 1.0, 3.5, fmax], np.float32)
    k = key_of(v).astype(np.int64)
    assert np.all(np.diff(k) > 0)
    assert key_of(np.float32(-0.0))[0] == key_of(np.float32(0.0))[0] == 0x80000000
    assert key_of(-tiny)[0] == 0x7FFFFFFE and key_of(tiny)[0] == 0x80000001
    assert key_of(np.float32(-np.inf))[0] < key_of(-fmax)[0] and key_of(np.float32(np.inf))[0] > key_of(fmax)[0]
    rs = np.random.RandomState(0)
    a = rs.randint(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    a = a[np.isfinite(a)]
    order = np.argsort(key_of(a), kind="stable")
    assert np.all(np.diff(a[order].astype(np.float64)) >= 0)


def _brute(scores, n, excluded, allowed):
    """the contract as loops over single f32 values: pick the best remaining column n times"""
    ptr, ids, out, cuts = [0], [], [], []
    for r in range(scores.shape[0]):
        left = [c for c in range(scores.shape[1])
                if (allowed is None or allowed[r, c]) and (excluded is None or c not in set(int(x) for x in excluded[r]))]
        m = len(left)
        row = []
        while left and len(row) < n[r]:
            best = 0
            for j in range(1, len(left)):
                if scores[r, left[j]] > scores[r, left[best]] or (scores[r, left[j]] == scores[r, left[best]] and left[j] < left[best]):
                    best = j
            row.append(left.pop(best))
        cuts.append(np.inf if n[r] == 0 else -np.inf if m < n[r] else scores[r, row[-1]])
        ids += row
        out += [scores[r, c] for c in row]
        ptr.append(len(ids))
    return np.array(ptr, np.uint64), np.array(ids, np.uint32), np.array(out, np.float32), np.array(cuts, np.float32)


@pytest.mark.parametrize("seed", range(3))
def test_expectation_agrees_with_brute_force_on_ties(seed):
    """scores from a handful of values — both zeros and a denormal among them — so that most pairs tie and the cut falls inside a tie
    group; n below, at and past the number eligible, and 0"""
    rs = np.random.RandomState(seed)
    rows, cols = 8, 40
    values = np.array([0.0, -0.0, 1.5, -2.25, 1.5, 3.0e-39, -0.0, -3.0e-39], dtype=np.float32)
    scores = values[rs.randint(0, values.size, size=(rows, cols))]
    assert np.signbit(scores[scores == 0]).any() and not np.signbit(scores[scores == 0]).all()
    excluded = [rs.randint(0, cols, rs.randint(0, 12)) for _ in range(rows)]
    allowed = rs.rand(rows, cols) < 0.7
    for ex, al in ((None, None), (excluded, None), (None, allowed), (excluded, allowed)):
        m = np.ones((rows, cols), bool) if al is None else al.copy()
        if ex is not None:
            for r in range(rows):
                m[r, ex[r]] = False
        elig = m.sum(axis=1)
        n = np.array([0, 1, 7, elig[3] - 1, elig[4], elig[5] + 1, cols + 5, 13])
        got = top_expect(scores, n, ex, al, "score")
        want = _brute(scores, n, ex, al)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2]))
        assert np.array_equal(got[3], want[3]) and not np.signbit(got[3][got[3] == 0]).any()  # a zero cut is +0.0
        assert np.array_equal(np.diff(got[0]), np.minimum(n, elig).astype(np.uint64))
        assert got[3][0] == np.inf and got[3][5] == -np.inf and got[3][6] == -np.inf and np.isfinite(got[3][4])
        by_id = top_expect(scores, n, ex, al, "id")
        assert np.array_equal(by_id[0], got[0]) and np.array_equal(by_id[3], got[3])
        for r in range(rows):
            a, b = int(got[0][r]), int(got[0][r + 1])
            assert np.array_equal(by_id[1][a:b], np.sort(got[1][a:b])) and np.array_equal(scores[r, by_id[1][a:b]], by_id[2][a:b])
    scalar = top_expect(scores, 7)
    assert np.all(np.diff(scalar[0]) == 7)
    named = top_expect(scores, 7, ids=np.arange(cols) * 3 + 1)
    assert np.array_equal(named[1], scalar[1] * 3 + 1)


def test_cpp_program_builds_without_a_device():
    from sbr_rs_amd import build as hip_build

    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_top_tests(verbose=False))
