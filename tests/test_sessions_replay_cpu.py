"""CPU: replay and save / load of the session store exist at every layer — sbr_sessions_replay declared in include/sbr_hip.h, bound
by the loader with its four-argument signature (tests/test_abi.py checks the export), wrapped by engine.Sessions, reachable from
both models and the C++ header — a NULL store is refused, and the host halves of the store file (persistence.sessions_file_arrays
/ sessions_file_chunks), which touch no device, round-trip synthetic arrays."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from sbr_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    return _lib.load()


def test_replay_declared_and_bound_with_four_arguments():
    L = _library()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbr_hip.h")).read(), flags=re.S)
    assert re.search(r"sbr_status\s+sbr_sessions_replay\s*\(\s*sbr_sessions\s*\*\s*st\s*,\s*const\s+uint32_t\s*\*\s*slots\s*,\s*uint64_t\s+n\s*,"
                     r"\s*uint64_t\s*\*\s*out_replayed\s*\)\s*;", code)
    assert "sbr_sessions_replay" in _lib.DECLARED_SYMBOLS
    fn = L.sbr_sessions_replay
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]


def test_null_store_is_refused():
    from sbr_rs_amd._abi import Status

    L = _library()
    n = C.c_uint64(7)
    sl = np.array([0, 1], np.uint32)
    assert L.sbr_sessions_replay(None, None, 0, C.byref(n)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_replay(None, sl.ctypes.data_as(C.c_void_p), 2, None) == Status.INVALID_ARGUMENT
    assert n.value == 7


def test_python_and_cpp_surfaces():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import build, engine, persistence

    assert inspect.signature(engine.Sessions.replay).parameters["slots"].default is None
    assert callable(engine.Sessions.save)
    assert "replay()" in engine.Sessions.__doc__ and "reset()" in engine.Sessions.__doc__
    for mod in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel, engine.Model):
        p = inspect.signature(mod.load_sessions).parameters
        assert p["capacity"].default is None and p["remember"].default is None and p["replay"].default is False, mod
    p = inspect.signature(persistence.load_sessions).parameters
    assert list(p) == ["model", "path", "capacity", "remember", "replay"]
    assert list(inspect.signature(persistence.save_sessions).parameters) == ["store", "path"]
    assert persistence.SESSIONS_CHUNK == 65536
    hpp = open(os.path.join(ROOT, "include", "sbr.hpp")).read()
    for text in ("std::size_t replay()", "std::size_t replay(const std::vector<std::uint32_t>& slots)", "sbr_sessions_replay("):
        assert text in hpp, text
    assert callable(build.build_sessions_replay_tests) and os.path.exists(build.SESSIONS_REPLAY_SRC)


def _synthetic(kind, dim, n, w, seed):
    """what Sessions.state / seen return for slots 0 .. n - 1: a third empty, a third with a state only, the rest with both"""
    rs = np.random.RandomState(seed)
    lens = np.array([0 if i % 3 == 0 else 1 + i % 5 for i in range(n)], dtype=np.uint64)
    seen = [rs.randint(0, 1000, 0 if i % 3 != 2 and i % 7 else 1 + i % w).astype(np.uint32) for i in range(n)]
    h = rs.randn(n, dim).astype(np.float32)
    c = rs.randn(n, dim).astype(np.float32) if kind != 2 else None
    return np.arange(n, dtype=np.uint32), h, c, lens, seen


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_file_arrays_round_trip_without_a_device(kind, tmp_path):
    from sbr_rs_amd.persistence import sessions_file_arrays, sessions_file_chunks

    dim, n, w = 6, 50, 4
    sl, h, c, lens, seen = _synthetic(kind, dim, n, w, seed=kind)
    cuts = [0, 17, 18, 50]  # the store is read in runs of slots
    runs = [(sl[a:b], h[a:b], None if c is None else c[a:b], lens[a:b], seen[a:b]) for a, b in zip(cuts, cuts[1:])]
    z = sessions_file_arrays(n + 3, w, dim, kind, runs)
    live = [i for i in range(n) if lens[i] or len(seen[i])]
    assert 0 < len(live) < n and any(lens[i] == 0 for i in live) and any(len(seen[i]) == 0 for i in live)
    assert z["slots"].tolist() == live and z["slots"].dtype == np.uint32
    assert int(z["capacity"]) == n + 3 and int(z["seen_capacity"]) == w and int(z["embedding_dim"]) == dim and int(z["model"]) == kind
    assert ("c" in z) == (kind != 2)
    assert z["len"].dtype == np.uint64 and z["seen_ptr"].dtype == np.uint64 and z["seen_items"].dtype == np.uint32
    assert z["seen_ptr"].size == len(live) + 1 and int(z["seen_ptr"][-1]) == z["seen_items"].size
    path = str(tmp_path / "arrays.npz")
    np.savez(path, **z)
    back = np.load(path)
    got = {}
    for bs, bh, bc, bn, (bp, bi) in sessions_file_chunks(back, chunk=7):
        assert 1 <= bs.size <= 7 and bp[0] == 0 and bp.size == bs.size + 1 and int(bp[-1]) == bi.size
        for j, s in enumerate(bs.tolist()):
            got[s] = (bh[j], None if bc is None else bc[j], int(bn[j]), bi[int(bp[j]):int(bp[j + 1])])
    assert sorted(got) == live
    for s in live:
        assert np.array_equal(got[s][0].view(np.uint32), h[s].view(np.uint32))
        assert (c is None and got[s][1] is None) or np.array_equal(got[s][1].view(np.uint32), c[s].view(np.uint32))
        assert got[s][2] == int(lens[s]) and np.array_equal(got[s][3], seen[s])


def test_file_arrays_of_an_empty_store_and_bad_input():
    from sbr_rs_amd.persistence import sessions_file_arrays, sessions_file_chunks

    z = sessions_file_arrays(10, 0, 4, 0, [(np.arange(10), np.zeros((10, 4)), np.zeros((10, 4)), np.zeros(10), None)])
    assert z["slots"].size == 0 and z["h"].shape == (0, 4) and z["seen_ptr"].tolist() == [0] and z["seen_items"].size == 0
    assert list(sessions_file_chunks(z)) == []
    with pytest.raises(ValueError):  # an LSTM's cell states are part of its state
        sessions_file_arrays(2, 0, 4, 0, [(np.arange(2), np.zeros((2, 4)), None, np.ones(2), None)])
    with pytest.raises(ValueError):  # runs of slots ascend
        sessions_file_arrays(4, 0, 4, 2, [(np.array([2, 3]), np.zeros((2, 4)), None, np.ones(2), None),
                                          (np.array([0, 1]), np.zeros((2, 4)), None, np.ones(2), None)])
