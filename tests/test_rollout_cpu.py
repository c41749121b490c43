"""CPU: the numpy statement of the rollout contract (rollout_expect.py) holds its own properties on the oracle, the Python layer
refuses bad arguments before any library call, and the new surface is there at every layer."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams
from oracle.oracle import OracleModel
from partition_expect import frac_bits, weights
from recommend_expect import NO_ITEM, topk_expectation
from rollout_expect import oracle_callables, rollout_expect
from sampled_expect import sampled_expect
from sbr_rs_amd import _abi, _lib
from sbr_rs_amd._abi import ModelKind, Param, Status

HERE = os.path.dirname(os.path.abspath(__file__))
_ITEMS, _T, _D = 60, 12, 16


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oracle(kind):
    o = OracleModel(hparams(_ITEMS, _T, _D, int(kind), LOSS_HINGE, B=8))
    rs = np.random.RandomState(3)
    E = (rs.randn(_ITEMS, _D) * 0.3).astype(np.float32)
    E[[20, 21, 22]] = E[0]  # exact ties: the duplicate of a picked item is the natural next pick
    o.set_param(Param.ITEM_EMBEDDING, E)
    o.set_param(Param.ITEM_BIAS, np.round(rs.randn(_ITEMS) * 0.5, 1).astype(np.float32))
    return o


_HIST = [[], [3], [1, 2, 3, 4], [5, 5, 7]]


@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA])
def test_one_step_is_the_top_1_and_the_draw(kind):
    o = _oracle(kind)
    rep, scores = oracle_callables(o, _ITEMS)
    excl = [[0, 1], [], [9], list(range(30))]
    e = rollout_expect(rep, scores, _ITEMS, _HIST, 1, excl)
    s = np.array([scores(rep(h)) for h in _HIST])
    for i in range(len(_HIST)):
        it, sc = topk_expectation(s[i], excl[i], 1)
        assert e.items[i, 0] == it[0] and _bits(e.scores[i, 0]) == _bits(sc[0])
    assert e.lengths.tolist() == [1] * len(_HIST) and e.keys is None and e.shift is None
    streams = np.array([7, 8, 9, 2 ** 40], dtype=np.uint64)
    es = rollout_expect(rep, scores, _ITEMS, _HIST, 1, excl, sample=(0.7, 11), streams=streams)
    wi, ws, wk = sampled_expect(s, excl, 1, 0.7, 11, streams)
    assert np.array_equal(es.items, wi) and np.array_equal(_bits(es.scores), _bits(ws)) and np.array_equal(_bits(es.keys), _bits(wk))


def test_rows_end_when_nothing_is_left_and_never_come_back():
    o = _oracle(ModelKind.LSTM_NORMAL)
    rep, scores = oracle_callables(o, _ITEMS)
    steps = 6
    hist = [[], [1], [2, 3], [4], [5]]
    excl = [np.delete(np.arange(_ITEMS), [4, 8, 30]), np.arange(_ITEMS), [], np.arange(1, _ITEMS), np.arange(6, _ITEMS)]
    e = rollout_expect(rep, scores, _ITEMS, hist, steps, excl, partition_temperature=0.5)
    m = [3, 0, _ITEMS, 1, 6]
    assert e.lengths.tolist() == [min(x, steps) for x in m]
    for i, n in enumerate(e.lengths):
        assert np.all(e.items[i, n:] == NO_ITEM) and np.all(np.isneginf(e.scores[i, n:]))
        assert np.all(np.isneginf(e.shift[i, n:])) and np.all(e.mass[i, n:] == 0)
        picks = e.items[i, :n]
        assert len(set(picks.tolist())) == n and not set(picks.tolist()) & set(np.asarray(excl[i]).tolist())
        assert e.histories[i] == list(hist[i]) + picks.tolist()
        # the arg-max weighs exactly 2^F, so a live step's mass is at least that; the greedy pick IS the arg-max
        fb = frac_bits(_ITEMS)
        assert np.all(e.mass[i, :n] >= np.uint64(1) << np.uint64(fb))
        assert np.all(weights(e.scores[i, :n], 0.5, e.shift[i, :n], fb) == np.uint64(1) << np.uint64(fb))
    assert sorted(e.items[0, :3].tolist()) == [4, 8, 30]
    # the state moves: the scores of step 1 are taken against the history with pick 0 appended
    s1 = scores(rep(hist[2] + [int(e.items[2, 0])]))
    it, sc = topk_expectation(s1, [int(e.items[2, 0])], 1)
    assert e.items[2, 1] == it[0] and _bits(e.scores[2, 1]) == _bits(sc[0])


def test_allow_repeats_may_repeat_and_keeps_the_eligible_set():
    o = _oracle(ModelKind.EWMA)
    rep, scores = oracle_callables(o, _ITEMS)
    only = [np.delete(np.arange(_ITEMS), [17])]  # one eligible item: without repeats the row ends after it
    a = rollout_expect(rep, scores, _ITEMS, [[2]], 4, only)
    b = rollout_expect(rep, scores, _ITEMS, [[2]], 4, only, allow_repeats=True)
    assert a.lengths.tolist() == [1] and a.items[0].tolist() == [17] + [NO_ITEM] * 3
    assert b.lengths.tolist() == [4] and b.items[0].tolist() == [17] * 4
    assert len(set(_bits(b.scores[0]).tolist())) > 1  # the same item, scored against a state that moved


def test_sampled_steps_use_their_own_seed():
    o = _oracle(ModelKind.LSTM_COUPLED)
    rep, scores = oracle_callables(o, _ITEMS)
    e = rollout_expect(rep, scores, _ITEMS, [[1, 2]], 3, None, sample=(1.0, 2 ** 64 - 1), streams=[5], allow_repeats=True)
    # step j is the draw at (seed + j) mod 2^64 against the history so far
    for j in range(3):
        hist = [1, 2] + e.items[0, :j].tolist()
        wi, ws, wk = sampled_expect(np.array([scores(rep(hist))]), None, 1, 1.0, (2 ** 64 - 1 + j) % 2 ** 64, [5])
        assert e.items[0, j] == wi[0, 0] and _bits(e.keys[0, j]) == _bits(wk[0, 0])


def test_argument_refusals_come_before_any_library_call():
    from sbr_rs_amd import engine

    st = engine.Sessions.__new__(engine.Sessions)  # no handle and no library: reaching either is an AttributeError, not a ValueError
    st._seen = 0
    m = engine.Model.__new__(engine.Model)
    for kw in ({"steps": 0}, {"steps": 1025}, {"steps": -1}, {"steps": 2.5}, {"steps": True}, {"mode": "beam"}, {"mode": None},
               {"temperature": 0.0}, {"temperature": -1.0}, {"temperature": float("nan")}, {"temperature": float("inf")},
               {"temperature": 1e-45}, {"include_seen": True}):
        steps = kw.pop("steps", 3)
        with pytest.raises(ValueError):
            st.rollout([0, 1], steps, **kw)
        if "include_seen" not in kw:
            with pytest.raises(ValueError):
                m.rollout([[1, 2]], steps, **kw)
    st._seen = 4
    with pytest.raises(ValueError):
        st.rollout([0, 1], 3, exclude=[[1]])  # one list per slot
    with pytest.raises(ValueError):
        st.rollout([0, 1], 3, mode="sample", streams=[1, 2, 3])
    with pytest.raises(ValueError):
        st.rollout([0, 1], 3, any_of=[1, 2, 3])


def test_surface_at_every_layer():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine

    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    L = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "sbr_hip.h")).read()
    name = "sbr_sessions_rollout"
    assert name in _lib.DECLARED_SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == 17
    assert f"sbr_status {name}(" in header and "typedef struct sbr_rollout_args" in header
    assert _abi.ABI_VERSION == 13 and L.sbr_abi_version() == 13 and "#define SBR_ABI_VERSION 13u" in header  # an addition only
    for macro, value in (("SBR_ROLLOUT_MAX_STEPS", _abi.ROLLOUT_MAX_STEPS), ("SBR_ROLLOUT_SAMPLE", _abi.ROLLOUT_SAMPLE),
                         ("SBR_ROLLOUT_ALLOW_REPEATS", _abi.ROLLOUT_ALLOW_REPEATS), ("SBR_ROLLOUT_INCLUDE_SEEN", _abi.ROLLOUT_INCLUDE_SEEN)):
        assert f"#define {macro} {value}u" in header, macro
    # struct sbr_rollout_args {u32 steps; u32 flags; struct sbr_sample_args {f32; u64; ptr}}
    assert C.sizeof(_abi.SbrRolloutArgs) == 8 + C.sizeof(_abi.SbrSampleArgs) and _abi.SbrRolloutArgs.sample.offset == 8
    p = inspect.signature(engine.Sessions.rollout).parameters
    assert list(p)[:3] == ["self", "slots", "steps"]
    assert [p[k].default for k in ("mode", "temperature", "seed", "streams", "exclude", "any_of", "none_of", "include_seen",
                                   "allow_repeats", "log_prob", "final_state")] == ["greedy", 1.0, 0, None, None, None, None, False, False,
                                                                                    False, False]
    for fn in (engine.Model.rollout, sbr.lstm.ImplicitLSTMModel.rollout, sbr.ewma.ImplicitEWMAModel.rollout):
        q = inspect.signature(fn).parameters
        assert list(q)[:3] == ["self", "histories", "steps"] and q["exclude_history"].default is True and q["mode"].default == "greedy"
    r = engine.Rollout(np.array([[4, 9, NO_ITEM], [NO_ITEM] * 3], np.uint32), np.zeros((2, 3), np.float32), np.array([2, 0], np.uint32))
    assert [x.tolist() for x in r.rows()] == [[4, 9], []] and r.keys is None and r.log_prob is None and r.h is None


def test_entry_point_refuses_without_a_store():
    L = _lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(4, 7, np.uint32)
    slots = np.zeros(1, np.uint32)
    ra = _abi.SbrRolloutArgs()
    ra.steps, ra.flags = 4, 0
    ra.sample.temperature = 1.0
    nulls = [None] * 8
    assert L.sbr_sessions_rollout(None, vp(slots), 1, C.byref(ra), None, None, None, None, vp(out), *nulls) == Status.INVALID_ARGUMENT
    assert np.all(out == 7)
