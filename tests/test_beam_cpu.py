"""CPU: the numpy statement of the beam-search contract (beam_expect.py) holds its own properties on the oracle — the f32 lp against
float64, exhaustion of a small tree, width 1 as greedy rollout — the Python layer refuses bad arguments before any library call, and
the new surface is there at every layer."""
import ctypes as C
import inspect
import itertools
import os

import numpy as np
import pytest

from beam_expect import beam_expect, log_mass, step_log_prob
from helpers import LOSS_HINGE, hparams
from oracle.oracle import OracleModel
from partition_expect import frac_bits, partition_row, weights
from recommend_expect import NO_ITEM, topk_expectation
from rollout_expect import oracle_callables, rollout_expect
from sbr_rs_amd import _abi, _lib
from sbr_rs_amd._abi import ModelKind, Param, Status

HERE = os.path.dirname(os.path.abspath(__file__))
_ITEMS, _T, _D = 60, 12, 16
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oracle(kind):
    o = OracleModel(hparams(_ITEMS, _T, _D, int(kind), LOSS_HINGE, B=8))
    rs = np.random.RandomState(3)
    E = (rs.randn(_ITEMS, _D) * 0.3).astype(np.float32)
    E[[20, 21, 22]] = E[0]  # exact ties
    o.set_param(Param.ITEM_EMBEDDING, E)
    o.set_param(Param.ITEM_BIAS, np.round(rs.randn(_ITEMS) * 0.5, 1).astype(np.float32))
    return o


_HIST = [[], [3], [1, 2, 3, 4], [5, 5, 7]]


def test_step_log_prob_is_log_w_over_mass_to_a_few_ulps():
    """lp = fl(fl(t - shift) - L) against float64 log(w / mass), w and mass the contract's fixed-point integers, over random rows of
    a 1e4-item softmax, where w >= 2^20.  The bound is 4 f32 ulps of |lp|, from the error budget: d = fl(t - shift) is exact
    (Sterbenz: t and shift are within a factor 2 for the items that carry weight, or d is rounded once, <= 0.5 ulp of |d| <= |lp|);
    log(w / 2^F) differs from d by exp32's error (a few 1e-8 relative, so absolute in the log) and by w's truncation (at most
    1 / w <= 2^-20 absolute); x carries mass to 24 bits (<= 2^-24 relative, absolute in the log); log32 is within about one ulp of L;
    the last subtraction rounds once (0.5 ulp of |lp|).  The rows are drawn so that no item dominates: L >= 1, hence |lp| >= 1 and
    one ulp of |lp| >= 2^-23, and the sum of these terms stays below 4 ulps of |lp|."""
    rs = np.random.RandomState(11)
    items, temperature = 10000, 0.7
    fb = frac_bits(items)
    worst = 0.0
    checked = 0
    for row in range(8):
        s = (rs.randn(items) * (0.5 + 0.125 * row)).astype(F)  # score spreads of 0.5 .. 1.375: no item dominates
        shift, mass = partition_row(s, (), temperature)
        L = log_mass(mass, fb)
        assert L >= 1.0
        w = weights(s, temperature, shift, fb)
        keep = w >= np.uint64(2 ** 20)
        lp = np.array([step_log_prob(x, shift, L, temperature) for x in s[keep]], dtype=F)
        ref = np.log(w[keep].astype(np.float64)) - np.log(float(mass))
        err = np.abs(lp.astype(np.float64) - ref)
        ulp = np.spacing(np.abs(lp)).astype(np.float64)
        ratio = float(np.max(err / ulp))
        print(f"row {row}: L={float(L):.4f} {int(keep.sum())} items, max |lp - log(w/mass)| = {ratio:.3f} ulps")
        worst = max(worst, ratio)
        checked += int(keep.sum())
        assert np.all(np.isfinite(lp)) and np.all(lp <= 0)
    assert checked > 1000
    assert worst <= 4.0, worst


def test_the_mass_logarithm_is_exact_in_its_argument():
    fb = 40
    for mass in (2 ** 40, 2 ** 40 + 1, 3 * 2 ** 40 + 12345, 2 ** 62 - 1, (2 ** 24 - 1) << 17):
        s = max(0, mass.bit_length() - 24)
        x = F(np.ldexp(F(mass >> s), s - fb))
        assert float(x) == (mass >> s) * 2.0 ** (s - fb) and float(x) >= 1.0
        assert _bits(log_mass(mass, fb)) == _bits(F(log_mass(mass, fb)))
    assert log_mass(2 ** 40, 40) == 0.0  # one item of weight 2^F: log 1


@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA])
def test_exhaustion_returns_every_path_in_the_three_key_order(kind):
    o = _oracle(kind)
    rep, scores = oracle_callables(o, _ITEMS)
    allowed = [4, 9, 20, 21, 33, 47]  # 20 and 21 are duplicates: a tie decided by id
    excl = [[x for x in range(_ITEMS) if x not in allowed]]
    hist = [[2, 8]]
    T = 0.7
    e = beam_expect(rep, scores, _ITEMS, hist, 2, 32, T, excl)
    assert e.lengths.tolist() == [2] and e.beams.tolist() == [30]
    # the same by brute force: every (a, b), its cum by the formula, sorted by (cum desc, a's rank at step 0, b's place under a)
    fb = frac_bits(_ITEMS)
    s0 = np.asarray(scores(rep(hist[0])), dtype=F)
    it0, sc0 = topk_expectation(s0, excl[0], 32)
    sh0, m0 = partition_row(s0, excl[0], T)
    first = [(int(it0[q]), step_log_prob(sc0[q], sh0, log_mass(m0, fb), T)) for q in range(6)]
    order0 = sorted(range(6), key=lambda q: (-float(first[q][1]), q))  # the beams after step 0, in selection order
    paths = []
    for rank, q0 in enumerate(order0):
        a, lp0 = first[q0]
        s1 = np.asarray(scores(rep(hist[0] + [a])), dtype=F)
        ex1 = excl[0] + [a]
        it1, sc1 = topk_expectation(s1, ex1, 32)
        sh1, m1 = partition_row(s1, ex1, T)
        for q1 in range(5):
            lp1 = step_log_prob(sc1[q1], sh1, log_mass(m1, fb), T)
            paths.append((F(F(F(0.0) + lp0) + lp1), rank, q1, [a, int(it1[q1])]))
    paths.sort(key=lambda p: (-float(p[0]), p[1], p[2]))
    assert sorted(tuple(p[3]) for p in paths) == sorted(itertools.permutations(allowed, 2))
    assert [p[3] for p in paths] == e.items[0, :30].tolist()
    assert np.array_equal(_bits([p[0] for p in paths]), _bits(e.cum[0, :30]))
    assert np.all(e.items[0, 30:] == NO_ITEM) and np.all(np.isneginf(e.cum[0, 30:]))
    assert np.all(np.diff(e.cum[0, :30]) <= 0)


@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA])
def test_width_one_is_greedy_rollout(kind):
    o = _oracle(kind)
    rep, scores = oracle_callables(o, _ITEMS)
    excl = [[0, 1], [], [9], list(range(57))]
    T = 0.7
    e = beam_expect(rep, scores, _ITEMS, _HIST, 5, 1, T, excl)
    r = rollout_expect(rep, scores, _ITEMS, _HIST, 5, excl, partition_temperature=T)
    assert np.array_equal(e.items[:, 0], r.items) and np.array_equal(_bits(e.scores[:, 0]), _bits(r.scores))
    assert np.array_equal(e.lengths, r.lengths) and e.lengths.tolist() == [5, 5, 5, 3]
    assert np.array_equal(_bits(e.shift[:, 0]), _bits(r.shift)) and np.array_equal(e.mass[:, 0], r.mass)
    fb = frac_bits(_ITEMS)
    for i in range(len(_HIST)):  # cum: the formula over rollout's shift and mass
        c = F(0.0)
        for j in range(int(r.lengths[i])):
            c = F(c + step_log_prob(r.scores[i, j], r.shift[i, j], log_mass(int(r.mass[i, j]), fb), T))
        assert _bits(c) == _bits(e.cum[i, 0])


def test_shapes_padding_and_rows_that_end():
    o = _oracle(ModelKind.LSTM_NORMAL)
    rep, scores = oracle_callables(o, _ITEMS)
    W, steps = 4, 5
    excl = [[], list(range(57)), list(range(_ITEMS)), [3, 3, 1]]  # row 1: 3 items, 3 steps, fewer than W paths at the end; row 2: none
    e = beam_expect(rep, scores, _ITEMS, _HIST, steps, W, 1.0, excl)
    assert e.items.shape == (4, W, steps) and e.cum.shape == (4, W) and e.mass.dtype == np.uint64
    assert e.lengths.tolist() == [steps, 3, 0, steps] and e.beams.tolist() == [W, W, 0, W]
    assert all(len(set(p)) == 3 and set(p) <= {57, 58, 59} for p in e.items[1, :, :3].tolist())
    assert len(set(map(tuple, e.items[1, :, :3].tolist()))) == W  # distinct paths
    assert np.all(e.items[1, :, 3:] == NO_ITEM) and np.all(np.isneginf(e.step_lp[1, :, 3:])) and np.all(e.mass[1, :, 3:] == 0)
    assert np.all(e.items[2] == NO_ITEM) and np.all(np.isneginf(e.cum[2])) and np.all(np.isneginf(e.scores[2]))
    live = e.items != NO_ITEM
    assert np.all(e.step_lp[live] <= 0) and np.all(np.isfinite(e.step_lp[live]))
    # one step over 2 items: 2 paths, fewer than W
    e2 = beam_expect(rep, scores, _ITEMS, [[1]], 1, W, 1.0, [list(range(58))])
    assert e2.beams.tolist() == [2] and sorted(e2.items[0, :2, 0].tolist()) == [58, 59] and np.all(e2.items[0, 2:] == NO_ITEM)
    from sbr_rs_amd import engine

    b = engine.Beams(e.items, e.scores, e.step_lp, e.cum, e.lengths, e.beams)
    assert b.best().shape == (4, steps) and np.array_equal(b.best(), e.items[:, 0])
    assert [x.tolist() for x in b.rows(0)][1:3] == [e.items[1, 0, :3].tolist(), []]
    assert b.shift is None and b.mass is None and b.frac_bits is None


def test_allow_repeats_keeps_the_eligible_set():
    o = _oracle(ModelKind.EWMA)
    rep, scores = oracle_callables(o, _ITEMS)
    e = beam_expect(rep, scores, _ITEMS, [[1]], 4, 3, 1.0, [list(range(1, _ITEMS))], allow_repeats=True)
    assert e.lengths.tolist() == [4] and e.beams.tolist() == [1] and e.items[0, 0].tolist() == [0] * 4


def test_argument_refusals_come_before_any_library_call():
    from sbr_rs_amd import engine

    st = engine.Sessions.__new__(engine.Sessions)  # no handle and no library: reaching either is an AttributeError, not a ValueError
    st._seen = 0
    m = engine.Model.__new__(engine.Model)
    for kw in ({"steps": 0}, {"steps": 1025}, {"steps": -1}, {"steps": 2.5}, {"steps": True}, {"width": 0}, {"width": 33},
               {"width": 1.5}, {"width": False}, {"temperature": 0.0}, {"temperature": -1.0}, {"temperature": float("nan")},
               {"temperature": float("inf")}, {"temperature": 1e-45}, {"include_seen": True}):
        steps = kw.pop("steps", 3)
        with pytest.raises(ValueError):
            st.beam_search([0, 1], steps, **kw)
        if "include_seen" not in kw:
            with pytest.raises(ValueError):
                m.beam_search([[1, 2]], steps, **kw)
    st._seen = 4
    with pytest.raises(ValueError):
        st.beam_search([0, 1], 3, exclude=[[1]])  # one list per slot
    with pytest.raises(ValueError):
        st.beam_search([0, 1], 3, any_of=[1, 2, 3])


def test_surface_at_every_layer():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine

    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    L = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "sbr_hip.h")).read()
    name = "sbr_sessions_beam_search"
    assert name in _lib.DECLARED_SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == 17
    assert f"sbr_status {name}(" in header and "typedef struct sbr_beam_args" in header
    assert _abi.ABI_VERSION == 13 and L.sbr_abi_version() == 13 and "#define SBR_ABI_VERSION 13u" in header  # an addition only
    assert f"#define SBR_BEAM_MAX_WIDTH {_abi.BEAM_MAX_WIDTH}u" in header
    assert C.sizeof(_abi.SbrBeamArgs) == 16 and _abi.SbrBeamArgs.temperature.offset == 12
    p = inspect.signature(engine.Sessions.beam_search).parameters
    assert list(p)[:3] == ["self", "slots", "steps"]
    assert [p[k].default for k in ("width", "temperature", "exclude", "any_of", "none_of", "include_seen", "allow_repeats",
                                   "partitions")] == [4, 1.0, None, None, None, False, False, False]
    for fn in (engine.Model.beam_search, sbr.lstm.ImplicitLSTMModel.beam_search, sbr.ewma.ImplicitEWMAModel.beam_search):
        q = inspect.signature(fn).parameters
        assert list(q)[:3] == ["self", "histories", "steps"] and q["exclude_history"].default is True and q["width"].default == 4


def test_entry_point_refuses_without_a_store():
    L = _lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(8, 7, np.uint32)
    slots = np.zeros(1, np.uint32)
    ba = _abi.SbrBeamArgs()
    ba.steps, ba.width, ba.flags, ba.temperature = 2, 4, 0, 1.0
    nulls = [None] * 8
    assert L.sbr_sessions_beam_search(None, vp(slots), 1, C.byref(ba), None, None, None, None, vp(out), *nulls) == Status.INVALID_ARGUMENT
    assert np.all(out == 7)
