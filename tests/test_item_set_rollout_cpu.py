"""CPU: rollout and beam search within an item set.  The two entries are exported and the Python and C++ surfaces exist; the Python
layer refuses bad arguments before any library call; and the numpy statements (rollout_expect, beam_expect) with every item outside
S joined to each exclusion list equal, on the oracle, the same statements run on a catalogue that IS S's rows — scores restricted to
S, positions mapped back to ids, the noise keyed by catalogue id and F the model's, as the contract states — ties included.  So
"restrict" and "exclude the complement" agree in the reference itself."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import beam_expect as beam_mod
import partition_expect
import rollout_expect as rollout_mod
from beam_expect import beam_expect
from helpers import LOSS_HINGE, hparams
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM
from rollout_expect import oracle_callables, rollout_expect
from sbr_rs_amd import _abi, _lib
from sbr_rs_amd._abi import ModelKind, Param, Status

HERE = os.path.dirname(os.path.abspath(__file__))
_ITEMS, _T, _D = 60, 12, 16
_TEMP = 0.7
_OFF = 1 << 20  # a history item of the restricted statement: catalogue id + _OFF; a pick there is a position of S


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oracle(kind):
    o = OracleModel(hparams(_ITEMS, _T, _D, int(kind), LOSS_HINGE, B=8))
    rs = np.random.RandomState(5)
    E = (rs.randn(_ITEMS, _D) * 0.3).astype(np.float32)
    E[[20, 21, 22, 50, 52]] = E[0]  # exact ties, some straddling the set (50 and 52 in it, 51 not)
    E[51] = E[0]
    o.set_param(Param.ITEM_EMBEDDING, E)
    o.set_param(Param.ITEM_BIAS, np.round(rs.randn(_ITEMS) * 0.5, 1).astype(np.float32))
    return o


_HIST = [[], [3], [1, 2, 3, 4], [5, 5, 7], [50, 52], [0]]
_SETS = {
    "small": np.array([0, 3, 20, 22, 31, 40, 50, 52, 59], dtype=np.uint32),
    "third": np.arange(0, _ITEMS, 3, dtype=np.uint32),
    "one": np.array([21], dtype=np.uint32),
    "all": np.arange(_ITEMS, dtype=np.uint32),
}


def _excl(S):
    """per row: the caller's list (one leaves 3 set items, one nothing), and the same with C(S) joined"""
    comp = np.setdiff1d(np.arange(_ITEMS), S)
    lists = [[], [9, 3], [], S[3:].tolist() if S.size > 3 else [], S.tolist(), [59, 0, 7]]
    return lists, [np.concatenate([np.asarray(x, dtype=np.int64), comp]) for x in lists]


def _restricted(o, S, monkeypatch):
    """rep / scores of a catalogue that is S's rows: positions of S stand for S's ids, F stays the model's, noise is keyed by id"""
    rep, scores = oracle_callables(o, _ITEMS)
    fb = partition_expect.frac_bits(_ITEMS)
    monkeypatch.setattr(partition_expect, "frac_bits", lambda n: fb)
    monkeypatch.setattr(beam_mod, "frac_bits", lambda n: fb)
    noise = rollout_mod.noise
    monkeypatch.setattr(rollout_mod, "noise", lambda seed, streams, items: noise(seed, streams, S[np.asarray(items, dtype=np.int64)]))

    def rep_r(hist):
        return rep([x - _OFF if x >= _OFF else int(S[x]) for x in hist])

    return rep_r, lambda h: np.asarray(scores(h), dtype=np.float32)[S]


def _positions(S, lists):
    return [np.searchsorted(S, np.intersect1d(np.asarray(x, dtype=np.int64), S)) for x in lists]


def _ids(S, items):
    out = np.full(items.shape, NO_ITEM, dtype=np.uint32)
    real = items != NO_ITEM
    out[real] = S[items[real].astype(np.int64)]
    return out


@pytest.mark.parametrize("name", sorted(_SETS))
@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA], ids=lambda k: k.name)
def test_restricting_is_excluding_the_complement_in_the_statements(kind, name, monkeypatch):
    o = _oracle(kind)
    S = _SETS[name]
    rep, scores = oracle_callables(o, _ITEMS)
    lists, joined = _excl(S)
    rs = np.random.RandomState(2)
    tags = rs.randint(0, 8, _ITEMS).astype(np.uint32)
    any_of = rs.randint(0, 8, len(_HIST)).astype(np.uint32)
    steps, w = 4, 3
    # the complement route over the whole catalogue
    greedy = rollout_expect(rep, scores, _ITEMS, _HIST, steps, joined, partition_temperature=_TEMP)
    sampled = rollout_expect(rep, scores, _ITEMS, _HIST, steps, joined, sample=(_TEMP, 9), partition_temperature=_TEMP)
    filt = rollout_expect(rep, scores, _ITEMS, _HIST, steps, joined, tags=tags, any_of=any_of, none_of=4)
    beams = beam_expect(rep, scores, _ITEMS, _HIST, steps, w, _TEMP, joined)
    beams_rep = beam_expect(rep, scores, _ITEMS, _HIST, 3, w, _TEMP, joined, allow_repeats=True)
    # the restricted route: a catalogue of S's rows
    rep_r, scores_r = _restricted(o, S, monkeypatch)
    hist_r = [[x + _OFF for x in h] for h in _HIST]
    pos = _positions(S, lists)
    n = len(S)
    g_r = rollout_expect(rep_r, scores_r, n, hist_r, steps, pos, partition_temperature=_TEMP)
    s_r = rollout_expect(rep_r, scores_r, n, hist_r, steps, pos, sample=(_TEMP, 9), partition_temperature=_TEMP)
    f_r = rollout_expect(rep_r, scores_r, n, hist_r, steps, pos, tags=tags[S], any_of=any_of, none_of=4)
    b_r = beam_expect(rep_r, scores_r, n, hist_r, steps, w, _TEMP, pos)
    br_r = beam_expect(rep_r, scores_r, n, hist_r, 3, w, _TEMP, pos, allow_repeats=True)
    for e, r in ((greedy, g_r), (sampled, s_r), (filt, f_r)):
        assert np.array_equal(e.items, _ids(S, r.items)) and np.array_equal(e.lengths, r.lengths)
        assert np.array_equal(_bits(e.scores), _bits(r.scores))
        if e.keys is not None:
            assert np.array_equal(_bits(e.keys), _bits(r.keys))
        if e.shift is not None:
            assert np.array_equal(_bits(e.shift), _bits(r.shift)) and np.array_equal(e.mass, r.mass)
    for e, r in ((beams, b_r), (beams_rep, br_r)):
        assert np.array_equal(e.items, _ids(S, r.items)) and np.array_equal(e.lengths, r.lengths) and np.array_equal(e.beams, r.beams)
        for f in ("scores", "step_lp", "cum", "shift"):
            assert np.array_equal(_bits(getattr(e, f)), _bits(getattr(r, f))), f
        assert np.array_equal(e.mass, r.mass)
    # the cases the tests lean on: the row left with 3 set items ends after 3 steps (at most 6 paths), the last list may see nothing
    # only for the one-item set, and a row whose list is S itself sees nothing
    if S.size > 3:
        assert greedy.lengths[3] == 3 and beams.lengths[3] == 3 and beams.beams[3] == min(w, 6)
    assert greedy.lengths[4] == 0 and beams.beams[4] == 0 and np.all(greedy.items[4] == NO_ITEM)
    assert np.all(np.isin(greedy.items[greedy.items != NO_ITEM], S)) and np.all(np.isin(beams.items[beams.items != NO_ITEM], S))


def test_the_empty_set_ends_every_row_at_step_zero():
    o = _oracle(ModelKind.LSTM_COUPLED)
    rep, scores = oracle_callables(o, _ITEMS)
    every = [np.arange(_ITEMS)] * len(_HIST)
    e = rollout_expect(rep, scores, _ITEMS, _HIST, 3, every, partition_temperature=_TEMP)
    assert np.all(e.lengths == 0) and np.all(e.items == NO_ITEM) and np.all(e.mass == 0) and np.all(np.isneginf(e.shift))
    b = beam_expect(rep, scores, _ITEMS, _HIST, 3, 4, _TEMP, every)
    assert np.all(b.lengths == 0) and np.all(b.beams == 0) and np.all(b.items == NO_ITEM)


class _FakeSet:
    _h = None

    @staticmethod
    def _check(st):  # reaching the library from a refused call is an AttributeError on None, not a ValueError
        raise AssertionError("the library was called")


def test_argument_refusals_come_before_any_library_call():
    from sbr_rs_amd import engine

    st = engine.Sessions.__new__(engine.Sessions)  # no handle and no library: reaching either is an AttributeError, not a ValueError
    st._seen = 0
    on = engine.ItemSetSessions(_FakeSet(), st)
    for kw in ({"steps": 0}, {"steps": 1025}, {"steps": -1}, {"steps": 2.5}, {"steps": True}, {"mode": "beam"}, {"mode": None},
               {"temperature": 0.0}, {"temperature": -1.0}, {"temperature": float("nan")}, {"temperature": float("inf")},
               {"include_seen": True}):
        steps = kw.pop("steps", 3)
        with pytest.raises(ValueError):
            on.rollout([0, 1], steps, **kw)
    for kw in ({"steps": 0}, {"steps": 1025}, {"steps": 2.5}, {"width": 0}, {"width": 33}, {"width": 1.5}, {"width": False},
               {"temperature": 0.0}, {"temperature": float("nan")}, {"include_seen": True}):
        steps = kw.pop("steps", 3)
        with pytest.raises(ValueError):
            on.beam_search([0, 1], steps, **kw)
    s = engine.ItemSet.__new__(engine.ItemSet)  # histories: refused before any store is made
    for kw in ({"steps": 0}, {"mode": "beam"}, {"temperature": 0.0}):
        steps = kw.pop("steps", 3)
        with pytest.raises(ValueError):
            s.rollout([[1, 2]], steps, **kw)
    for kw in ({"steps": 0}, {"width": 33}, {"temperature": -1.0}):
        steps = kw.pop("steps", 3)
        with pytest.raises(ValueError):
            s.beam_search([[1, 2]], steps, **kw)
    st._seen = 4
    with pytest.raises(ValueError):
        on.rollout([0, 1], 3, exclude=[[1]])  # one list per slot
    with pytest.raises(ValueError):
        on.beam_search([0, 1], 3, any_of=[1, 2, 3])


def test_surface_at_every_layer():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine

    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    L = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "sbr_hip.h")).read()
    for name in ("sbr_item_set_rollout", "sbr_item_set_beam_search"):
        assert name in _lib.DECLARED_SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == 13
        assert f"sbr_status {name}(sbr_item_set* set, const struct sbr_scan_rows* rows" in header
    assert _abi.ABI_VERSION == 13 and L.sbr_abi_version() == 13 and "#define SBR_ABI_VERSION 13u" in header  # additions only
    for a, b in ((engine.ItemSetSessions.rollout, engine.Sessions.rollout), (engine.ItemSetSessions.beam_search, engine.Sessions.beam_search)):
        pa, pb = inspect.signature(a).parameters, inspect.signature(b).parameters
        assert list(pa) == list(pb) and all(pa[k].default == pb[k].default for k in pa)
    for a, b in ((engine.ItemSet.rollout, engine.Model.rollout), (engine.ItemSet.beam_search, engine.Model.beam_search),
                 (sbr.lstm.ItemSetView.rollout, sbr.lstm.ImplicitLSTMModel.rollout),
                 (sbr.lstm.ItemSetView.beam_search, sbr.lstm.ImplicitLSTMModel.beam_search)):
        pa, pb = inspect.signature(a).parameters, inspect.signature(b).parameters
        assert list(pa) == list(pb) and all(pa[k].default == pb[k].default for k in pa)
    hpp = open(os.path.join(HERE, "..", "include", "sbr.hpp")).read()
    for s in ("Result<Rollout, PredictionError> rollout(const std::vector<std::uint32_t>& slots, const RolloutArgs& a) const {\n"
              "            return store_.rollout_in(set_.h_, slots, a);",
              "Result<Beams, PredictionError> beam_search(const std::vector<std::uint32_t>& slots, const BeamArgs& a) const {\n"
              "            return store_.beam_search_in(set_.h_, slots, a);",
              "sbr_item_set_rollout(set, &d", "sbr_item_set_beam_search(set, &d"):
        assert s in hpp, s
    assert "ITEM_SET_ROLLOUT_SRC" in open(os.path.join(HERE, "..", "sbr_rs_amd", "build.py")).read()


def test_entry_points_refuse_without_a_set_or_a_store():
    L = _lib.load()
    out = np.full(8, 7, np.uint32)
    ra = _abi.SbrRolloutArgs()
    ra.steps = 2
    ba = _abi.SbrBeamArgs()
    ba.steps, ba.width, ba.temperature = 2, 4, 1.0
    d = _abi.SbrScanRows()
    vp = out.ctypes.data_as(C.c_void_p)
    assert L.sbr_item_set_rollout(None, C.byref(d), 1, C.byref(ra), vp, *([None] * 8)) == Status.INVALID_ARGUMENT
    assert L.sbr_item_set_beam_search(None, C.byref(d), 1, C.byref(ba), vp, *([None] * 8)) == Status.INVALID_ARGUMENT
    assert L.sbr_item_set_rollout(None, None, 1, C.byref(ra), vp, *([None] * 8)) == Status.INVALID_ARGUMENT
    assert np.all(out == 7)
