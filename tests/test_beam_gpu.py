"""GPU: sbr_sessions_beam_search (beam_select_kernel and its neighbours in sbr_sessions.hip, launch_topk_partition in
sbr_catalogue.hip) against the contract stated in beam_expect.py over the oracle's representations and scores.  Everything is an
equality: ids, lengths and beam counts as integers, f32 by bits, masses as integers.  1 000 items (32 item tiles, the last ragged),
70 rows (crossing a row tile of 64 at W = 1 and every tile boundary of the beam rows above), d = 16 and d = 100 (stored as 128),
SBR_CATALOGUE_GROUPS=3.  Embeddings are planted as in test_rollout_gpu (duplicate rows, biases on a 0.1 grid), so ties decide both
the scans' order and the selection's.  Histories of at most 6 items and at most 6 steps stay inside the oracle's window."""
import ctypes as C
import functools

import numpy as np
import pytest

from beam_expect import Expected, beam_expect, log_mass, step_log_prob
from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from partition_expect import frac_bits
from recommend_expect import NO_ITEM
from rollout_expect import oracle_callables
from sbr_rs_amd import _abi, _lib
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError

pytestmark = pytest.mark.gpu

NORMAL, COUPLED, EWMA = ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA
_ITEMS, _ROWS, _T, _STEPS = 1000, 70, 24, 5
_CONFIGS = [(k, d) for d in (16, 100) for k in (NORMAL, COUPLED, EWMA)]
_SMALL = [(NORMAL, 16), (COUPLED, 16), (EWMA, 16), (NORMAL, 100)]
_ids = lambda v: getattr(v, "name", str(v))  # noqa: E731
_TEMP = 0.7


@pytest.fixture(autouse=True)
def _groups(monkeypatch):
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", "3")  # the scan reads the hook per call


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _planted(items, d, seed):
    rs = np.random.RandomState(seed)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    E[rs.choice(np.arange(10, items), 20, replace=False)] = E[0]
    E[5] = 0.0
    E[7] = 2.0 * E[3]
    E[9] = -E[3]
    return E, np.round(rs.randn(items) * 0.5, 1).astype(np.float32)


def _pair(kind, d, items=_ITEMS, T=_T):
    hp = hparams(items, T, d, int(kind), LOSS_HINGE, B=8)
    g, o = Model(hp), OracleModel(hp)
    E, bias = _planted(items, d, d + items)
    rs = np.random.RandomState(int(kind) * 7 + d)
    extra = ({Param.EWMA_ALPHA: rs.randn(d)} if kind == EWMA else
             {Param.LSTM_W: rs.randn(2 * d, (4 if kind == NORMAL else 3) * d) * 0.3, Param.LSTM_B: rs.randn((4 if kind == NORMAL else 3) * d) * 0.5})
    for m in (g, o):
        m.set_param(Param.ITEM_EMBEDDING, E)
        m.set_param(Param.ITEM_BIAS, bias)
        for which, v in extra.items():
            m.set_param(which, v.astype(np.float32).ravel())
    return g, o


def _memo(o, items):
    rep, scores = oracle_callables(o, items)
    memo = {}

    def scores_of(hist):
        key = tuple(int(x) for x in hist)
        if key not in memo:
            memo[key] = scores(rep(list(key)))
        return memo[key]

    return (lambda hist: hist), scores_of  # the "representation" handed on is the history: scores_of memoises on it


class _Case:
    """One configuration: the model pair, a store holding 70 histories (a row left with 3 items, a row that may see nothing, an
    unsorted list, an empty slot among them), and the memoised oracle."""

    def __init__(self, kind, d):
        self.kind, self.d = kind, d
        self.g, self.o = _pair(kind, d)
        rs = np.random.RandomState(d + int(kind))
        self.hist = [rs.randint(0, _ITEMS, rs.randint(0, 7)).astype(np.uint32) for _ in range(_ROWS)]
        self.hist[3] = np.zeros(0, np.uint32)  # an empty slot
        self.excl = [rs.randint(0, _ITEMS, rs.randint(0, 30)) for _ in range(_ROWS)]
        self.excl[0] = np.delete(np.arange(_ITEMS), [17, 500, 999])  # three eligible items: ends after 3 steps, at most 6 paths
        self.excl[1] = np.arange(_ITEMS)                             # may see nothing
        self.excl[2] = rs.permutation(_ITEMS)[:900]                  # an unsorted list
        self.excl[3] = []
        self.tags = rs.randint(0, 16, _ITEMS).astype(np.uint32)
        self.any_of = rs.randint(0, 16, _ROWS).astype(np.uint32)
        self.none_of = 8
        self.g.set_item_tags(self.tags)
        self.slots = (np.arange(_ROWS, dtype=np.uint32) * 3 + 1)  # not the identity: a slot is not a row
        self.store = self.g.sessions(3 * _ROWS + 5)
        self.store.append(self.slots, self.hist)
        self.rep, self.scores = _memo(self.o, _ITEMS)

    @functools.lru_cache(maxsize=None)
    def expect(self, variant, w, rows=_ROWS, steps=_STEPS):
        kw = {"plain": {}, "tags": dict(tags=self.tags, any_of=self.any_of[:rows], none_of=self.none_of),
              "repeats": dict(allow_repeats=True)}[variant]
        return beam_expect(self.rep, self.scores, _ITEMS, self.hist[:rows], steps, w, _TEMP, self.excl[:rows], **kw)


@functools.lru_cache(maxsize=None)
def _case(kind, d):
    return _Case(kind, d)


def _same(r, e: Expected, what=""):
    bad = np.argwhere(r.items != e.items)
    assert bad.size == 0, f"{what}: {len(bad)} items differ; first at {bad[0]}: {r.items[tuple(bad[0])]} vs {e.items[tuple(bad[0])]}"
    assert np.array_equal(r.lengths, e.lengths), what
    assert np.array_equal(r.beams, e.beams), what
    assert np.array_equal(_bits(r.scores), _bits(e.scores)), what
    assert np.array_equal(_bits(r.step_log_probs), _bits(e.step_lp)), what
    assert np.array_equal(_bits(r.log_probs), _bits(e.cum)), what
    if r.shift is not None:
        assert np.array_equal(_bits(r.shift), _bits(e.shift)), what
        assert np.array_equal(r.mass, e.mass), what


# ---- 1. against the contract over the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 3, 8])
@pytest.mark.parametrize("kind,d", _CONFIGS, ids=_ids)
def test_beams_are_the_contract_over_the_oracle(kind, d, w):
    c = _case(kind, d)
    e = c.expect("plain", w)
    r = c.store.beam_search(c.slots, _STEPS, width=w, temperature=_TEMP, exclude=c.excl)
    _same(r, e, f"W={w}")
    assert r.shift is None and r.mass is None
    assert e.lengths[:4].tolist() == [3, 0, _STEPS, _STEPS]
    assert e.beams[0] == min(w, 6) and e.beams[1] == 0  # 3 eligible items: 3 * 2 * 1 paths
    assert np.all(r.items[1] == NO_ITEM) and np.all(np.isneginf(r.log_probs[1]))


# ---- 2. tags, repeats, the seen-item memory ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", _SMALL, ids=_ids)
def test_tag_masks_repeats_and_seen_memory(kind, d):
    c = _case(kind, d)
    rows, w = 24, 3
    r = c.store.beam_search(c.slots[:rows], _STEPS, width=w, temperature=_TEMP, exclude=c.excl[:rows], any_of=c.any_of[:rows],
                            none_of=c.none_of)
    _same(r, c.expect("tags", w, rows), "tags")
    r = c.store.beam_search(c.slots[:rows], _STEPS, width=w, temperature=_TEMP, exclude=c.excl[:rows], allow_repeats=True)
    e = c.expect("repeats", w, rows)
    _same(r, e, "repeats")
    assert e.lengths[0] == _STEPS and e.lengths[1] == 0
    # nothing excluded at all: the scans run without an exclusion CSR
    r = c.store.beam_search(c.slots[:rows], 2, width=w, temperature=_TEMP, allow_repeats=True)
    _same(r, beam_expect(c.rep, c.scores, _ITEMS, c.hist[:rows], 2, w, _TEMP, None, allow_repeats=True), "bare")
    # a store with memory (remember = W): its ring's items join X_0 unless include_seen
    st = c.g.sessions(rows, w)
    slots = np.arange(rows, dtype=np.uint32)[::-1].copy()
    st.append(slots, c.hist[:rows])
    seen = st.seen(slots)
    full = [np.concatenate([np.asarray(c.excl[i], dtype=np.int64), seen[i].astype(np.int64)]) for i in range(rows)]
    r = st.beam_search(slots, _STEPS, width=w, temperature=_TEMP, exclude=c.excl[:rows])
    _same(r, beam_expect(c.rep, c.scores, _ITEMS, c.hist[:rows], _STEPS, w, _TEMP, full), "seen")
    r = st.beam_search(slots, _STEPS, width=w, temperature=_TEMP, exclude=c.excl[:rows], include_seen=True)
    _same(r, c.expect("plain", w, rows), "include_seen")
    st.close()


# ---- 3. width 1 is greedy rollout -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", _CONFIGS, ids=_ids)
def test_width_one_is_rollout(kind, d):
    c = _case(kind, d)
    r = c.store.beam_search(c.slots, _STEPS, width=1, temperature=_TEMP, exclude=c.excl, partitions=True)
    g = c.store.rollout(c.slots, _STEPS, exclude=c.excl, log_prob=True, temperature=_TEMP)
    assert np.array_equal(r.items[:, 0], g.items) and np.array_equal(_bits(r.scores[:, 0]), _bits(g.scores))
    assert np.array_equal(r.lengths, g.lengths)
    assert np.array_equal(_bits(r.shift[:, 0]), _bits(g.shift)) and np.array_equal(r.mass[:, 0], g.mass)
    fb = frac_bits(_ITEMS)
    want = np.full(_ROWS, -np.inf, np.float32)
    for i in range(_ROWS):
        if g.lengths[i]:
            cum = np.float32(0.0)
            for j in range(int(g.lengths[i])):
                cum = np.float32(cum + step_log_prob(g.scores[i, j], g.shift[i, j], log_mass(int(g.mass[i, j]), fb), _TEMP))
            want[i] = cum
    assert np.array_equal(_bits(r.log_probs[:, 0]), _bits(want))


# ---- 4. exhaustion ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 100)], ids=_ids)
def test_exhaustive_tree_of_six_items(kind, d):
    c = _case(kind, d)
    keep = [4, 5, 7, 9, 0, 998]  # planted: 5 is zero, 7 = 2 x 3, 9 = -3, 0 has duplicates elsewhere
    excl = [np.setdiff1d(np.arange(_ITEMS), keep)] * 3
    rows = [c.slots[3], c.slots[10], c.slots[11]]
    r = c.store.beam_search(rows, 2, width=32, temperature=_TEMP, exclude=excl)
    e = beam_expect(c.rep, c.scores, _ITEMS, [c.hist[3], c.hist[10], c.hist[11]], 2, 32, _TEMP, excl)
    _same(r, e, "exhaustive")
    assert r.beams.tolist() == [30] * 3 and r.lengths.tolist() == [2] * 3
    assert all(len({tuple(p) for p in r.items[i, :30].tolist()}) == 30 for i in range(3))


# ---- 5. partitions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", _CONFIGS, ids=_ids)
def test_partitions_per_beam_and_step(kind, d):
    c = _case(kind, d)
    e = c.expect("plain", 3)
    r = c.store.beam_search(c.slots, _STEPS, width=3, temperature=_TEMP, exclude=c.excl, partitions=True)
    _same(r, e, "partitions")
    assert r.frac_bits == int(_lib.load().sbr_softmax_frac_bits(_ITEMS))
    pad = r.items == NO_ITEM
    assert np.all(np.isneginf(r.shift[pad])) and np.all(r.mass[pad] == 0) and np.all(r.mass[~pad] >= np.uint64(2 ** r.frac_bits))


# ---- 6. nothing is written --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remember", [0, 3])
@pytest.mark.parametrize("kind,d", _SMALL, ids=_ids)
def test_the_store_is_untouched(kind, d, remember):
    c = _case(kind, d)
    n = 30
    slots = np.arange(n, dtype=np.uint32)[::-1].copy()
    st = c.g.sessions(n + 3, remember)
    st.append(slots, c.hist[:n])
    every = np.arange(n + 3, dtype=np.uint32)
    before = st.state(every)
    seen_before = st.seen(every) if remember else None
    st.beam_search(slots, _STEPS, width=4, temperature=_TEMP, exclude=c.excl[:n], partitions=True)
    after = st.state(every)
    assert np.array_equal(_bits(before[0]), _bits(after[0])) and np.array_equal(before[2], after[2])
    assert (before[1] is None) == (after[1] is None) and (before[1] is None or np.array_equal(_bits(before[1]), _bits(after[1])))
    if remember:
        assert all(np.array_equal(x, y) for x, y in zip(seen_before, st.seen(every)))
    st.close()


# ---- 7. invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", _SMALL, ids=_ids)
def test_the_same_bits_whatever_the_split(kind, d, monkeypatch):
    c = _case(kind, d)
    w = 3
    e = c.expect("plain", w)
    kw = dict(width=w, temperature=_TEMP, partitions=True)
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", "1")
    _same(c.store.beam_search(c.slots, _STEPS, exclude=c.excl, **kw), e, "one item range")
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", "3")
    monkeypatch.setenv("SBR_BEAM_CHUNK", "7")
    _same(c.store.beam_search(c.slots, _STEPS, exclude=c.excl, **kw), e, "chunks of 7")
    monkeypatch.delenv("SBR_BEAM_CHUNK")
    sub = np.random.RandomState(1).permutation(_ROWS)[:41]
    r = c.store.beam_search(c.slots[sub], _STEPS, exclude=[c.excl[i] for i in sub], **kw)
    p = Expected(0, w, _STEPS)
    for f in ("items", "scores", "step_lp", "shift", "mass", "cum", "lengths", "beams"):
        setattr(p, f, getattr(e, f)[sub])
    _same(r, p, "permuted subset")


# ---- 8. the scan's real chunk of 8 192 rows ---------------------------------------------------------------------------------
def test_the_real_chunk_of_8192_scan_rows_is_crossed():
    items, d, n, w, steps, distinct = 64, 16, 2100, 4, 2, 12
    g, o = _pair(NORMAL, d, items=items)
    rep, scores = _memo(o, items)
    rs = np.random.RandomState(8)
    base = [rs.randint(0, items, rs.randint(0, 6)) for _ in range(distinct)]
    base[2] = []
    st = g.sessions(n)
    slots = np.arange(n, dtype=np.uint32)
    hist = [base[i % distinct] for i in range(n)]
    st.append(slots, hist)
    r = st.beam_search(slots, steps, width=w, temperature=_TEMP, exclude=hist)
    st.close()
    e = beam_expect(rep, scores, items, base, steps, w, _TEMP, base)
    sample = np.r_[0:30, 2030:2100, rs.choice(n, 60, replace=False)]
    tile = sample % distinct
    assert np.array_equal(r.items[sample], e.items[tile]) and np.array_equal(_bits(r.scores[sample]), _bits(e.scores[tile]))
    assert np.array_equal(_bits(r.step_log_probs[sample]), _bits(e.step_lp[tile]))
    assert np.array_equal(_bits(r.log_probs[sample]), _bits(e.cum[tile]))
    assert np.array_equal(r.lengths[sample], e.lengths[tile]) and np.array_equal(r.beams[sample], e.beams[tile])


# ---- 9. poison --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0xFF, 0x7F, 0x80], ids=lambda p: f"poison{p:02X}")
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 16), (COUPLED, 100)], ids=_ids)
def test_on_poisoned_scratch(kind, d, pattern, monkeypatch):
    c = _case(kind, d)
    w = 3
    e = c.expect("plain", w)  # made without the device
    monkeypatch.setenv("SBR_TEST_POISON", str(pattern))
    monkeypatch.setenv("SBR_BEAM_CHUNK", "16")
    r = c.store.beam_search(c.slots, _STEPS, width=w, temperature=_TEMP, exclude=c.excl, partitions=True)
    _same(r, e, f"poison {pattern:#x}")


# ---- 10. errors -------------------------------------------------------------------------------------------------------------
def _raw(st, slots, steps, width=4, flags=0, temperature=1.0, any_of=None):
    L = _lib.load()
    sl = np.ascontiguousarray(slots, dtype=np.uint32)
    ba = _abi.SbrBeamArgs()
    ba.steps, ba.width, ba.flags, ba.temperature = steps, width, flags, temperature
    out = np.full((max(sl.size, 1), max(min(width, 64), 1), max(min(steps, 2000), 1)), 7, np.uint32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    status = L.sbr_sessions_beam_search(st._h, vp(sl), sl.size, C.byref(ba), None, None, vp(any_of), None, vp(out), *([None] * 8))
    assert np.all(out == 7)
    return status


def test_refusals_launch_nothing_and_change_nothing():
    g, _ = _pair(NORMAL, 16, items=300)
    st = g.sessions(8)
    slots = np.arange(6, dtype=np.uint32)
    st.append(slots, [[1, 2], [], [3], [4, 5, 6], [7], [8]])
    before, rec = st.state(slots), st.recommend(slots, 5)
    bad = [lambda: _raw(st, [0, 8], 3), lambda: _raw(st, [0, 2, 0], 3), lambda: _raw(st, slots, 0), lambda: _raw(st, slots, 1025),
           lambda: _raw(st, slots, 3, width=0), lambda: _raw(st, slots, 3, width=33),
           lambda: _raw(st, slots, 3, temperature=float("nan")), lambda: _raw(st, slots, 3, temperature=0.0),
           lambda: _raw(st, slots, 3, temperature=-2.0), lambda: _raw(st, slots, 3, flags=8),
           lambda: _raw(st, slots, 3, flags=_abi.ROLLOUT_SAMPLE),        # stochastic beam search is not built
           lambda: _raw(st, slots, 3, flags=_abi.ROLLOUT_INCLUDE_SEEN),  # a store without memory has nothing to include
           lambda: _raw(st, slots, 3, any_of=np.ones(6, np.uint32))]     # masks, and the model has no tags
    for i, call in enumerate(bad):
        assert call() == Status.INVALID_ARGUMENT, i
    with pytest.raises(EngineError) as err:
        st.beam_search(slots, 3, any_of=1)
    assert err.value.status == Status.INVALID_ARGUMENT

    def unchanged():
        after, rec2 = st.state(slots), st.recommend(slots, 5)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(before[:2], after[:2])) and np.array_equal(before[2], after[2])
        assert np.array_equal(rec[0], rec2[0]) and np.array_equal(_bits(rec[1]), _bits(rec2[1]))

    unchanged()
    assert np.array_equal(st.beam_search(slots, 1, width=5).items[:, :, 0], rec[0])  # the call itself works here: one step is the top 5
    unchanged()
    plan = g.fit_begin(*synthetic_interactions(24, 300, 12, seed=3))
    assert _raw(st, slots, 3) == Status.INVALID_ARGUMENT  # an open fit plan
    plan.close()
    assert _raw(st, slots, 3) == Status.INVALID_ARGUMENT  # stale: the plan may have stepped
    g.set_param(Param.ITEM_BIAS, g.get_param(Param.ITEM_BIAS))
    assert _raw(st, slots, 3) == Status.INVALID_ARGUMENT  # and stale by a parameter write
    st.close()


def test_a_non_finite_score_fails_the_whole_call():
    from sbr_rs_amd.errors import PredictionError

    g, _ = _pair(EWMA, 16, items=300)
    bias = g.get_param(Param.ITEM_BIAS)
    st = g.sessions(4)
    bias[77] = np.nan
    g.set_param(Param.ITEM_BIAS, bias)
    st.reset()
    st.append([0, 1], [[1], [2]])
    with pytest.raises(PredictionError.InvalidPredictionValue):
        st.beam_search([0, 1], 3, width=4)


# ---- 11. the Model form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 100)], ids=_ids)
def test_model_beam_search_is_its_definition(kind, d):
    c = _case(kind, d)
    hist = [c.hist[i] for i in range(20)] + [np.arange(30, dtype=np.uint32)]  # one longer than max_sequence_length
    T = int(c.g.hp.max_sequence_length)
    r = c.g.beam_search(hist, 4, width=3, temperature=_TEMP, partitions=True)
    st = c.g.sessions(len(hist))
    slots = np.arange(len(hist), dtype=np.uint32)
    st.append(slots, [h[-T:] for h in hist])
    w = st.beam_search(slots, 4, width=3, temperature=_TEMP, exclude=hist, partitions=True)
    st.close()
    for f in ("items", "lengths", "beams", "mass"):
        assert np.array_equal(getattr(r, f), getattr(w, f)), f
    for f in ("scores", "step_log_probs", "log_probs", "shift"):
        assert np.array_equal(_bits(getattr(r, f)), _bits(getattr(w, f))), f
