"""GPU: rollout and beam search within an item set (sbr_item_set_rollout / sbr_item_set_beam_search; rollout_advance_kernel and
beam_select_kernel with the set's ids, the unchanged scans over the set's sub-table).  The contract: a call through a set S returns,
bit for bit, what the store's own call returns with every item outside S appended to each row's exclusion list.  Every case is held
two ways, integers exactly and f32 by bits:

    exclusion  the store's own rollout / beam_search with the complement of S appended to every list
    numpy      rollout_expect / beam_expect over the oracle with the complement joined to every list

Shapes are test_item_set_gpu's and test_beam_gpu's: 1 000 items (32-item tiles, the last ragged), 70 slots (crossing the 64-row
tile at W = 1 and the beam-row tiles above), d = 16 and d = 100 (stored as 128), NORMAL, COUPLED and EWMA at d = 16 and NORMAL at
d = 100, SBR_CATALOGUE_GROUPS = 1 and 3, histories of at most 6 items and 5 steps, the sets {1, 31, 32, 33, every third item, all,
empty}.  The embeddings are test_beam_gpu._planted's, and items 50, 51 and 52 share one row and one bias: the small sets hold 50 and
52 but not 51, so a planted tie straddles the set."""
import ctypes as C
import functools

import numpy as np
import pytest

from beam_expect import beam_expect
from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM
from rollout_expect import rollout_expect
from sbr_rs_amd import _abi, _lib
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import PredictionError
from test_beam_gpu import _memo, _planted
from test_beam_gpu import _same as _same_beam_expect

pytestmark = pytest.mark.gpu

NORMAL, COUPLED, EWMA = ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA
ITEMS, ROWS, T, STEPS, TEMP, SEED = 1000, 70, 24, 5, 0.7, 41
SMALL = [(NORMAL, 16), (COUPLED, 16), (EWMA, 16), (NORMAL, 100)]
SET_NAMES = ["1", "31", "32", "33", "third", "all", "empty"]
_ids = lambda v: getattr(v, "name", str(v))  # noqa: E731


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _groups(monkeypatch):
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", "3")  # the scan reads the hook per call


@functools.lru_cache(maxsize=None)
def _sets():
    """name -> sorted unique ids.  The small ones hold 50 and 52 and leave 51 out: a tie group that straddles the set."""
    perm = np.random.RandomState(5).permutation(ITEMS)
    perm = perm[~np.isin(perm, (50, 51, 52))]
    out = {"1": np.array([52]), "empty": np.zeros(0)}
    for n in (31, 32, 33):
        out[str(n)] = np.sort(np.concatenate([[50, 52], perm[: n - 2]]))
    out["third"] = np.arange(0, ITEMS, 3)
    out["all"] = np.arange(ITEMS)
    return {k: v.astype(np.uint32) for k, v in out.items()}


def _pair(kind, d, items=ITEMS):
    """test_beam_gpu._pair's model and oracle, with items 50, 51 and 52 one planted row"""
    hp = hparams(items, T, d, int(kind), LOSS_HINGE, B=8)
    g, o = Model(hp), OracleModel(hp)
    E, bias = _planted(items, d, d + items)
    E[51] = E[52] = E[50]
    bias[51] = bias[52] = bias[50]
    rs = np.random.RandomState(int(kind) * 7 + d)
    extra = ({Param.EWMA_ALPHA: rs.randn(d)} if kind == EWMA else
             {Param.LSTM_W: rs.randn(2 * d, (4 if kind == NORMAL else 3) * d) * 0.3, Param.LSTM_B: rs.randn((4 if kind == NORMAL else 3) * d) * 0.5})
    for m in (g, o):
        m.set_param(Param.ITEM_EMBEDDING, E)
        m.set_param(Param.ITEM_BIAS, bias)
        for which, v in extra.items():
            m.set_param(which, v.astype(np.float32).ravel())
    return g, o


class _Case:
    """One configuration: the model pair, a store of 70 histories (an empty slot among them), the sets, tags and the memoised
    oracle.  The slots are not the rows' indices."""

    def __init__(self, kind, d):
        self.g, self.o = _pair(kind, d)
        rs = np.random.RandomState(d + int(kind))
        self.hist = [rs.randint(0, ITEMS, rs.randint(0, 7)).astype(np.uint32) for _ in range(ROWS)]
        self.hist[3] = np.zeros(0, np.uint32)
        self.tags = rs.randint(0, 16, ITEMS).astype(np.uint32)
        self.any_of = rs.randint(0, 16, ROWS).astype(np.uint32)
        self.none_of = 8
        self.g.set_item_tags(self.tags)
        self.slots = np.arange(ROWS, dtype=np.uint32) * 3 + 1
        self.store = self.g.sessions(3 * ROWS + 5)
        self.store.append(self.slots, self.hist)
        self.rep, self.scores = _memo(self.o, ITEMS)
        self.sets = {name: self.g.item_set(S) for name, S in _sets().items()}

    @functools.lru_cache(maxsize=None)
    def lists(self, name):
        """the caller's lists for set `name` — row 0 leaves 3 set items, row 1 nothing, row 2 is unsorted, row 3 empty — and the
        same with the complement of the set appended"""
        S = _sets()[name]
        rs = np.random.RandomState(S.size + 7)
        excl = [rs.randint(0, ITEMS, rs.randint(0, 30)).astype(np.uint32) for _ in range(ROWS)]
        keep = S[[0, S.size // 2, S.size - 1]] if S.size >= 3 else S
        excl[0] = np.setdiff1d(np.arange(ITEMS), keep).astype(np.uint32)
        excl[1] = np.arange(ITEMS, dtype=np.uint32)
        excl[2] = rs.permutation(ITEMS)[:900].astype(np.uint32)
        excl[3] = np.zeros(0, np.uint32)
        out = np.setdiff1d(np.arange(ITEMS), S).astype(np.uint32)
        return excl, [np.concatenate([x, out]) for x in excl]


@functools.lru_cache(maxsize=None)
def _case(kind, d):
    return _Case(kind, d)


def _same_rollout(r, x, what=""):
    """two Rollouts: every field the call returned"""
    assert np.array_equal(r.items, x.items), what
    assert np.array_equal(r.lengths, x.lengths), what
    assert np.array_equal(_bits(r.scores), _bits(x.scores)), what
    assert (r.keys is None) == (x.keys is None) and (r.keys is None or np.array_equal(_bits(r.keys), _bits(x.keys))), what
    assert (r.shift is None) == (x.shift is None), what
    if r.shift is not None:
        assert np.array_equal(_bits(r.shift), _bits(x.shift)) and np.array_equal(r.mass, x.mass) and r.frac_bits == x.frac_bits, what
        assert np.array_equal(r.log_prob.view(np.uint64), x.log_prob.view(np.uint64)), what
    assert (getattr(r, "h", None) is None) == (getattr(x, "h", None) is None), what
    if getattr(r, "h", None) is not None:
        assert np.array_equal(_bits(r.h), _bits(x.h)) and np.array_equal(r.len, x.len), what
        assert (r.c is None) == (x.c is None) and (r.c is None or np.array_equal(_bits(r.c), _bits(x.c))), what


def _same_rollout_expect(r, e, what=""):
    """a Rollout against rollout_expect's statement"""
    bad = np.argwhere(r.items != e.items)
    assert bad.size == 0, f"{what}: {len(bad)} items differ; first at {bad[0]}: {r.items[tuple(bad[0])]} vs {e.items[tuple(bad[0])]}"
    assert np.array_equal(r.lengths, e.lengths), what
    assert np.array_equal(_bits(r.scores), _bits(e.scores)), what
    if e.keys is not None:
        assert np.array_equal(_bits(r.keys), _bits(e.keys)), what
    if e.shift is not None:
        assert np.array_equal(_bits(r.shift), _bits(e.shift)) and np.array_equal(r.mass, e.mass), what


def _same_beams(r, x, what=""):
    """two Beams"""
    for f in ("items", "lengths", "beams"):
        assert np.array_equal(getattr(r, f), getattr(x, f)), (what, f)
    for f in ("scores", "step_log_probs", "log_probs"):
        assert np.array_equal(_bits(getattr(r, f)), _bits(getattr(x, f))), (what, f)
    assert (r.shift is None) == (x.shift is None), what
    if r.shift is not None:
        assert np.array_equal(_bits(r.shift), _bits(x.shift)) and np.array_equal(r.mass, x.mass) and r.frac_bits == x.frac_bits, what


# ---- 1. rollout, greedy and sampled, against both routes ---------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("kind,d", SMALL, ids=_ids)
def test_rollout_is_the_complement_route(kind, d, name, groups, monkeypatch):
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", str(groups))
    c = _case(kind, d)
    S, on = _sets()[name], c.sets[name].on(c.store)
    excl, joined = c.lists(name)
    for mode in ("greedy", "sample"):
        kw = dict(mode=mode, temperature=TEMP, seed=SEED, log_prob=True, final_state=True)
        r = on.rollout(c.slots, STEPS, exclude=excl, **kw)
        _same_rollout(r, c.store.rollout(c.slots, STEPS, exclude=joined, **kw), f"S={name} {mode}: exclusion route")
        assert r.frac_bits == int(_lib.load().sbr_softmax_frac_bits(ITEMS))  # the model's F, not one of |S|
        assert np.all(np.isin(r.items[r.items != NO_ITEM], S))
        if S.size >= 3:
            assert r.lengths[0] == 3
        assert r.lengths[1] == 0 and np.all(r.items[1] == NO_ITEM)
        if S.size == 0:  # every row ends at step 0, and the final state is the slots' current one
            h, cc, ln = c.store.state(c.slots)
            assert np.all(r.lengths == 0) and np.all(r.items == NO_ITEM) and np.all(r.mass == 0)
            assert np.array_equal(_bits(r.h), _bits(h)) and np.array_equal(r.len, ln)
            assert (cc is None) == (r.c is None) and (cc is None or np.array_equal(_bits(r.c), _bits(cc)))
        if groups == 3:  # the numpy statement does not depend on the scan's item ranges
            e = rollout_expect(c.rep, c.scores, ITEMS, c.hist, STEPS, joined, partition_temperature=TEMP,
                               sample=None if mode == "greedy" else (TEMP, SEED), streams=c.slots)
            _same_rollout_expect(r, e, f"S={name} {mode}: numpy route")


# ---- 2. beam search, W in {1, 4}, against both routes ------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("kind,d", SMALL, ids=_ids)
def test_beam_search_is_the_complement_route(kind, d, name, groups, monkeypatch):
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", str(groups))
    c = _case(kind, d)
    S, on = _sets()[name], c.sets[name].on(c.store)
    excl, joined = c.lists(name)
    for w in (1, 4):
        r = on.beam_search(c.slots, STEPS, width=w, temperature=TEMP, exclude=excl, partitions=True)
        _same_beams(r, c.store.beam_search(c.slots, STEPS, width=w, temperature=TEMP, exclude=joined, partitions=True),
                    f"S={name} W={w}: exclusion route")
        assert r.frac_bits == int(_lib.load().sbr_softmax_frac_bits(ITEMS))
        assert np.all(np.isin(r.items[r.items != NO_ITEM], S))
        if S.size >= 3:
            assert r.lengths[0] == 3 and r.beams[0] == min(w, 6)
        assert r.beams[1] == 0 and r.lengths[1] == 0
        if S.size == 0:
            assert np.all(r.beams == 0) and np.all(r.lengths == 0) and np.all(r.items == NO_ITEM)
        if groups == 3:
            _same_beam_expect(r, beam_expect(c.rep, c.scores, ITEMS, c.hist, STEPS, w, TEMP, joined), f"S={name} W={w}: numpy route")


# ---- 3. repeats, tag masks, the seen-item memory -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33", "third"])
@pytest.mark.parametrize("kind,d", SMALL, ids=_ids)
def test_repeats_tags_and_seen_memory(kind, d, name):
    c = _case(kind, d)
    S, s = _sets()[name], c.sets[name]
    rows = 24
    excl, joined = c.lists(name)
    excl, joined, slots, hist = excl[:rows], joined[:rows], c.slots[:rows], c.hist[:rows]
    on = s.on(c.store)
    variants = {"repeats": (dict(allow_repeats=True), dict(allow_repeats=True)),
                "tags": (dict(any_of=c.any_of[:rows], none_of=c.none_of), dict(tags=c.tags, any_of=c.any_of[:rows], none_of=c.none_of))}
    for what, (kw, ekw) in variants.items():
        for mode in ("greedy", "sample"):
            r = on.rollout(slots, STEPS, mode=mode, temperature=TEMP, seed=SEED, exclude=excl, log_prob=True, **kw)
            _same_rollout(r, c.store.rollout(slots, STEPS, mode=mode, temperature=TEMP, seed=SEED, exclude=joined, log_prob=True, **kw),
                          f"{what} {mode}")
            e = rollout_expect(c.rep, c.scores, ITEMS, hist, STEPS, joined, partition_temperature=TEMP,
                               sample=None if mode == "greedy" else (TEMP, SEED), streams=slots, **ekw)
            _same_rollout_expect(r, e, f"{what} {mode}: numpy")
        for w in (1, 4):
            r = on.beam_search(slots, STEPS, width=w, temperature=TEMP, exclude=excl, partitions=True, **kw)
            _same_beams(r, c.store.beam_search(slots, STEPS, width=w, temperature=TEMP, exclude=joined, partitions=True, **kw), f"{what} W={w}")
            _same_beam_expect(r, beam_expect(c.rep, c.scores, ITEMS, hist, STEPS, w, TEMP, joined, **ekw), f"{what} W={w}: numpy")
    # a store with memory (remember = 8): its ring's items join X_0 unless include_seen
    st = c.g.sessions(rows, 8)
    mslots = np.arange(rows, dtype=np.uint32)[::-1].copy()
    st.append(mslots, hist)
    seen = st.seen(mslots)
    full = [np.concatenate([joined[i].astype(np.int64), seen[i].astype(np.int64)]) for i in range(rows)]
    son = s.on(st)
    for include_seen in (False, True):
        lists = joined if include_seen else full
        for mode in ("greedy", "sample"):
            r = son.rollout(mslots, STEPS, mode=mode, temperature=TEMP, seed=SEED, exclude=excl, include_seen=include_seen, log_prob=True,
                            final_state=True)
            _same_rollout(r, st.rollout(mslots, STEPS, mode=mode, temperature=TEMP, seed=SEED, exclude=joined, include_seen=include_seen,
                                        log_prob=True, final_state=True), f"seen={not include_seen} {mode}")
            e = rollout_expect(c.rep, c.scores, ITEMS, hist, STEPS, lists, partition_temperature=TEMP,
                               sample=None if mode == "greedy" else (TEMP, SEED), streams=mslots)
            _same_rollout_expect(r, e, f"seen={not include_seen} {mode}: numpy")
        for w in (1, 4):
            r = son.beam_search(mslots, STEPS, width=w, temperature=TEMP, exclude=excl, include_seen=include_seen, partitions=True)
            _same_beams(r, st.beam_search(mslots, STEPS, width=w, temperature=TEMP, exclude=joined, include_seen=include_seen, partitions=True),
                        f"seen={not include_seen} W={w}")
            _same_beam_expect(r, beam_expect(c.rep, c.scores, ITEMS, hist, STEPS, w, TEMP, lists), f"seen={not include_seen} W={w}: numpy")
    st.close()
    if name == "third":  # the memory holds set items: its merge is turned into positions of the set
        assert np.any(np.isin(np.concatenate([x for x in seen]), S))


# ---- 4. the widest beam ------------------------------------------------------------------------------------------------------
def test_width_32():
    c = _case(NORMAL, 16)
    name, rows = "33", 12
    excl, joined = c.lists(name)
    on = c.sets[name].on(c.store)
    r = on.beam_search(c.slots[:rows], 3, width=32, temperature=TEMP, exclude=excl[:rows], partitions=True)
    _same_beams(r, c.store.beam_search(c.slots[:rows], 3, width=32, temperature=TEMP, exclude=joined[:rows], partitions=True), "W=32")
    _same_beam_expect(r, beam_expect(c.rep, c.scores, ITEMS, c.hist[:rows], 3, 32, TEMP, joined[:rows]), "W=32: numpy")
    assert r.beams[0] == 6 and r.lengths[0] == 3 and r.beams[3] == 32  # row 3: no list, 33 items


# ---- 5. the chunks give the one-chunk bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33", "all"])
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 100)], ids=_ids)
def test_chunks(kind, d, name, monkeypatch):
    c = _case(kind, d)
    on = c.sets[name].on(c.store)
    excl, _ = c.lists(name)
    kw = dict(temperature=TEMP, seed=SEED, exclude=excl, log_prob=True, final_state=True)
    one = [on.rollout(c.slots, STEPS, mode=m, **kw) for m in ("greedy", "sample")]
    beams = on.beam_search(c.slots, STEPS, width=4, temperature=TEMP, exclude=excl, partitions=True)
    monkeypatch.setenv("SBR_ROLLOUT_CHUNK", "7")
    monkeypatch.setenv("SBR_BEAM_CHUNK", "3")
    for m, want in zip(("greedy", "sample"), one):
        _same_rollout(on.rollout(c.slots, STEPS, mode=m, **kw), want, f"rollout chunks of 7, {m}")
    _same_beams(on.beam_search(c.slots, STEPS, width=4, temperature=TEMP, exclude=excl, partitions=True), beams, "beam chunks of 3")


# ---- 6. poisoned scratch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0xFF, 0x7F], ids=lambda p: f"poison{p:02X}")
def test_on_poisoned_scratch(pattern, monkeypatch):
    c = _case(COUPLED, 16)
    name = "32"
    on = c.sets[name].on(c.store)
    excl, _ = c.lists(name)
    kw = dict(temperature=TEMP, seed=SEED, exclude=excl, log_prob=True, final_state=True)
    want = [on.rollout(c.slots, STEPS, mode=m, **kw) for m in ("greedy", "sample")]
    wb = on.beam_search(c.slots, STEPS, width=4, temperature=TEMP, exclude=excl, partitions=True)
    monkeypatch.setenv("SBR_TEST_POISON", str(pattern))
    for m, w in zip(("greedy", "sample"), want):
        _same_rollout(on.rollout(c.slots, STEPS, mode=m, **kw), w, f"poison {pattern:#x} {m}")
    _same_beams(on.beam_search(c.slots, STEPS, width=4, temperature=TEMP, exclude=excl, partitions=True), wb, f"poison {pattern:#x} beam")


# ---- 7. rows outside the set are never read ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [NORMAL, EWMA], ids=_ids)
def test_a_non_finite_row_outside_the_set_fails_nothing(kind):
    """NaN rows outside S (51, tied with 50 and 52; 1; a bias) leave the set's results bit-identical to those of the same model with
    every row finite; a NaN row inside S fails the call.  Item 0 stays finite: it is the model's own padding row, which the
    empty-history state is made from.  S leaves 0 out, so the stand-in feed of an ended row is a set item (ids[0] = 3)."""
    S = np.array([3, 7, 9, 50, 52, 120, 299], dtype=np.uint32)
    slots = np.arange(5, dtype=np.uint32)
    hist = [[4, 2], [], [3], [52, 7], [200]]
    excl = [[], [], [3, 7, 9, 50, 52, 120], [], []]  # row 2 ends after one step
    g, _ = _pair(kind, 16, items=300)
    ref, _ = _pair(kind, 16, items=300)  # the same model, every row finite
    E, b = g.get_param(Param.ITEM_EMBEDDING).reshape(300, 16), g.get_param(Param.ITEM_BIAS)
    E[[1, 51], 0] = np.nan
    b[5] = np.nan
    g.set_param(Param.ITEM_EMBEDDING, E)
    g.set_param(Param.ITEM_BIAS, b)

    def calls(model):
        s, st = model.item_set(S), model.sessions(6)
        st.append(slots, hist)
        on = s.on(st)
        out = ([on.rollout(slots, 4, mode=m, temperature=TEMP, exclude=excl, log_prob=True, final_state=True) for m in ("greedy", "sample")],
               on.beam_search(slots, 4, width=4, temperature=TEMP, exclude=excl, partitions=True))
        return out, s, st

    (rolls, beams), s, st = calls(g)
    (want, wbeams), s2, st2 = calls(ref)
    for r, w, m in zip(rolls, want, ("greedy", "sample")):
        _same_rollout(r, w, f"NaN outside S {m}")
    _same_beams(beams, wbeams, "NaN outside S beam")
    assert rolls[0].lengths[2] == 1 and beams.lengths[2] == 1
    E[50, 0] = np.nan  # now a row inside S
    g.set_param(Param.ITEM_EMBEDDING, E)
    with pytest.raises(ValueError):  # stale: every call through the set is refused until refresh()
        s.on(st).rollout(slots, 2)
    s.refresh()
    st.reset()
    st.append(slots, hist)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        s.on(st).rollout(slots, 3)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        s.on(st).beam_search(slots, 3, width=2)
    for x in (st, st2, s, s2, g, ref):
        x.close()


# ---- 8. the whole catalogue is the plain call --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(COUPLED, 16), (NORMAL, 100)], ids=_ids)
def test_the_set_of_all_items_is_the_plain_call(kind, d):
    c = _case(kind, d)
    on = c.sets["all"].on(c.store)
    for m in ("greedy", "sample"):
        kw = dict(mode=m, temperature=TEMP, seed=SEED, log_prob=True, final_state=True)
        _same_rollout(on.rollout(c.slots, STEPS, **kw), c.store.rollout(c.slots, STEPS, **kw), f"all {m}")
    for w in (1, 4):
        _same_beams(on.beam_search(c.slots, STEPS, width=w, temperature=TEMP, partitions=True),
                    c.store.beam_search(c.slots, STEPS, width=w, temperature=TEMP, partitions=True), f"all W={w}")


# ---- 9. the histories forms are their definitions ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 100)], ids=_ids)
def test_histories_forms_are_their_definitions(kind, d):
    c = _case(kind, d)
    s = c.sets["third"]
    hist = [c.hist[i] for i in range(20)] + [np.arange(30, dtype=np.uint32)]  # one longer than max_sequence_length
    Tm = int(c.g.hp.max_sequence_length)
    st = c.g.sessions(len(hist))
    slots = np.arange(len(hist), dtype=np.uint32)
    st.append(slots, [h[-Tm:] for h in hist])
    for m in ("greedy", "sample"):
        kw = dict(mode=m, temperature=TEMP, seed=SEED, log_prob=True, final_state=True)
        _same_rollout(s.rollout(hist, 4, **kw), s.on(st).rollout(slots, 4, exclude=hist, **kw), f"histories {m}")
    _same_beams(s.beam_search(hist, 4, width=3, temperature=TEMP, partitions=True),
                s.on(st).beam_search(slots, 4, width=3, temperature=TEMP, exclude=hist, partitions=True), "histories beam")
    st.close()


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------
def _raw(fn, s, desc, n, args, keys=False):
    """one entry call through ctypes; nothing may be written"""
    out = np.full(64, 7, np.uint32)
    kout = np.full(64, 7, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tail = [None] * 8
    if keys:
        tail[1] = vp(kout)  # out_keys
    status = fn(s._h, C.byref(desc), n, C.byref(args), vp(out), *tail)
    assert np.all(out == 7) and np.all(kout == 7)
    return status


def test_refusals_launch_nothing_and_write_nothing():
    L = _lib.load()
    g, _ = _pair(NORMAL, 16, items=300)
    other, _ = _pair(NORMAL, 16, items=300)
    s = g.item_set([0, 3, 50, 52, 120])
    st, st_other = g.sessions(8), other.sessions(8)
    slots = np.arange(4, dtype=np.uint32)
    st.append(slots, [[1, 2], [], [3], [4, 5, 6]])
    st_other.append(slots, [[1], [2], [3], [4]])
    ra = _abi.SbrRolloutArgs()
    ra.steps, ra.sample.temperature = 3, 1.0
    ba = _abi.SbrBeamArgs()
    ba.steps, ba.width, ba.temperature = 3, 2, 1.0

    def desc(store=st, **kw):
        d = _abi.SbrScanRows()
        d.store, d.slots = store._h.value, slots.ctypes.data
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    up = np.array([0, 1, 2, 3, 4], dtype=np.uint64)
    reps = np.zeros((4, 16), dtype=np.float32)
    bad = [desc(user_ptr=up.ctypes.data, item_ids=slots.ctypes.data), desc(reps=reps.ctypes.data), desc(flags=1),
           desc(store=st_other)]
    hist = _abi.SbrScanRows()
    hist.user_ptr, hist.item_ids = up.ctypes.data, slots.ctypes.data
    bad.append(hist)  # histories alone, no store
    for i, d in enumerate(bad):
        assert _raw(L.sbr_item_set_rollout, s, d, 4, ra) == Status.INVALID_ARGUMENT, i
        assert _raw(L.sbr_item_set_beam_search, s, d, 4, ba) == Status.INVALID_ARGUMENT, i
    assert _raw(L.sbr_item_set_rollout, s, desc(), 4, ra, keys=True) == Status.INVALID_ARGUMENT  # a greedy pick has no key
    assert s.on(st).rollout(slots, 3).items.shape == (4, 3)  # the descriptor itself is good
    # a stale set after set_param, and success after refresh() plus store.reset()
    g.set_param(Param.ITEM_BIAS, g.get_param(Param.ITEM_BIAS))
    st.reset()
    st.append(slots, [[1, 2], [], [3], [4, 5, 6]])
    assert _raw(L.sbr_item_set_rollout, s, desc(), 4, ra) == Status.INVALID_ARGUMENT
    assert _raw(L.sbr_item_set_beam_search, s, desc(), 4, ba) == Status.INVALID_ARGUMENT
    s.refresh()
    want = st.rollout(slots, 3, exclude=[np.setdiff1d(np.arange(300), [0, 3, 50, 52, 120])] * 4)
    _same_rollout(s.on(st).rollout(slots, 3), want, "after refresh")
    plan = g.fit_begin(*synthetic_interactions(24, 300, 12, seed=3))
    assert _raw(L.sbr_item_set_rollout, s, desc(), 4, ra) == Status.INVALID_ARGUMENT  # an open fit plan
    assert _raw(L.sbr_item_set_beam_search, s, desc(), 4, ba) == Status.INVALID_ARGUMENT
    plan.close()
    for x in (st, st_other, s, g, other):
        x.close()
