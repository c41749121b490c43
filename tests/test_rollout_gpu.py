"""GPU: sbr_sessions_rollout (rollout_advance_kernel and its neighbours in sbr_sessions.hip) against the contract stated in
rollout_expect.py over the oracle's representations and scores, and against the host loop it replaces — recommend(k = 1) + append +
a rebuilt exclusion list — on a second store.  Everything is an equality: ids and lengths as integers, f32 by bits, masses as
integers.  1 000 items (32 item tiles, the last ragged), 130 rows (the second row tile nearly empty), d = 16 and d = 100 (stored as
128), SBR_CATALOGUE_GROUPS=3.  Embeddings are planted as in test_capped_gpu (duplicate rows, biases on a 0.1 grid), so ties decide
picks and the duplicate of a picked item is the natural next pick.  An expectation is computed once per configuration at 17 steps
and shared; fewer steps are its prefix, which is the contract's own statement (X_j depends on picks 0 .. j - 1 only)."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM
from rollout_expect import Expected, oracle_callables, rollout_expect
from sampled_expect import inv_temperature, keys_of, noise
from sbr_rs_amd import _abi, _lib
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model, Partition
from sbr_rs_amd.errors import EngineError

pytestmark = pytest.mark.gpu

NORMAL, COUPLED, EWMA = ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA
_ITEMS, _ROWS, _T, _STEPS = 1000, 130, 24, 17  # histories of at most 6 items + 17 steps stay inside the oracle's window
_CONFIGS = [(k, d) for d in (16, 100) for k in (NORMAL, COUPLED, EWMA)]
_SMALL = [(NORMAL, 16), (COUPLED, 16), (EWMA, 16), (NORMAL, 100)]
_ids = lambda v: getattr(v, "name", str(v))  # noqa: E731
_TEMP, _SEED = 0.7, 2 ** 64 - 3  # the seed wraps at step 3


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


def _prefix(e: Expected, steps, rows=None) -> Expected:
    rows = slice(None) if rows is None else rows
    p = Expected(0, steps, e.keys is not None, e.shift is not None)
    p.items, p.scores = e.items[rows, :steps], e.scores[rows, :steps]
    p.lengths = np.minimum(e.lengths[rows], steps).astype(np.uint32)
    p.keys = None if e.keys is None else e.keys[rows, :steps]
    p.shift = None if e.shift is None else e.shift[rows, :steps]
    p.mass = None if e.mass is None else e.mass[rows, :steps]
    return p


class _Case:
    """One configuration: the model pair, a store holding 130 histories (an empty slot, a row left with 3 items, a row that may see
    nothing among them), and the memoised oracle."""

    def __init__(self, kind, d):
        self.kind, self.d = kind, d
        self.g, self.o = _pair(kind, d)
        rs = np.random.RandomState(d + int(kind))
        self.hist = [rs.randint(0, _ITEMS, rs.randint(0, 7)).astype(np.uint32) for _ in range(_ROWS)]
        self.hist[3] = np.zeros(0, np.uint32)  # an empty slot
        self.excl = [rs.randint(0, _ITEMS, rs.randint(0, 30)) for _ in range(_ROWS)]
        self.excl[0] = np.delete(np.arange(_ITEMS), [17, 500, 999])  # three real entries, then padding
        self.excl[1] = np.arange(_ITEMS)                             # may see nothing
        self.excl[2] = np.arange(_ITEMS)[::-1][:-1]                  # one item, unsorted list
        self.excl[3] = []
        self.tags = rs.randint(0, 16, _ITEMS).astype(np.uint32)
        self.any_of = rs.randint(0, 16, _ROWS).astype(np.uint32)
        self.none_of = 8
        self.g.set_item_tags(self.tags)
        self.slots = (np.arange(_ROWS, dtype=np.uint32) * 3 + 1)  # not the identity: a slot is not a row
        self.store = self.g.sessions(3 * _ROWS + 5)
        self.store.append(self.slots, self.hist)
        rep, scores = oracle_callables(self.o, _ITEMS)
        memo = {}

        def scores_of(hist):
            key = tuple(int(x) for x in hist)
            if key not in memo:
                memo[key] = scores(rep(list(key)))
            return memo[key]

        self.rep, self.scores = (lambda hist: hist), scores_of  # the "representation" handed on is the history: scores_of memoises on it

    @functools.lru_cache(maxsize=None)
    def expect(self, variant, rows=_ROWS, steps=_STEPS):
        kw = {"greedy": dict(partition_temperature=_TEMP),
              "sample": dict(sample=(_TEMP, _SEED), streams=self.slots[:rows].astype(np.uint64), partition_temperature=_TEMP),
              "tags": dict(tags=self.tags, any_of=self.any_of[:rows], none_of=self.none_of),
              "repeats": dict(allow_repeats=True)}[variant]
        return rollout_expect(self.rep, self.scores, _ITEMS, self.hist[:rows], steps, self.excl[:rows], **kw)


@functools.lru_cache(maxsize=None)
def _case(kind, d):
    return _Case(kind, d)


def _same(r, e: Expected, what=""):
    bad = np.argwhere(r.items != e.items)
    assert bad.size == 0, f"{what}: {len(bad)} items differ; first at {bad[0]}: {r.items[tuple(bad[0])]} vs {e.items[tuple(bad[0])]}"
    assert np.array_equal(_bits(r.scores), _bits(e.scores)), what
    assert np.array_equal(r.lengths, e.lengths), what
    if e.keys is not None and r.keys is not None:
        assert np.array_equal(_bits(r.keys), _bits(e.keys)), what
    if e.shift is not None and r.shift is not None:
        assert np.array_equal(_bits(r.shift), _bits(e.shift)), what
        assert np.array_equal(r.mass, e.mass), what


# ---- 1. greedy against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 17])
@pytest.mark.parametrize("kind,d", _CONFIGS, ids=_ids)
def test_greedy_is_the_contract_over_the_oracle(kind, d, steps):
    c = _case(kind, d)
    e = _prefix(c.expect("greedy"), steps)
    r = c.store.rollout(c.slots, steps, exclude=c.excl)
    _same(r, e, "greedy")
    assert r.keys is None and r.shift is None and r.log_prob is None and r.h is None
    assert e.lengths[:4].tolist() == [min(3, steps), 0, 1, steps]
    if steps >= 5:
        assert sorted(r.items[0, :3].tolist()) == [17, 500, 999] and np.all(r.items[0, 3:] == NO_ITEM) and np.all(np.isneginf(r.scores[0, 3:]))


@pytest.mark.parametrize("kind,d", _SMALL, ids=_ids)
def test_greedy_with_tag_masks_and_with_repeats(kind, d):
    c = _case(kind, d)
    rows, steps = 24, 5
    r = c.store.rollout(c.slots[:rows], steps, exclude=c.excl[:rows], any_of=c.any_of[:rows], none_of=c.none_of)
    _same(r, c.expect("tags", rows, steps), "tags")
    r = c.store.rollout(c.slots[:rows], steps, exclude=c.excl[:rows], allow_repeats=True)
    e = c.expect("repeats", rows, steps)
    _same(r, e, "repeats")
    assert e.lengths[:3].tolist() == [steps, 0, steps]
    assert len(set(r.items[2].tolist())) == 1  # one eligible item, picked at every step
    # nothing excluded at all: the scan runs without an exclusion CSR
    r = c.store.rollout(c.slots[:rows], 2, allow_repeats=True)
    _same(r, rollout_expect(c.rep, c.scores, _ITEMS, c.hist[:rows], 2, None, allow_repeats=True), "bare")


# ---- 2. against the host loop it replaces ----------------------------------------------------------------------------------------
def _host_loop(st, slots, steps, excl, *, sample=None, streams=None, any_of=None, none_of=None, allow_repeats=False, include_seen=False,
               log_prob=None):
    """recommend(k = 1) + append + a rebuilt exclude, `steps` times, on the store `st` (which it changes).  X_0 is fixed at call
    time: what the store remembers then is passed on as a list, because the loop's own appends would push it out of a ring."""
    n = len(slots)
    barred = [set(int(x) for x in (excl[i] if excl is not None else ())) for i in range(n)]
    if st.seen_capacity and not include_seen:
        for i, seen in enumerate(st.seen(slots)):
            barred[i] |= set(int(x) for x in seen)
    flag = dict(include_seen=True) if st.seen_capacity else {}
    e = Expected(n, steps, sample is not None, log_prob is not None)
    live = np.ones(n, dtype=bool)
    for j in range(steps):
        lists = [sorted(b) for b in barred]
        if sample is None:
            it, sc = st.recommend(slots, 1, exclude=lists, any_of=any_of, none_of=none_of, **flag)
        else:
            it, sc, ky = st.recommend_sampled(slots, 1, temperature=sample[0], seed=(sample[1] + j) % 2 ** 64, streams=streams, exclude=lists,
                                              any_of=any_of, none_of=none_of, **flag)
        if log_prob is not None:
            part = st.log_partition(slots, log_prob, exclude=lists, any_of=any_of, none_of=none_of, **flag)
        got = live & (it[:, 0] != NO_ITEM)
        e.lengths[live & ~got] = j
        live = got
        for i in np.flatnonzero(live):
            e.items[i, j], e.scores[i, j] = it[i, 0], sc[i, 0]
            if sample is not None:
                e.keys[i, j] = ky[i, 0]
            if log_prob is not None:
                e.shift[i, j], e.mass[i, j] = part.shift[i], part.mass[i]
            if not allow_repeats:
                barred[i].add(int(it[i, 0]))
        st.append(slots, [[int(it[i, 0])] if live[i] else [] for i in range(n)])
    return e


_LOOPS = [(r, m) for r in (0, 4) for m in ("greedy", "sample", "tags", "repeats", "partition")] + [(4, "keep_seen")]


@pytest.mark.parametrize("remember,mode", _LOOPS)
@pytest.mark.parametrize("kind,d", _SMALL, ids=_ids)
def test_rollout_is_the_host_loop(kind, d, remember, mode):
    c = _case(kind, d)
    n, steps = 40, 6
    rs = np.random.RandomState(5)
    hist = [rs.randint(0, _ITEMS, rs.randint(0, 10)) for _ in range(n)]  # up to 9 appended items: a ring of 4 has wrapped
    hist[0] = rs.randint(0, _ITEMS, _T + 16)  # longer than max_sequence_length: a session keeps the whole recurrence
    hist[1] = []
    slots = rs.permutation(2 * n)[:n].astype(np.uint32)
    excl = c.excl[:n]
    a, b = c.g.sessions(2 * n, remember), c.g.sessions(2 * n, remember)
    for st in (a, b):
        st.append(slots, hist)
    kw = dict(include_seen=mode == "keep_seen")
    lkw = dict(kw)
    if mode == "sample":
        kw.update(mode="sample", temperature=_TEMP, seed=_SEED)
        lkw.update(sample=(_TEMP, _SEED))
    if mode == "tags":
        kw.update(any_of=c.any_of[:n], none_of=c.none_of)
        lkw.update(any_of=c.any_of[:n], none_of=c.none_of)
    if mode == "repeats":
        kw.update(allow_repeats=True)
        lkw.update(allow_repeats=True)
    if mode == "partition":
        kw.update(log_prob=True, temperature=_TEMP)
        lkw.update(log_prob=_TEMP)
    r = a.rollout(slots, steps, exclude=excl, final_state=True, **kw)
    e = _host_loop(b, slots, steps, excl, **lkw)
    _same(r, e, mode)
    # the loop made it happen on b; the rollout's final state is b's state now, and a is where it was
    h, cc, ln = b.state(slots)
    assert np.array_equal(_bits(r.h), _bits(h)) and np.array_equal(r.len, ln)
    assert (cc is None and r.c is None) or np.array_equal(_bits(r.c), _bits(cc))
    a.close()
    b.close()


# ---- 3. sampled ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", _CONFIGS, ids=_ids)
def test_sampled_is_the_contract_and_one_step_is_recommend_sampled(kind, d, monkeypatch):
    c = _case(kind, d)
    e = c.expect("sample")
    r = c.store.rollout(c.slots, _STEPS, mode="sample", temperature=_TEMP, seed=_SEED, exclude=c.excl, log_prob=True)
    _same(r, e, "sample")
    one = c.store.rollout(c.slots, 1, mode="sample", temperature=_TEMP, seed=_SEED, exclude=c.excl)
    it, sc, ky = c.store.recommend_sampled(c.slots, 1, temperature=_TEMP, seed=_SEED, exclude=c.excl)
    assert np.array_equal(one.items, it) and np.array_equal(_bits(one.scores), _bits(sc)) and np.array_equal(_bits(one.keys), _bits(ky))
    # the same (seed, streams) gives the same rows under another batch order, other chunks and another item-range split
    perm = np.random.RandomState(1).permutation(_ROWS)
    kw = dict(mode="sample", temperature=_TEMP, seed=_SEED)
    p = c.store.rollout(c.slots[perm], _STEPS, exclude=[c.excl[i] for i in perm], **kw)
    _same(p, _prefix(e, _STEPS, perm), "permuted")
    monkeypatch.setenv("SBR_ROLLOUT_CHUNK", "64")
    _same(c.store.rollout(c.slots, _STEPS, exclude=c.excl, **kw), e, "chunks of 64")
    monkeypatch.delenv("SBR_ROLLOUT_CHUNK")
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", "1")
    _same(c.store.rollout(c.slots, _STEPS, exclude=c.excl, **kw), e, "one item range")


def test_a_step_has_noise_of_its_own():
    items = np.arange(_ITEMS, dtype=np.uint32)
    g0 = noise(_SEED, np.array([4], np.uint64), items)[0]
    g1 = noise((_SEED + 1) % 2 ** 64, np.array([4], np.uint64), items)[0]
    assert np.count_nonzero(_bits(g0) != _bits(g1)) > _ITEMS * 0.99
    # and on the device: row 2 may see item 0 alone, so with repeats every step draws it — under the noise of seed + j
    c = _case(EWMA, 16)
    steps = 4
    r = c.store.rollout(c.slots[2:3], steps, mode="sample", temperature=_TEMP, seed=_SEED, exclude=[c.excl[2]], allow_repeats=True)
    assert r.items[0].tolist() == [0] * steps
    stream = np.array([c.slots[2]], np.uint64)
    g = np.array([noise((_SEED + j) % 2 ** 64, stream, items[:1])[0, 0] for j in range(steps)], np.float32)
    assert len(set(_bits(g).tolist())) == steps
    assert np.array_equal(_bits(r.keys[0]), _bits(keys_of(r.scores[0], inv_temperature(_TEMP), g)))


# ---- 4. partition -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [2, 17])
@pytest.mark.parametrize("kind,d", _CONFIGS, ids=_ids)
def test_partition_per_step(kind, d, steps):
    c = _case(kind, d)
    e = _prefix(c.expect("greedy"), steps)
    r = c.store.rollout(c.slots, steps, exclude=c.excl, log_prob=True, temperature=_TEMP)
    _same(r, e, "partition")
    assert r.frac_bits == int(_lib.load().sbr_softmax_frac_bits(_ITEMS))
    want = Partition(_TEMP, e.shift.reshape(-1), e.mass.reshape(-1), r.frac_bits).log_prob(e.scores.reshape(-1, 1)).reshape(_ROWS, steps)
    pad = e.items == NO_ITEM
    assert np.array_equal(np.isnan(r.log_prob), pad) and np.array_equal(r.log_prob[~pad], want[~pad])
    assert np.all(np.isneginf(r.shift[pad])) and np.all(r.mass[pad] == 0) and pad[1].all() and pad[0, 3:].all()
    assert np.all(r.log_prob[~pad] <= 0)


# ---- 5. nothing is written ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("remember", [0, 6])
@pytest.mark.parametrize("kind,d", _SMALL, ids=_ids)
def test_a_rollout_writes_nothing_and_its_final_state_is_the_append(kind, d, remember, mode):
    c = _case(kind, d)
    n, steps = 50, 7
    slots = np.arange(n, dtype=np.uint32)[::-1].copy()
    st = c.g.sessions(n + 3, remember)
    st.append(slots, c.hist[:n])
    every = np.arange(n + 3, dtype=np.uint32)
    before = st.state(every)
    seen_before = st.seen(every) if remember else None
    r = st.rollout(slots, steps, mode=mode, temperature=_TEMP, seed=9, exclude=c.excl[:n], final_state=True, log_prob=True)
    after = st.state(every)
    assert np.array_equal(_bits(before[0]), _bits(after[0])) and np.array_equal(before[2], after[2])
    assert (before[1] is None) == (after[1] is None) and (before[1] is None or np.array_equal(_bits(before[1]), _bits(after[1])))
    if remember:
        assert all(np.array_equal(x, y) for x, y in zip(seen_before, st.seen(every)))
    assert r.lengths[:3].tolist() == [3, 0, 1]  # ended rows among them
    st.append(slots, r.rows())
    h, cc, ln = st.state(slots)
    assert np.array_equal(_bits(r.h), _bits(h)) and np.array_equal(r.len, ln)
    assert (cc is None and r.c is None) or np.array_equal(_bits(r.c), _bits(cc))
    assert np.array_equal(_bits(r.h[1]), _bits(before[0][slots[1]]))  # a row that ended at step 0 keeps the state it had
    st.close()


# ---- 6. chunks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", _SMALL, ids=_ids)
def test_three_chunks_of_64(kind, d, monkeypatch):
    c = _case(kind, d)
    monkeypatch.setenv("SBR_ROLLOUT_CHUNK", "64")
    r = c.store.rollout(c.slots, _STEPS, exclude=c.excl, log_prob=True, temperature=_TEMP, final_state=True)
    _same(r, c.expect("greedy"), "chunks of 64")
    monkeypatch.delenv("SBR_ROLLOUT_CHUNK")
    w = c.store.rollout(c.slots, _STEPS, exclude=c.excl, final_state=True)
    assert np.array_equal(_bits(r.h), _bits(w.h)) and np.array_equal(r.len, w.len)


@pytest.mark.parametrize("kind", [NORMAL, EWMA], ids=_ids)
def test_the_real_chunk_of_8192_rows_is_crossed(kind):
    items, d, n, steps, distinct = 300, 16, 8200, 3, 10
    g, o = _pair(kind, d, items=items)
    rs = np.random.RandomState(8)
    base = [rs.randint(0, items, rs.randint(0, 6)) for _ in range(distinct)]
    base[2] = []
    rep, scores = oracle_callables(o, items)
    e = rollout_expect(rep, scores, items, base, steps, base)  # each history excluded, as Model.rollout does
    st = g.sessions(n)
    slots = np.arange(n, dtype=np.uint32)
    hist = [base[i % distinct] for i in range(n)]
    st.append(slots, hist)
    r = st.rollout(slots, steps, exclude=hist)
    tile = np.arange(n) % distinct
    assert np.array_equal(r.items, e.items[tile]) and np.array_equal(_bits(r.scores), _bits(e.scores[tile]))
    assert np.array_equal(r.lengths, e.lengths[tile])
    st.close()
    m = g.rollout(base, steps)  # the convenience is that sequence of calls
    assert np.array_equal(m.items, e.items) and np.array_equal(_bits(m.scores), _bits(e.scores))


# ---- 7. poison -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0xFF, 0x7F, 0x80], ids=lambda p: f"poison{p:02X}")
@pytest.mark.parametrize("remember", [0, 5])
@pytest.mark.parametrize("kind,d", _SMALL, ids=_ids)
def test_on_poisoned_scratch(kind, d, remember, pattern, monkeypatch):
    c = _case(kind, d)
    rows, steps = 24, 5
    e = c.expect("greedy", rows, steps)  # made without the device
    monkeypatch.setenv("SBR_TEST_POISON", str(pattern))
    monkeypatch.setenv("SBR_ROLLOUT_CHUNK", "16")
    if not remember:
        r = c.store.rollout(c.slots[:rows], steps, exclude=c.excl[:rows], log_prob=True, temperature=_TEMP, final_state=True)
    else:  # the same eligibility through the seen-item memory: each row's list is what its slot remembers
        st = c.g.sessions(rows, remember)
        slots = np.arange(rows, dtype=np.uint32)
        st.append(slots, c.hist[:rows])
        seen = st.seen(slots)
        full = [np.concatenate([np.asarray(c.excl[i], dtype=np.int64), seen[i].astype(np.int64)]) for i in range(rows)]
        e = rollout_expect(c.rep, c.scores, _ITEMS, c.hist[:rows], steps, full, partition_temperature=_TEMP)
        r = st.rollout(slots, steps, exclude=c.excl[:rows], log_prob=True, temperature=_TEMP, final_state=True)
        st.close()
    _same(r, e, f"poison {pattern:#x}")
    assert np.all(np.isfinite(r.h))


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------
def _raw(st, slots, steps, flags=0, temperature=1.0, any_of=None):
    L = _lib.load()
    sl = np.ascontiguousarray(slots, dtype=np.uint32)
    ra = _abi.SbrRolloutArgs()
    ra.steps, ra.flags = steps, flags
    ra.sample.temperature = temperature
    out = np.full((max(sl.size, 1), max(min(steps, 2000), 1)), 7, np.uint32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    status = L.sbr_sessions_rollout(st._h, vp(sl), sl.size, C.byref(ra), None, None, vp(any_of), None, vp(out), *([None] * 8))
    assert np.all(out == 7)
    return status


def test_refusals_launch_nothing_and_change_nothing():
    g, _ = _pair(NORMAL, 16, items=300)
    st = g.sessions(8)
    slots = np.arange(6, dtype=np.uint32)
    st.append(slots, [[1, 2], [], [3], [4, 5, 6], [7], [8]])
    before, rec = st.state(slots), st.recommend(slots, 5)
    bad = [lambda: _raw(st, [0, 8], 3), lambda: _raw(st, [0, 2, 0], 3), lambda: _raw(st, slots, 0), lambda: _raw(st, slots, 1025),
           lambda: _raw(st, slots, 3, temperature=float("nan")), lambda: _raw(st, slots, 3, temperature=0.0),
           lambda: _raw(st, slots, 3, temperature=-2.0), lambda: _raw(st, slots, 3, flags=8),
           lambda: _raw(st, slots, 3, flags=_abi.ROLLOUT_INCLUDE_SEEN),  # a store without memory has nothing to include
           lambda: _raw(st, slots, 3, any_of=np.ones(6, np.uint32))]     # masks, and the model has no tags
    for i, call in enumerate(bad):
        assert call() == Status.INVALID_ARGUMENT, i
    with pytest.raises(EngineError) as err:
        st.rollout(slots, 3, any_of=1)
    assert err.value.status == Status.INVALID_ARGUMENT

    def unchanged():
        after, rec2 = st.state(slots), st.recommend(slots, 5)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(before[:2], after[:2])) and np.array_equal(before[2], after[2])
        assert np.array_equal(rec[0], rec2[0]) and np.array_equal(_bits(rec[1]), _bits(rec2[1]))

    unchanged()
    assert np.array_equal(st.rollout(slots, 2).items[:, 0], rec[0][:, 0])  # the call itself works here
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
    bias[77] = np.inf
    g.set_param(Param.ITEM_BIAS, bias)
    st.reset()
    st.append([0, 1], [[1], [2]])
    with pytest.raises(PredictionError.InvalidPredictionValue):
        st.rollout([0, 1], 3)
