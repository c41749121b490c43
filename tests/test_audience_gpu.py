"""GPU: the audience scan — for each query item the k sessions (or caller-supplied rows) that score it highest
(sbr_sessions_audience / sbr_audience_reps / sbr_audience; engine.Sessions.audience, engine.Model.audience_reps / audience).

What is held, always on the uint32 view of the scores: the rows are tests/audience_expect.py's — score descending, ties to the
lower slot id, padded with (0xFFFFFFFF, -inf) — over scores taken from store.score_candidates for the same (slot, item) pairs,
which is already held to predict and runs on the vector ALU, not in the scan.  So the scan's MFMA chain with the operands' roles
exchanged, and the query bias added in its epilogue, must reproduce predict's bits.

Shapes, the smallest at which each path exists: 300 items; a store of 200 slots with 170 live ones (6 scanned 32-row tiles, the last
partial); 150 queries, unsorted, with repeats (two 128-query tiles, the second partial); several slots with identical item
sequences, hence identical scores; a memory of 8 items against sessions of up to 12."""
import ctypes as C
import functools

import numpy as np
import pytest

import audience_expect as ae
from helpers import LOSS_HINGE, hparams
from seen_expect import SeenModel
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.errors import EngineError, PredictionError

pytestmark = pytest.mark.gpu

NORMAL, COUPLED, EWMA = ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA
T, ITEMS, CAPACITY, LIVE, Q, W = 8, 300, 200, 170, 150, 8
CASES = [(NORMAL, 16), (NORMAL, 128), (EWMA, 16), (EWMA, 128), (EWMA, 256), (COUPLED, 20)]
ids_of = lambda v: getattr(v, "name", str(v))  # noqa: E731


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_rows(got, want, what):
    rows, sc = got
    assert rows.dtype == np.uint32 and sc.dtype == np.float32
    assert np.array_equal(rows, want[0]), (what, "ids", np.argwhere(rows != want[0])[:5].tolist())
    assert np.array_equal(bits(sc), want[1]), (what, "score bits", np.argwhere(bits(sc) != want[1])[:5].tolist())


def new_model(kind, d):
    from sbr_rs_amd.engine import Model

    rs = np.random.RandomState(1000 * int(kind) + d)
    ng = {NORMAL: 4, COUPLED: 3, EWMA: 0}[kind]
    m = Model(hparams(ITEMS, T, d, int(kind), LOSS_HINGE))
    params = {Param.ITEM_EMBEDDING: rs.randn(ITEMS, d) * 0.3, Param.ITEM_BIAS: rs.randn(ITEMS) * 0.5}
    if ng:
        params[Param.LSTM_W] = rs.randn(2 * d, ng * d) * 0.3
        params[Param.LSTM_B] = rs.randn(ng * d) * 0.5
    else:
        params[Param.EWMA_ALPHA] = rs.randn(d)
    for which, v in params.items():
        m.set_param(which, v.astype(np.float32).ravel())
    return m


def session_items(seed):
    """LIVE distinct slots of CAPACITY in no order and their item sequences: 1..12 items drawn from 40 ids (so items repeat inside
    a session and across sessions, and a memory of 8 has wrapped for the long ones); slots 3 k, k < 6, of the list share one
    sequence, and so do three others: identical states, identical scores."""
    rs = np.random.RandomState(seed)
    slots = rs.permutation(CAPACITY)[:LIVE].astype(np.uint32)
    seqs = [rs.randint(0, 40, size=1 + i % 12).astype(np.uint32) for i in range(LIVE)]
    for i in range(0, 18, 3):
        seqs[i] = seqs[0]
    for i in (40, 77, 131):
        seqs[i] = seqs[40]
    return slots, seqs


QUERIES = np.random.RandomState(5).randint(0, ITEMS, size=Q).astype(np.uint32)
QUERIES[:40] = np.random.RandomState(6).randint(0, 40, size=40)  # items the sessions hold
QUERIES[100:110] = QUERIES[0:10]  # repeats


class Setup:
    """one model, a plain store and a store with memory holding the same sessions, and the reference scores of every
    (query, live slot) pair — computed once, read by every test of the case"""

    def __init__(self, kind, d):
        self.m = new_model(kind, d)
        self.slots, self.seqs = session_items(d)
        self.plain = self.m.sessions(CAPACITY)
        self.mem = self.m.sessions(CAPACITY, remember=W)
        self.model = SeenModel(CAPACITY, W)
        for st in (self.plain, self.mem, self.model):
            half = LIVE // 2  # two calls, the second one splitting nothing: states do not depend on how items arrive
            st.append(self.slots[:half], self.seqs[:half])
            st.append(self.slots[half:], self.seqs[half:])
        self.order = np.argsort(self.slots)
        self.sorted_slots = self.slots[self.order]
        self.score_bits = self.scores(self.plain, self.sorted_slots, QUERIES)

    @staticmethod
    def scores(store, slots, items):
        """[len(items), len(slots)] uint32: score_candidates' bits of every pair"""
        per_slot = store.score_candidates(slots, [items] * len(slots))
        return np.stack([bits(x) for x in per_slot], axis=1)


@functools.lru_cache(maxsize=None)
def setup(kind, d):
    return Setup(kind, d)


# ---- 1. bits, order, padding, item ranges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", CASES, ids=ids_of)
def test_rows_have_score_candidates_bits_in_the_total_order(kind, d, monkeypatch):
    s = setup(kind, d)
    for k in (1, 10, LIVE + 7):
        want = ae.expected_rows(s.score_bits, s.sorted_slots, k)
        if k > LIVE:
            assert np.all(want[0][:, LIVE:] == ae.NO_ROW) and np.all(want[0][:, :LIVE] != ae.NO_ROW)
        for groups in (None, "1", "3"):  # the test hook is read per call: one long range of candidates, or three
            if groups is None:
                monkeypatch.delenv("SBR_CATALOGUE_GROUPS", raising=False)
            else:
                monkeypatch.setenv("SBR_CATALOGUE_GROUPS", groups)
            got = s.plain.audience(QUERIES, k, slots=s.slots)
            assert_rows(got, want, (k, groups))
        monkeypatch.delenv("SBR_CATALOGUE_GROUPS", raising=False)
    # repeated queries get equal rows
    got = s.plain.audience(QUERIES, 10, slots=s.slots)
    assert np.array_equal(got[0][100:110], got[0][0:10]) and np.array_equal(bits(got[1][100:110]), bits(got[1][0:10]))


@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 128)], ids=ids_of)
def test_ties_go_to_the_lower_slot_at_and_across_the_kth_position(kind, d):
    s = setup(kind, d)
    tied = sorted(int(x) for x in s.slots[[40, 77, 131]])
    cols = [int(np.searchsorted(s.sorted_slots, t)) for t in tied]
    assert len({int(v) for v in s.score_bits[0, cols]}) == 1, "identical sessions score identically"
    full = ae.expected_rows(s.score_bits, s.sorted_slots, LIVE)[0]
    for j in (0, 57):
        at = [int(np.flatnonzero(full[j] == t)[0]) for t in tied]
        assert at == [at[0], at[0] + 1, at[0] + 2], "neighbours in the order, lower slot first"
        for k in (at[0] + 1, at[0] + 2, at[0] + 3):  # the k-th position cuts the group after 1, 2 and 3 of its members
            got = s.plain.audience(QUERIES[j: j + 1], k, slots=s.slots)
            assert_rows(got, ae.expected_rows(s.score_bits[j: j + 1], s.sorted_slots, k), (j, k))
            assert got[0][0, at[0]: k].tolist() == tied[: k - at[0]]


# ---- 2. candidates ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 128), (EWMA, 16)], ids=ids_of)
def test_candidate_lists(kind, d):
    s = setup(kind, d)
    # slots=None: the live slots, ascending
    assert_rows(s.plain.audience(QUERIES, 10), ae.expected_rows(s.score_bits, s.sorted_slots, 10), "slots=None")
    # a shuffled subset with an empty slot in it: results are slot ids, the empty slot scores as the empty-history row
    empty = int(np.setdiff1d(np.arange(CAPACITY), s.slots)[3])
    rs = np.random.RandomState(d)
    subset = np.concatenate([rs.choice(s.slots, size=45, replace=False), [empty]]).astype(np.uint32)
    rs.shuffle(subset)
    sub_sorted = np.sort(subset)
    sub_bits = Setup.scores(s.plain, sub_sorted, QUERIES)
    got = s.plain.audience(QUERIES, 46, slots=subset)
    assert_rows(got, ae.expected_rows(sub_bits, sub_sorted, 46), "subset")
    assert np.all(np.sort(got[0], axis=1) == sub_sorted), "every candidate, as a slot id, in every full row"
    reps0 = s.m.user_representations(np.array([0, 0], np.uint64), np.zeros(0, np.uint32))
    col = int(np.searchsorted(sub_sorted, empty))
    assert np.array_equal(sub_bits[:, col], bits(s.m.predict(reps0[0], QUERIES))), "the empty slot is the empty history"
    # caller exclusions: slot ids per query; one that is no candidate is ignored
    exclude = [rs.choice(np.arange(CAPACITY), size=j % 5, replace=False).astype(np.uint32) for j in range(Q)]
    assert_rows(s.plain.audience(QUERIES, 12, slots=subset, exclude=exclude), ae.expected_rows(sub_bits, sub_sorted, 12, exclude), "exclude")
    # no candidates at all: rows of padding; no queries: a no-op
    rows, sc = s.plain.audience(QUERIES[:3], 4, slots=[])
    assert np.all(rows == ae.NO_ROW) and np.all(np.isneginf(sc))
    rows, sc = s.plain.audience([], 4)
    assert rows.shape == (0, 4) and sc.shape == (0, 4)


# ---- 3. seen-item memory --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 128), (COUPLED, 20)], ids=ids_of)
def test_seen_memory_excludes_on_the_device(kind, d, monkeypatch):
    s = setup(kind, d)
    assert any(len(x) > W for x in s.seqs) and any(len(set(x.tolist())) < len(x) for x in s.seqs)
    seen = ae.seen_excluded(s.model, s.sorted_slots, QUERIES)
    assert any(seen) and any(len(x) > 3 for x in seen)
    # a wrapped ring excludes by its last W items only
    long_i = next(i for i, x in enumerate(s.seqs) if len(x) > W and x[0] not in x[-W:].tolist())
    j_forgot = np.array([s.seqs[long_i][0]], dtype=np.uint32)
    assert int(s.slots[long_i]) not in ae.seen_excluded(s.model, s.sorted_slots, j_forgot)[0]
    for k in (1, 10, LIVE + 7):
        for groups in ("1", "3"):
            monkeypatch.setenv("SBR_CATALOGUE_GROUPS", groups)
            assert_rows(s.mem.audience(QUERIES, k), ae.expected_rows(s.score_bits, s.sorted_slots, k, seen), ("seen", k, groups))
        monkeypatch.delenv("SBR_CATALOGUE_GROUPS", raising=False)
    assert_rows(s.mem.audience(j_forgot, LIVE), ae.expected_rows(Setup.scores(s.plain, s.sorted_slots, j_forgot), s.sorted_slots, LIVE,
                                                                 ae.seen_excluded(s.model, s.sorted_slots, j_forgot)), "forgotten item")
    # include_seen ignores the memory: the plain store's rows
    free = s.mem.audience(QUERIES, 10, include_seen=True)
    assert_rows(free, ae.expected_rows(s.score_bits, s.sorted_slots, 10), "include_seen")
    assert_rows(free, (s.plain.audience(QUERIES, 10)[0], bits(s.plain.audience(QUERIES, 10)[1])), "the plain store")
    assert not np.array_equal(free[0], s.mem.audience(QUERIES, 10)[0]), "the memory excludes something"
    # the caller's lists unite with the memory; explicit candidates in no order
    rs = np.random.RandomState(d + 3)
    exclude = [rs.choice(s.slots, size=j % 4, replace=False) for j in range(Q)]
    both = ae.unite(seen, exclude)
    assert_rows(s.mem.audience(QUERIES, 10, slots=s.slots, exclude=exclude), ae.expected_rows(s.score_bits, s.sorted_slots, 10, both), "union")


@pytest.mark.parametrize("kind,d", [(EWMA, 16), (NORMAL, 128)], ids=ids_of)
def test_item_seen_by_everyone_and_reset(kind, d):
    m = setup(kind, d).m
    slots, seqs = session_items(d + 1)
    slots, seqs = slots[:70], seqs[:70]  # three tiles, the last partial
    st, model = m.sessions(CAPACITY, remember=W), SeenModel(CAPACITY, W)
    everyone = np.uint32(299)
    for x in (st, model):
        x.append(slots, seqs)
        x.append(slots, [[everyone, everyone]] * len(slots))  # twice: a repeat in a ring counts once
    sorted_slots = np.sort(slots)
    queries = np.array([299, 3, 299, 17, 250], dtype=np.uint32)
    score_bits = Setup.scores(st, sorted_slots, queries)
    got = st.audience(queries, 5)
    assert np.all(got[0][[0, 2]] == ae.NO_ROW) and np.all(np.isneginf(got[1][[0, 2]])), "everybody has it: a row of padding"
    assert_rows(got, ae.expected_rows(score_bits, sorted_slots, 5, ae.seen_excluded(model, sorted_slots, queries)), "before reset")
    # reset slots are empty: their memory is gone, and as named candidates they are eligible again (the empty-history row)
    back = slots[:9]
    st.reset(back)
    model.reset(back)
    score_bits = Setup.scores(st, sorted_slots, queries)
    got = st.audience(queries, 70, slots=slots)
    assert_rows(got, ae.expected_rows(score_bits, sorted_slots, 70, ae.seen_excluded(model, sorted_slots, queries)), "after reset")
    assert sorted(int(x) for x in got[0][0] if x != ae.NO_ROW) == sorted(int(x) for x in back)
    assert not np.isin(back, st.audience(queries, 70)[0]).any(), "slots=None: an empty slot is no candidate"
    st.close()


def test_second_chunk_of_queries():
    """8 200 queries are two launches (8 192 per chunk): the second one's rows, its share of the caller's lists and — on the store
    with memory — its own inverted lists start past zero"""
    s = setup(EWMA, 16)
    rs = np.random.RandomState(11)
    queries = rs.randint(0, 60, size=8200).astype(np.uint32)  # mostly items the sessions hold
    exclude = [s.slots[[j % LIVE, (7 * j) % LIVE]] for j in range(queries.size)]
    score_bits = Setup.scores(s.plain, s.sorted_slots, queries)
    want = ae.expected_rows(score_bits, s.sorted_slots, 5, exclude)
    assert_rows(s.plain.audience(queries, 5, exclude=exclude), want, "host lists")
    seen = ae.seen_excluded(s.model, s.sorted_slots, queries)
    assert any(seen[8192:])
    assert_rows(s.mem.audience(queries, 5, exclude=exclude), ae.expected_rows(score_bits, s.sorted_slots, 5, ae.unite(seen, exclude)), "device lists")
    assert_rows(s.mem.audience(queries, 5), ae.expected_rows(score_bits, s.sorted_slots, 5, seen), "device lists alone")


# ---- 4. the other two entry points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 256)], ids=ids_of)
def test_audience_reps_and_model_audience(kind, d):
    s = setup(kind, d)
    reps = s.plain.representations(s.sorted_slots)
    store_rows, store_scores = s.plain.audience(QUERIES, 10)
    rows, sc = s.m.audience_reps(reps, QUERIES, 10)
    pos = np.where(store_rows == ae.NO_ROW, ae.NO_ROW, np.searchsorted(s.sorted_slots, store_rows)).astype(np.uint32)
    assert_rows((rows, sc), (pos, bits(store_scores)), "positions in place of slot ids")
    # histories of at most max_sequence_length items: model.audience is audience_reps with the holders' lists
    hist = [x[:T] for x in s.seqs]
    ptr = np.zeros(len(hist) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(x) for x in hist])
    flat = np.concatenate(hist).astype(np.uint32)
    ureps = s.m.user_representations(ptr, flat)
    holders = [[u for u, x in enumerate(hist) if int(q) in x.tolist()] for q in QUERIES]
    assert any(holders)
    want = s.m.audience_reps(ureps, QUERIES, 10, exclude=holders)
    assert_rows(s.m.audience(ptr, flat, QUERIES, 10), (want[0], bits(want[1])), "exclude_history")
    assert not np.array_equal(want[0], s.m.audience_reps(ureps, QUERIES, 10)[0])
    free = s.m.audience_reps(ureps, QUERIES, 10)
    assert_rows(s.m.audience(ptr, flat, QUERIES, 10, include_history=True), (free[0], bits(free[1])), "include_history")
    # the reference of the whole: predict's bits for a few pairs
    for j in (0, 149):
        for c in range(3):
            u = int(free[0][j, c])
            assert bits(s.m.predict(ureps[u], QUERIES[j: j + 1]))[0] == bits(free[1])[j, c]


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_non_finite_state_fails_the_call_only_among_the_candidates():
    kind, d = EWMA, 16
    m = setup(kind, d).m
    st = m.sessions(64, remember=W)
    slots = np.arange(40, dtype=np.uint32)
    st.append(slots, [[i % 30, (i * 7) % 30] for i in range(40)])
    h, c, n = st.state([5])
    h[0, 3] = np.nan
    st.set_state([5], h, c, n)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        st.audience([1, 2, 3], 5)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        st.audience([1, 2, 3], 5, slots=[4, 5, 6])
    others = np.delete(slots, 5)
    rows, sc = st.audience([1, 2, 3], 5, slots=others)
    assert np.all(np.isfinite(sc)) and not np.isin(5, rows)
    st.close()


def test_argument_errors_and_a_stale_store():
    kind, d = NORMAL, 16
    m = new_model(kind, d)  # its own model: the parameters change below
    st = m.sessions(32)
    st.append([1, 2, 3], [[4], [5, 6], [7]])
    with pytest.raises(EngineError) as e:
        st.audience([1, ITEMS], 3)
    assert e.value.status == Status.INVALID_ARGUMENT
    with pytest.raises(EngineError):
        st.audience([1], 3, slots=[1, 32])
    with pytest.raises(EngineError):
        st.audience([1], 3, exclude=[[32]])
    with pytest.raises(EngineError):
        m.audience_reps(np.zeros((4, d), np.float32), [1], 0)
    with pytest.raises(EngineError):
        m.audience_reps(np.zeros((4, d), np.float32), [1], 2, exclude=[[4]])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    q, dup, out = np.array([1], np.uint32), np.array([2, 3, 2], np.uint32), np.zeros(3, np.uint32)
    assert st._L.sbr_sessions_audience(st._h, vp(q), 1, 3, vp(dup), 3, None, None, 0, vp(out), None) == Status.INVALID_ARGUMENT
    assert st._L.sbr_sessions_audience(st._h, vp(q), 1, 3, None, 0, None, None, 1, vp(out), None) == Status.INVALID_ARGUMENT  # no memory, a flag
    before = st.audience([1, 9], 3)
    assert set(before[0][0].tolist()) == {1, 2, 3} and set(before[0][1].tolist()) == {1, 2, 3}
    m.set_param(Param.ITEM_BIAS, np.zeros(ITEMS, np.float32))
    with pytest.raises(EngineError) as e:
        st.audience([1, 9], 3)
    assert e.value.status == Status.INVALID_ARGUMENT
    st.reset()
    rows, sc = st.audience([1, 9], 3)
    assert np.all(rows == ae.NO_ROW), "re-bound and empty: no live slot"
    st.append([1, 2, 3], [[4], [5, 6], [7]])
    assert set(st.audience([1, 9], 3)[0][0].tolist()) == {1, 2, 3}
    st.close()
    m.close()
