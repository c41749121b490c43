"""GPU: the session store (sbr_sessions_*, engine.Sessions).  Everything is compared on the uint32 view of the floats: a slot's
representation has the BITS of user_representation of the items appended to it, however they were split across append calls, at
every storage width and for all three model kinds; beyond max_sequence_length it has the bits of a model with a longer window;
recommend / score_candidates read the rows in place and equal the *_reps calls on the representations; errors leave the store
untouched; a parameter change makes the store refuse until reset() re-binds it.

Shapes: 300 items, max_sequence_length 8, every parameter block set to seeded random values (gates and biases non-trivial)."""
import functools

import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams, synthetic_interactions
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.errors import EngineError

pytestmark = pytest.mark.gpu

ITEMS, T = 300, 8
NORMAL, COUPLED, EWMA = ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA
BLOCKS = (Param.ITEM_EMBEDDING, Param.ITEM_BIAS, Param.LSTM_W, Param.LSTM_B, Param.EWMA_ALPHA)
WIDTHS = [(NORMAL, d) for d in (8, 16, 32, 48, 128, 256)] + [(COUPLED, 32), (COUPLED, 128)] + [(EWMA, d) for d in (20, 128, 256)]
ONE_PER_KIND = [(NORMAL, 32), (COUPLED, 32), (EWMA, 20)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def random_params(kind, d, seed):
    """{block: values} for a model of `kind` and embedding_dim d (the blocks it has)."""
    rs = np.random.RandomState(seed)
    ng = {NORMAL: 4, COUPLED: 3, EWMA: 0}[kind]
    out = {Param.ITEM_EMBEDDING: rs.randn(ITEMS, d) * 0.3, Param.ITEM_BIAS: rs.randn(ITEMS) * 0.5}
    if ng:
        out[Param.LSTM_W] = rs.randn(2 * d, ng * d) * 0.3
        out[Param.LSTM_B] = rs.randn(ng * d) * 0.5
    else:
        out[Param.EWMA_ALPHA] = rs.randn(d)
    return {k: v.astype(np.float32).ravel() for k, v in out.items()}


def new_model(kind, d, max_len=T, seed=None):
    from sbr_rs_amd.engine import Model

    m = Model(hparams(ITEMS, max_len, d, int(kind), LOSS_HINGE))
    for which, v in random_params(kind, d, 1000 * int(kind) + d if seed is None else seed).items():
        m.set_param(which, v)
    return m


def histories(n, max_len, seed):
    """n histories, lengths cycling through 0 .. max_len (every length present from n > max_len on), random items"""
    rs = np.random.RandomState(seed)
    return [rs.randint(0, ITEMS, size=i % (max_len + 1)).astype(np.uint32) for i in range(n)]


def csr(seqs):
    ptr = np.zeros(len(seqs) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(s) for s in seqs])
    return ptr, (np.concatenate(seqs) if len(seqs) else np.zeros(0)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def case(kind, d):
    """(model, the 70 histories, user_representations of them): made once per (kind, width), never changed"""
    m = new_model(kind, d)
    h = histories(70, T, seed=d)
    want = m.user_representations(*csr(h))
    want.setflags(write=False)
    return m, h, want


def append_one_per_call(st, slots, h):
    for t in range(max(len(x) for x in h)):
        live = [i for i, x in enumerate(h) if len(x) > t]
        st.append([slots[i] for i in live], [h[i][t: t + 1] for i in live])


def append_ragged(st, slots, h, rs):
    """random splits of 0 .. 5 items per call; slots shuffled, not all of them in every call, some listed with no items"""
    done = [0] * len(h)
    while any(done[i] < len(h[i]) for i in range(len(h))):
        pick = rs.permutation(len(h))[: max(1, len(h) - len(h) // 5)]
        take = [min(len(h[i]) - done[i], int(rs.randint(0, 6))) for i in pick]
        st.append([slots[i] for i in pick], [h[i][done[i]: done[i] + n] for i, n in zip(pick, take)])
        for i, n in zip(pick, take):
            done[i] += n


# ---- 1. split-invariance and parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", WIDTHS, ids=lambda v: getattr(v, "name", str(v)))
def test_three_ways_of_appending_give_user_representations_bits(kind, d):
    m, h, want = case(kind, d)
    n = len(h)
    slots = np.arange(n, dtype=np.uint32) * 2 + 1  # non-contiguous slots of a larger store
    st = m.sessions(2 * n + 5)
    append_one_per_call(st, slots, h)
    assert same(st.representations(slots), want), "one item per call"
    assert st.lengths(slots).tolist() == [len(x) for x in h]
    st.reset(slots)
    assert st.lengths(slots).tolist() == [0] * n
    st.append(slots, h)
    assert same(st.representations(slots), want), "all at once"
    st.reset()
    append_ragged(st, slots, h, np.random.RandomState(d + 1))
    assert same(st.representations(slots), want), "ragged splits"
    assert st.lengths(slots).tolist() == [len(x) for x in h]
    untouched = np.arange(0, 2 * n + 5, 2, dtype=np.uint32)
    assert st.lengths(untouched).tolist() == [0] * untouched.size
    st.close()


@pytest.mark.parametrize("kind,d", ONE_PER_KIND, ids=lambda v: getattr(v, "name", str(v)))
def test_slots_equal_the_oracle(kind, d):
    from oracle.oracle import OracleModel

    m, h, want = case(kind, d)
    orc = OracleModel(hparams(ITEMS, T, d, int(kind), LOSS_HINGE))
    for which, v in random_params(kind, d, 1000 * int(kind) + d).items():
        orc.set_param(which, v)
    st = m.sessions(len(h))
    slots = np.arange(len(h), dtype=np.uint32)
    append_ragged(st, slots, h, np.random.RandomState(3))
    got = st.representations(slots)
    for i, x in enumerate(h):
        assert same(got[i], orc.user_representation(x)), i
    st.close()


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("kind,d", ONE_PER_KIND, ids=lambda v: getattr(v, "name", str(v)))
def test_one_and_thirty_three_sessions(kind, d, n):
    m, h, want = case(kind, d)
    pick = [5] if n == 1 else list(range(33))  # a five-item history; one full tile and one session
    hh = [h[i] for i in pick]
    slots = np.arange(n, dtype=np.uint32)[::-1].copy()
    st = m.sessions(n)
    append_one_per_call(st, slots, hh)
    assert same(st.representations(slots), want[pick])
    st.reset(slots)
    st.append(slots, hh)
    assert same(st.representations(slots), want[pick])
    st.reset()
    append_ragged(st, slots, hh, np.random.RandomState(n))
    assert same(st.representations(slots), want[pick])
    st.close()


# ---- 2. beyond the window ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", ONE_PER_KIND, ids=lambda v: getattr(v, "name", str(v)))
def test_beyond_the_window_a_session_keeps_the_whole_recurrence(kind, d):
    m, _, _ = case(kind, d)
    twin = new_model(kind, d, max_len=32, seed=77)  # other values first: the copy below is what makes it a twin
    for which in BLOCKS:
        if m.param_count(which):
            twin.set_param(which, m.get_param(which))
    h = histories(42, 20, seed=9)  # lengths 0 .. 20, twice
    st = m.sessions(len(h))
    slots = np.arange(len(h), dtype=np.uint32)
    append_ragged(st, slots, h, np.random.RandomState(4))
    got = st.representations(slots)
    assert same(got, twin.user_representations(*csr(h)))
    windowed = m.user_representations(*csr(h))
    for i, x in enumerate(h):  # the test can see the difference: the T = 8 model truncates
        assert same(got[i], windowed[i]) == (len(x) <= T), (i, len(x))
    st.close()
    twin.close()


# ---- 3. empty slots ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", ONE_PER_KIND, ids=lambda v: getattr(v, "name", str(v)))
def test_empty_slots(kind, d):
    m, _, _ = case(kind, d)
    st = m.sessions(4)
    empty = m.user_representation([])
    assert same(st.representations([0, 3]), np.stack([empty, empty]))
    assert st.lengths([0, 1, 2, 3]).tolist() == [0, 0, 0, 0]
    h0, c0, n0 = st.state([2])
    assert not h0.any() and (c0 is None or not c0.any()) and n0.tolist() == [0]  # the item-0 step of an empty slot is not stored
    st.append([2], [[17]])
    got = st.representations([2])[0]
    assert same(got, m.user_representation([17]))
    assert not same(got, m.user_representation([0, 17]))  # not the history with item 0 prepended
    # appending item 0 to an empty slot is a real step that happens to give the empty history's representation
    st.append([1], [[0]])
    assert same(st.representations([1])[0], empty) and st.lengths([1]).tolist() == [1]
    st.append([1], [[17]])
    assert same(st.representations([1])[0], m.user_representation([0, 17]))
    st.close()


# ---- 4. isolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", ONE_PER_KIND, ids=lambda v: getattr(v, "name", str(v)))
def test_unnamed_slots_keep_their_bits_and_reset_reproduces(kind, d):
    m, h, want = case(kind, d)
    n = len(h)
    slots = np.arange(n, dtype=np.uint32)
    st = m.sessions(n)
    st.append(slots, [x[:3] for x in h])
    odd, even = slots[1::2], slots[0::2]
    before = st.state(odd)
    st.append(even, [h[i][3:] for i in even])
    after = st.state(odd)
    assert same(before[0], after[0]) and (kind == EWMA or same(before[1], after[1])) and np.array_equal(before[2], after[2])
    st.append(odd, [h[i][3:] for i in odd])
    first = st.state(slots)
    assert same(st.representations(slots), want)
    st.reset(slots)
    st.append(slots, [x[:3] for x in h])
    st.append(even, [h[i][3:] for i in even])
    st.append(odd, [h[i][3:] for i in odd])
    again = st.state(slots)
    assert same(first[0], again[0]) and (kind == EWMA or same(first[1], again[1])) and np.array_equal(first[2], again[2])
    st.close()


# ---- 5. checkpoint round trip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 48), (COUPLED, 32), (EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_checkpoint_round_trip(kind, d):
    m, h, want = case(kind, d)
    n = len(h)
    slots = np.arange(n, dtype=np.uint32)
    a = m.sessions(n)
    a.append(slots, [x[:4] for x in h])
    hs, cs, ns = a.state(slots)
    b = m.sessions(n + 9)
    there = (slots + 9)[::-1].copy()
    b.set_state(there, hs[::-1], None if cs is None else cs[::-1], ns[::-1])
    a.append(slots, [x[4:] for x in h])
    b.append(there, [h[i][4:] for i in slots[::-1]])
    sa, sb = a.state(slots), b.state(there[::-1].copy())
    assert same(sa[0], sb[0]) and (kind == EWMA or same(sa[1], sb[1])) and np.array_equal(sa[2], sb[2])
    assert same(b.representations(there[::-1].copy()), want)
    a.close()
    b.close()


# ---- 6. scans in place -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("kind,d", [(NORMAL, 48), (COUPLED, 128), (EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_scans_read_the_store_in_place(kind, d, k):
    m, h, want = case(kind, d)
    n = len(h)  # 70 slots; histories 0, 9, 18, ... are empty: empty slots among them
    rs = np.random.RandomState(k)
    order = rs.permutation(n).astype(np.uint32)  # not ascending
    slots = order + 2
    st = m.sessions(n + 2)
    st.append(slots, [h[i] for i in order])
    reps = st.representations(slots)
    assert same(reps, want[order])
    excl = [rs.randint(0, ITEMS, size=int(rs.randint(0, 6))).astype(np.uint32) for _ in range(n)]
    gi, gs = st.recommend(slots, k, exclude=excl)
    wi, ws = m.recommend_reps(reps, k, exclude=excl)
    assert np.array_equal(gi, wi) and same(gs, ws)
    gi, gs = st.recommend(slots, k)
    wi, ws = m.recommend_reps(reps, k)
    assert np.array_equal(gi, wi) and same(gs, ws)
    # with each history as the exclusion list: recommend of the histories
    gi, gs = st.recommend(slots, k, exclude=[h[i] for i in order])
    wi, ws = m.recommend(*csr([h[i] for i in order]), k)
    assert np.array_equal(gi, wi) and same(gs, ws)
    cands = [rs.randint(0, ITEMS, size=int(rs.randint(0, 7))).astype(np.uint32) for _ in range(n)]
    got = st.score_candidates(slots, cands)
    exp = m.score_candidates_reps(reps, *csr(cands))
    hist = m.score_candidates(*csr([h[i] for i in order]), *csr(cands))
    for g, e, f in zip(got, exp, hist):
        assert same(g, e) and same(g, f)
    st.close()


# ---- 7. errors leave the store untouched -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 32), (EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_errors_leave_the_store_untouched(kind, d):
    m, h, _ = case(kind, d)
    cap = 12
    st = m.sessions(cap)
    slots = np.arange(cap, dtype=np.uint32)
    st.append(slots, h[:cap])
    before = st.state(slots)
    two = [np.array([1, 2], np.uint32), np.array([3], np.uint32)]
    bad = [
        lambda: st.append([3, 3], two),  # the same slot twice
        lambda: st.append([3, cap], two),  # a slot == capacity
        lambda: st.append([3, 4], [np.array([1, ITEMS], np.uint32), np.array([3], np.uint32)]),  # an item id == num_items
        lambda: st.append([3, 4], (np.array([0, 2, 1], np.uint64), np.array([1, 2, 3], np.uint32))),  # decreasing pointers
        lambda: st.recommend([3, 3], 5),
        lambda: st.recommend([3, cap], 5),
        lambda: st.recommend([3, 4], 0),
        lambda: st.recommend([3, 4], 1025),
        lambda: st.recommend([3, 4], 5, exclude=[[ITEMS], []]),
        lambda: st.score_candidates([3, cap], two),
        lambda: st.score_candidates([3, 4], [np.array([ITEMS], np.uint32), np.array([3], np.uint32)]),
        lambda: st.representations([cap]),
        lambda: st.reset([2, 2]),
        lambda: st.set_state([1, 1], before[0][:2], None if before[1] is None else before[1][:2], before[2][:2]),
        lambda: st.state([cap]),
        lambda: st.lengths([0, cap]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT, i
        after = st.state(slots)
        assert same(before[0], after[0]) and (kind == EWMA or same(before[1], after[1])) and np.array_equal(before[2], after[2]), i
    st.close()


# ---- 8. staleness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", ["fit", "set_param"])
@pytest.mark.parametrize("kind,d", [(NORMAL, 32), (EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_a_parameter_change_makes_the_store_stale_until_reset(kind, d, change):
    m = new_model(kind, d)  # its own model: the parameters change here
    h = histories(20, T, seed=5)
    slots = np.arange(len(h), dtype=np.uint32)
    st = m.sessions(len(h))
    st.append(slots, h)
    hs, cs, ns = st.state(slots)
    if change == "fit":
        m.fit(*synthetic_interactions(24, ITEMS, 12, seed=3))
    else:
        m.set_param(Param.ITEM_BIAS, m.get_param(Param.ITEM_BIAS))  # even the same values: the generation is what counts
    calls = [lambda: st.append(slots, h), lambda: st.representations(slots), lambda: st.recommend(slots, 5),
             lambda: st.score_candidates(slots, h), lambda: st.state(slots), lambda: st.set_state(slots, hs, cs, ns),
             lambda: st.lengths(slots), lambda: st.reset(slots)]
    for i, call in enumerate(calls):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT, i
    assert st.capacity == len(h)
    st.reset()  # reset_all re-binds
    assert st.lengths(slots).tolist() == [0] * len(h)
    st.append(slots, h)
    assert same(st.representations(slots), m.user_representations(*csr(h)))
    st.close()
    m.close()


def test_no_store_call_while_a_fit_plan_is_open_and_model_close_closes_stores():
    m = new_model(NORMAL, 32)
    h = histories(10, T, seed=6)
    slots = np.arange(len(h), dtype=np.uint32)
    st = m.sessions(len(h))
    st.append(slots, h)
    plan = m.fit_begin(*synthetic_interactions(24, ITEMS, 12, seed=3))
    for i, call in enumerate([lambda: st.representations(slots), lambda: st.append(slots, h), lambda: st.reset()]):
        with pytest.raises(EngineError) as e:  # the plan's steps rewrite parameters: not even reset_all binds to them
            call()
        assert e.value.status == Status.INVALID_ARGUMENT, i
    plan.close()
    with pytest.raises(EngineError):
        st.representations(slots)  # stale: the plan may have stepped
    st.reset()
    st.append(slots, h)
    assert same(st.representations(slots), m.user_representations(*csr(h)))
    m.close()  # closes its live stores first; closing the store again touches nothing
    assert st._h is None
    st.close()
