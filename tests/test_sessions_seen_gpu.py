"""GPU: the seen-item memory of the session store (sbr_sessions_create_seen, engine.Sessions(remember=W)).

What is held, always on the uint32 view of the scores: a store with memory answers recommend / recommend_diverse and their filtered
forms with, bit for bit, the *_reps call on store.representations(slots) whose exclusion lists are the plain-Python model's
(tests/seen_expect.py) united with the caller's; for histories of at most min(W, max_sequence_length) items that is
model.recommend(histories); store.seen() is the model's list, order and repeats included; reset / set_state / set_seen / a
parameter change follow the header's rules; errors leave states and memory as they were; a store without memory is unchanged.

Shapes are the smallest at which each path exists: 300 items (several 32-item tiles) and 40 slots for the oracles, 3 000 items
where a list has to be longer than 2 000 ids or a memory 1 024 deep, 40 items for the padding, 64 items x 8 200 slots for the second
chunk of a call."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams
from seen_expect import SeenModel
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.errors import EngineError

pytestmark = pytest.mark.gpu

NORMAL, COUPLED, EWMA = ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA
T = 8
NO_ITEM = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_rows(a, b):
    """(items, scores) pairs equal in items and score bits"""
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def random_params(kind, items, d, seed):
    rs = np.random.RandomState(seed)
    ng = {NORMAL: 4, COUPLED: 3, EWMA: 0}[kind]
    out = {Param.ITEM_EMBEDDING: rs.randn(items, d) * 0.3, Param.ITEM_BIAS: rs.randn(items) * 0.5}
    if ng:
        out[Param.LSTM_W] = rs.randn(2 * d, ng * d) * 0.3
        out[Param.LSTM_B] = rs.randn(ng * d) * 0.5
    else:
        out[Param.EWMA_ALPHA] = rs.randn(d)
    return {k: v.astype(np.float32).ravel() for k, v in out.items()}


def new_model(kind, items, d, max_len=T):
    from sbr_rs_amd.engine import Model

    m = Model(hparams(items, max_len, d, int(kind), LOSS_HINGE))
    for which, v in random_params(kind, items, d, 1000 * int(kind) + d).items():
        m.set_param(which, v)
    return m


@functools.lru_cache(maxsize=None)
def model(kind, items, d):
    """one model per (kind, catalogue, width), shared by the tests that only read it"""
    return new_model(kind, items, d)


def csr(seqs):
    ptr = np.zeros(len(seqs) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(s) for s in seqs])
    return ptr, (np.concatenate(seqs) if len(seqs) else np.zeros(0)).astype(np.uint32)


def histories(n, items, max_len, seed):
    """n histories, lengths cycling through 0 .. max_len, drawn from a tenth of the catalogue so that items repeat"""
    rs = np.random.RandomState(seed)
    return [rs.randint(0, max(items // 10, 2), size=i % (max_len + 1)).astype(np.uint32) for i in range(n)]


def append_ragged(st, expect, slots, h, rs):
    done = [0] * len(h)
    while any(done[i] < len(h[i]) for i in range(len(h))):
        pick = rs.permutation(len(h))[: max(1, len(h) - len(h) // 5)]
        take = [min(len(h[i]) - done[i], int(rs.randint(0, 6))) for i in pick]
        parts = [h[i][done[i]: done[i] + n] for i, n in zip(pick, take)]
        st.append([slots[i] for i in pick], parts)
        expect.append([slots[i] for i in pick], parts)
        for i, n in zip(pick, take):
            done[i] += n


def both(st, expect):
    """st and its model driven together"""
    class Both:
        def append(self, slots, items):
            st.append(slots, items)
            expect.append(slots, items)

    return Both()


def assert_seen(st, expect, slots):
    got, want = st.seen(slots), expect.seen(slots)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint32 and g.tolist() == w.tolist(), (i, g.tolist(), w.tolist())


# ---- 1. the two oracles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 48), (COUPLED, 128), (EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_store_with_memory_equals_recommend_of_the_histories(kind, d):
    items, n = 300, 40
    m = model(kind, items, d)
    h = histories(n, items, T, seed=d)
    assert any(len(set(x.tolist())) < len(x) for x in h), "some history repeats an item"
    slots = np.arange(n, dtype=np.uint32) * 2 + 1
    want = {k: m.recommend(*csr(h), k) for k in (1, 10)}
    for way in ("whole", "one per call", "ragged"):
        st, expect = m.sessions(2 * n + 3, remember=T), SeenModel(2 * n + 3, T)
        assert st.seen_capacity == T
        if way == "whole":
            both(st, expect).append(slots, h)
        elif way == "one per call":
            for t in range(T):
                live = [i for i, x in enumerate(h) if len(x) > t]
                both(st, expect).append([slots[i] for i in live], [h[i][t: t + 1] for i in live])
        else:
            append_ragged(st, expect, slots, h, np.random.RandomState(d + 1))
        assert_seen(st, expect, slots)
        reps = st.representations(slots)
        for k in (1, 10):
            got = st.recommend(slots, k)
            assert same_rows(got, want[k]), (way, k, "model.recommend of the histories")
            assert same_rows(got, m.recommend_reps(reps, k, exclude=expect.excluded(slots))), (way, k, "recommend_reps with the model's lists")
            free = st.recommend(slots, k, include_seen=True)
            assert same_rows(free, m.recommend_reps(reps, k)), (way, k, "include_seen ignores the memory")
            if k == 10:  # so that excluding nothing cannot pass: among 10 of 300 items some slot's own items rank
                seen_in_free = [np.intersect1d(free[0][i], expect.seen([s])[0]).size for i, s in enumerate(slots)]
                assert any(seen_in_free) and not np.array_equal(got[0], free[0]), (way, k, "the memory excludes something")
        st.close()


# ---- 2. the ring -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 5, 64, 100, 1024])
@pytest.mark.parametrize("kind", [NORMAL, EWMA], ids=lambda v: v.name)
def test_ring_keeps_the_last_w_in_order_with_repeats(kind, w):
    items = 3000
    m = model(kind, items, 16)
    rs = np.random.RandomState(w)
    st, expect = m.sessions(9, remember=w), SeenModel(9, w)
    assert st.seen_capacity == w
    b = both(st, expect)
    draw = lambda n: rs.randint(0, items, size=n).astype(np.uint32)  # noqa: E731
    # slot 7: 3 w + 1 items in ONE call; slot 1: one item w + 2 times; slot 2: w + 3 items over ragged calls that wrap the ring;
    # slot 3: fewer than w; slot 4: exactly w; slot 5: nothing; slot 0: 2 w + 1 then w - 1 (a full overwrite, then a partial one)
    b.append([7, 1, 3], [draw(3 * w + 1), np.full(w + 1, 17, np.uint32), draw(w // 2)])
    b.append([1, 4, 0], [np.full(1, 17, np.uint32), draw(w), draw(2 * w + 1)])
    left = draw(w + 3)
    while left.size:
        n = min(left.size, int(rs.randint(1, max(2, w // 3 + 2))))
        b.append([2, 5], [left[:n], left[:0]])
        left = left[n:]
    b.append([0], [draw(w - 1)])
    slots = np.array([7, 1, 2, 3, 4, 5, 0, 8], dtype=np.uint32)
    assert_seen(st, expect, slots)
    assert expect.seen([1])[0].tolist() == [17] * min(w, w + 2)
    reps = st.representations(slots)
    for k in (1, 10):
        assert same_rows(st.recommend(slots, k), m.recommend_reps(reps, k, exclude=expect.excluded(slots))), k
    st.close()


# ---- 3. union with the caller's lists -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def union_case():
    """(model with item tags, store, its model, slots, the caller's lists): 3 000 items so that one list can hold more than 2 000
    distinct ids; made once, only read afterwards"""
    items, n, w = 3000, 40, 8
    m = new_model(NORMAL, items, 32)
    rs = np.random.RandomState(5)
    m.set_item_tags(rs.randint(0, 16, size=items).astype(np.uint32))
    h = [rs.randint(0, items, size=i % 12).astype(np.uint32) for i in range(n)]  # some longer than w
    slots = rs.permutation(n + 9)[:n].astype(np.uint32)
    st, expect = m.sessions(n + 9, remember=w), SeenModel(n + 9, w)
    both(st, expect).append(slots, h)
    caller = []
    for i in range(n):
        mine = expect.seen([slots[i]])[0]
        if i % 4 == 0:
            caller.append(np.zeros(0, np.uint32))                                     # empty
        elif i % 4 == 1:
            caller.append(np.concatenate([mine, mine[:2], rs.randint(0, items, size=5).astype(np.uint32)]))  # overlaps, with repeats
        elif i % 4 == 2:
            caller.append(np.setdiff1d(rs.randint(0, items, size=30).astype(np.uint32), mine))               # disjoint
        else:
            caller.append(rs.randint(0, items, size=3).astype(np.uint32))
    caller[7] = rs.permutation(items)[:2400].astype(np.uint32)  # longer than 2 000 ids, unsorted
    assert np.unique(caller[7]).size > 2000
    return m, st, expect, slots, caller


def test_union_recommend():
    m, st, expect, slots, caller = union_case()
    assert_seen(st, expect, slots)
    reps = st.representations(slots)
    for k in (1, 10):
        got = st.recommend(slots, k, exclude=caller)
        assert same_rows(got, m.recommend_reps(reps, k, exclude=expect.excluded(slots, caller))), k
    # the caller's lists alone, the memory ignored
    assert same_rows(st.recommend(slots, 10, exclude=caller, include_seen=True), m.recommend_reps(reps, 10, exclude=caller))


def test_union_recommend_diverse():
    m, st, expect, slots, caller = union_case()
    reps = st.representations(slots)
    for metric in ("cosine", "dot"):
        got = st.recommend_diverse(slots, 4, 16, trade_off=0.4, metric=metric, exclude=caller)
        want = m.recommend_diverse_reps(reps, 4, 16, trade_off=0.4, metric=metric, exclude=expect.excluded(slots, caller))
        assert same_rows(got, want), metric
    assert same_rows(st.recommend_diverse(slots, 4, 16), m.recommend_diverse_reps(reps, 4, 16, exclude=expect.excluded(slots)))


def test_union_filtered_forms():
    m, st, expect, slots, caller = union_case()
    reps = st.representations(slots)
    n = slots.size
    any_of = np.where(np.arange(n) % 3 == 0, 0, 0b0110).astype(np.uint32)
    none_of = np.where(np.arange(n) % 2 == 0, 0b1000, 0).astype(np.uint32)
    united = expect.excluded(slots, caller)
    got = st.recommend(slots, 10, exclude=caller, any_of=any_of, none_of=none_of)
    assert same_rows(got, m.recommend_reps(reps, 10, exclude=united, any_of=any_of, none_of=none_of))
    assert not same_rows(got, st.recommend(slots, 10, exclude=caller)), "the masks do something"
    free = st.recommend(slots, 10, exclude=caller, any_of=any_of, none_of=none_of, include_seen=True)
    assert same_rows(free, m.recommend_reps(reps, 10, exclude=caller, any_of=any_of, none_of=none_of))
    got = st.recommend_diverse(slots, 4, 16, exclude=caller, any_of=any_of, none_of=none_of)
    assert same_rows(got, m.recommend_diverse_reps(reps, 4, 16, exclude=united, any_of=any_of, none_of=none_of))


def test_score_candidates_masks_nothing():
    m, st, expect, slots, caller = union_case()
    cands = [np.concatenate([expect.seen([s])[0], np.array([1, 2], np.uint32)]) for s in slots]
    got = st.score_candidates(slots, cands)
    want = m.score_candidates_reps(st.representations(slots), *csr(cands))
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w)) and np.all(np.isfinite(g))


# ---- 4. padding ------------------------------------------------------------------------------------------------------------------
def test_a_slot_that_has_seen_almost_everything_pads():
    items = 40
    m = model(EWMA, items, 16)
    st = m.sessions(3, remember=64)
    seen38 = np.random.RandomState(1).permutation(items)[:38].astype(np.uint32)
    st.append([1], [seen38])
    it, sc = st.recommend([1, 2], 10)
    left = np.setdiff1d(np.arange(items, dtype=np.uint32), seen38)
    assert sorted(it[0, :2].tolist()) == left.tolist() and np.all(np.isfinite(sc[0, :2]))
    assert it[0, 2:].tolist() == [NO_ITEM] * 8 and np.all(np.isneginf(sc[0, 2:]))
    assert np.all(it[1] != NO_ITEM)  # the empty slot beside it is not padded
    assert same_rows((it, sc), m.recommend_reps(st.representations([1, 2]), 10, exclude=[seen38, []]))
    st.close()


# ---- 5. lifecycle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 32), (EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_reset_set_state_set_seen_and_round_trip(kind, d):
    items, n, w = 300, 12, 5
    m = model(kind, items, d)
    h = histories(n, items, 9, seed=3)  # up to 9 items into a memory of 5
    slots = np.arange(n, dtype=np.uint32)
    st, expect = m.sessions(n, remember=w), SeenModel(n, w)
    both(st, expect).append(slots, h)
    assert_seen(st, expect, slots)
    # the round trip into a second store: state + seen -> set_state + set_seen
    hh, cc, ll = st.state(slots)
    mem = st.seen(slots)
    other = m.sessions(n + 2, remember=w)
    to = slots[::-1] + 2
    other.append(to[:3], [[5, 6, 7, 8, 9, 10]] * 3)  # an earlier occupant, whose memory must not survive set_state
    other.set_state(to, hh, cc, ll)
    assert [a.size for a in other.seen(to)] == [0] * n, "set_state empties the memory"
    other.set_seen(to, mem)
    for a, b_ in zip(other.seen(to), mem):
        assert a.tolist() == b_.tolist()
    assert same_rows(other.recommend(to, 10), st.recommend(slots, 10))
    other.append(to, [[3]] * n)  # and both go on alike
    both(st, expect).append(slots, [[3]] * n)
    assert same_rows(other.recommend(to, 10), st.recommend(slots, 10))
    assert_seen(st, expect, slots)
    other.close()
    # set_seen keeps the last w of a longer list
    st.set_seen([2], [np.arange(20, 31, dtype=np.uint32)])
    expect.set_seen([2], [np.arange(20, 31)])
    assert st.seen([2])[0].tolist() == [26, 27, 28, 29, 30]
    # reset of named slots: theirs and no other
    st.reset([1, 4])
    expect.reset([1, 4])
    assert_seen(st, expect, slots)
    assert st.seen([1, 4])[0].size == 0 and st.seen([1, 4])[1].size == 0
    assert same_rows(st.recommend(slots, 10), m.recommend_reps(st.representations(slots), 10, exclude=expect.excluded(slots)))
    st.reset()
    assert [a.size for a in st.seen(slots)] == [0] * n
    st.close()


def test_errors_leave_states_and_memory_unchanged():
    items, n, w = 300, 6, 4
    m = model(NORMAL, items, 32)
    st = m.sessions(n, remember=w)
    plain = m.sessions(n)
    slots = np.arange(n, dtype=np.uint32)
    h = histories(n, items, 6, seed=8)
    st.append(slots, h)
    plain.append(slots, h)

    def snapshot(s):
        hh, cc, ll = s.state(slots)
        mem = [a.tolist() for a in s.seen(slots)] if s.seen_capacity else None
        return bits(hh).tolist(), bits(cc).tolist(), ll.tolist(), mem

    before, before_plain = snapshot(st), snapshot(plain)
    for call in (lambda: st.append([0, n], [[1], [2]]),                 # a bad slot
                 lambda: st.append([2, 2], [[1], [2]]),                 # a duplicate slot
                 lambda: st.set_seen([0, n], [[1], [2]]),
                 lambda: st.set_seen([3, 3], [[1], [2]]),
                 lambda: st.set_seen([0, 1], [[1, 2], [3, items]]),     # an id >= num_items
                 lambda: st.seen([0, n]),
                 lambda: st.recommend([0, n], 5),
                 lambda: st.recommend([0, 1], 5, exclude=[[items], []])):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT
        assert snapshot(st) == before
    # flags on a store without memory: refused by the library itself, as before
    with pytest.raises(ValueError):
        plain.recommend(slots, 5, include_seen=True)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros((n, 5), np.uint32)
    assert plain._L.sbr_sessions_recommend(plain._h, vp(slots), n, 5, None, None, 1, vp(out), None) == Status.INVALID_ARGUMENT
    masks = np.zeros(n, np.uint32)
    assert plain._L.sbr_sessions_recommend_filtered(plain._h, vp(slots), n, 5, None, None, 1, vp(masks), vp(masks), vp(out), None) == Status.INVALID_ARGUMENT
    assert st._L.sbr_sessions_recommend(st._h, vp(slots), n, 5, None, None, 2, vp(out), None) == Status.INVALID_ARGUMENT  # an unknown flag
    for call in (lambda: plain.seen(slots), lambda: plain.set_seen([0], [[1]])):  # no memory to read or write
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT
    assert plain.seen_capacity == 0
    assert snapshot(plain) == before_plain and snapshot(st) == before
    for bad in (1025, 5000):
        with pytest.raises((EngineError, ValueError)):
            m.sessions(4, remember=bad)
    h_ = C.c_void_p()
    assert st._L.sbr_sessions_create_seen(m._h, 4, 1025, C.byref(h_)) == Status.INVALID_ARGUMENT and not h_.value
    st.close()
    plain.close()


def test_parameter_change_refuses_until_reset_which_empties_the_memory():
    items = 300
    m = new_model(EWMA, items, 20)
    st = m.sessions(4, remember=3)
    st.append([0, 1], [[1, 2], [3]])
    m.set_param(Param.ITEM_BIAS, np.zeros(items, np.float32))
    for call in (lambda: st.seen([0]), lambda: st.set_seen([0], [[1]]), lambda: st.append([0], [[1]]), lambda: st.recommend([0], 3)):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT
    st.reset()
    assert [a.size for a in st.seen([0, 1, 2])] == [0, 0, 0]
    st.append([0], [[7]])
    assert st.seen([0])[0].tolist() == [7]
    it, _ = st.recommend([0], items)
    assert 7 not in it[0].tolist() and it[0, -1] == NO_ITEM
    st.close()
    m.close()


# ---- 6. two chunks ---------------------------------------------------------------------------------------------------------------
def test_second_chunk_reads_its_slots_through_the_calls_index():
    items, n, w = 64, 8200, 4  # recommend_users_cap cuts a call at 8 192 users
    m = model(NORMAL, items, 16)
    rs = np.random.RandomState(11)
    h = [rs.randint(0, items, size=int(x)).astype(np.uint32) for x in rs.randint(0, 7, size=n)]
    slots = rs.permutation(n + 50)[:n].astype(np.uint32)
    st, expect = m.sessions(n + 50, remember=w), SeenModel(n + 50, w)
    both(st, expect).append(slots, h)
    order = rs.permutation(n)
    named = slots[order]
    caller = [np.array([i % items], np.uint32) if i % 3 == 0 else np.zeros(0, np.uint32) for i in range(n)]
    got = st.recommend(named, 3, exclude=caller)
    want = m.recommend_reps(st.representations(named), 3, exclude=expect.excluded(named, caller))
    assert same_rows((got[0][8192:], got[1][8192:]), (want[0][8192:], want[1][8192:])), "the second chunk"
    assert same_rows(got, want)
    assert not np.array_equal(got[0], st.recommend(named, 3, exclude=caller, include_seen=True)[0])
    st.close()


# ---- 7. a store without memory is the store it was ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 48), (EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_store_without_memory_is_unchanged(kind, d):
    items, n = 300, 40
    m = model(kind, items, d)
    h = histories(n, items, T, seed=d)
    slots = np.arange(n, dtype=np.uint32)
    a, b_ = m.sessions(n), m.sessions(n, remember=0)
    for st in (a, b_):
        st.append(slots, h)
        assert st.seen_capacity == 0
    ra, rb = a.representations(slots), b_.representations(slots)
    assert np.array_equal(bits(ra), bits(rb))
    assert same_rows(a.recommend(slots, 10), b_.recommend(slots, 10))
    assert same_rows(a.recommend(slots, 10), m.recommend_reps(ra, 10)), "nothing is excluded without memory"
    assert same_rows(a.recommend(slots, 10, exclude=h), b_.recommend(slots, 10, exclude=h))
    assert same_rows(a.recommend(slots, 10, exclude=h), m.recommend(*csr(h), 10))
    assert same_rows(a.recommend_diverse(slots, 4, 16), b_.recommend_diverse(slots, 4, 16))
    a.close()
    b_.close()
