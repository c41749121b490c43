"""GPU: rank_targets under a serving policy — tag masks, an item set, a session store's seen items (ELIGIBLE RANKS,
include/sbr_hip.h) — against the CPU oracle's scores and tests/rank_eligible_expect.py, integer for integer.

Shapes are the serving matrix's, the smallest at which these kernels can go wrong: 229 items, 130 rows (the second row tile holds
two), SBR_CATALOGUE_GROUPS 1 and 3 (ranges of 96 / 96 / 37: a ragged last tile, a short range), the planted identical pairs across
a tile edge (31, 32) and a range edge (95, 96); stored widths 16 .. 256 and one padded dim each (tests/rank_eligible_cases.py).
A row's targets: 0, 1, 8, 9, 16, 17, 19 or 35 of them — TM and TM + 1 and 2 TM + 3 at both TM = 16 and TM = 8, so a row is cut into
scan rows at both — and, where the row has room, a duplicate, the row's best and worst eligible item, the four items of the tie
classes, a forbidden item, an item outside the set, a listed item that is also forbidden (it must leave the count once, not twice)
and a listed item the masks allow.  Masks cycle through the serving matrix's seven kinds (zero / zero, any_of, none_of, both, a pair
that allows nothing, ...), so rows 127 and 128 — neighbours in one row tile — differ."""
import numpy as np
import pytest

import rank_eligible_cases as rc
import serving_matrix as sm
from helpers import LOSS_HINGE, hparams
from rank_eligible_expect import expect_rows, mask_list
from sbr_rs_amd._abi import ModelKind, Param
from sbr_rs_amd.engine import Model, guard_report
from sbr_rs_amd.errors import EngineError, PredictionError
from sequence_expect import csr
from test_serving_matrix_gpu import KIND, Case, _rep_rows, _store_with_memory

pytestmark = pytest.mark.gpu

ITEMS, ROWS = sm.ITEMS, sm.ROWS
COUNTS = (0, 1, 8, 9, 16, 17, 19, 35)
TIE_ITEMS = (31, 32, 95, 96)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(case):
        key = (case.kind, case.dim)
        if key not in made:
            made[key] = Policy(Case(KIND[case.kind], case.dim))
        return made[key]

    yield get
    for p in made.values():
        p.close()


@pytest.fixture(params=[1, 3], ids=lambda g: f"groups{g}")
def groups(request, monkeypatch):
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", str(request.param))
    return request.param


@pytest.fixture
def guard(request, monkeypatch):
    """SBR_TEST_GUARD=256 around one test, as tests/test_guarded_scratch_gpu.py sets it (that module's own fixture proves the hook is
    live: a byte outside a buffer is seen and placed); what the process checked before is drained first"""
    monkeypatch.setenv("SBR_TEST_GUARD", "256")
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", "3")
    guard_report()
    yield 256
    r = guard_report()
    print(f"guard report: {request.node.name}: {r}")
    assert r.violations == 0, f"a store outside its buffer: {r}"
    assert r.checked > 0 and r.bytes > 0, f"nothing was checked: {r}"


def _targets(scores, lists, tags, any_of, none_of, members, seed):
    """one target array per row (see the module's docstring); the specials are taken under the row's FULL policy (list, masks and
    set), so every body that uses a part of the policy still meets forbidden, outside and listed targets"""
    rs = np.random.RandomState(seed)
    out = []
    for u in range(ROWS):
        n = COUNTS[u % len(COUNTS)]
        t = rs.randint(0, ITEMS, n).astype(np.uint32)
        if n >= 16:
            listed = {int(i) for i in np.asarray(lists[u]).tolist()}
            forbidden = mask_list(ITEMS, (), tags, any_of[u], none_of[u])
            outside = mask_list(ITEMS, (), None, 0, 0, members)
            m = listed | forbidden | outside
            ok = [i for i in range(ITEMS) if i not in m]
            special = [int(t[0]), int(t[0]), *TIE_ITEMS]
            if ok:
                special += [max(ok, key=lambda i: (scores[u][i], -i)), min(ok, key=lambda i: (scores[u][i], i))]
            for pool in (forbidden, outside, listed & forbidden, listed - forbidden - outside):
                if pool:
                    special.append(sorted(pool)[u % len(pool)])
            t[: len(special)] = special[: t.size]
        out.append(t)
    return out


class Policy:
    """A serving-matrix case with what the bodies below share: targets, their CSR, and a store with memory — made once, read only."""

    def __init__(self, c):
        self.c = c
        self.targets = _targets(c.scores, c.excl, c.tags, c.any_of, c.none_of, c.S, c.dim)
        self.tptr, self.tit = csr(self.targets)
        self.masks = dict(any_of=c.any_of, none_of=c.none_of)
        self._store = None

    def store(self):
        """the 130 histories behind a memory of 5 (the ring wraps: histories have up to 6 items), their oracle scores, and the
        store's targets — specials taken under memory ∪ caller's list"""
        if self._store is None:
            c = self.c
            st, seen = _store_with_memory(c, 5, c.hists)
            c._closing.append(st)
            items = np.arange(ITEMS, dtype=np.uint32)
            scores = np.array([c.o.predict(r, items) for r in _rep_rows(c, c.hists)], np.float32).reshape(ROWS, ITEMS)
            lists = seen.excluded(c.slots, c.excl)
            targets = _targets(scores, lists, c.tags, c.any_of, c.none_of, c.S, c.dim + 7)
            self._store = (st, scores, lists, targets, seen.seen(c.slots))
        return self._store

    def close(self):
        self.c.close()


def _same(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert np.array_equal(got, want), f"{what}: {bad.size} of {want.size} ranks differ, first at {bad[:5].tolist()}: {got[bad[:5]].tolist()} vs {want[bad[:5]].tolist()}"


# ------------------------------------------------------------------------------------------------
# 1. against the oracle's scores and the numpy expectation
# ------------------------------------------------------------------------------------------------
def body_filter(p):
    c = p.c
    _same(c.g.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=c.excl, **p.masks),
          expect_rows(c.scores, p.targets, c.excl, c.tags, c.any_of, c.none_of), "filter")
    _same(c.g.rank_targets_reps(c.reps, p.tptr, p.tit, **p.masks), expect_rows(c.scores, p.targets, None, c.tags, c.any_of, c.none_of),
          "filter, no lists")


def body_set(p):
    c = p.c
    _same(c.item_set.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=c.excl), expect_rows(c.scores, p.targets, c.excl, members=c.S), "set")
    _same(c.item_set.rank_targets_reps(c.reps, p.tptr, p.tit), expect_rows(c.scores, p.targets, members=c.S), "set, no lists")


def body_set_filter(p):
    c = p.c
    _same(c.item_set.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=c.excl, **p.masks),
          expect_rows(c.scores, p.targets, c.excl, c.tags, c.any_of, c.none_of, c.S), "set + filter")


def body_histories(p):
    """the histories source: the forward pass runs, the list is the history"""
    c = p.c
    st, scores = p.store()[:2]
    up, it = csr(c.hists)
    _same(c.g.rank_targets(up, it, p.tptr, p.tit, **p.masks), expect_rows(scores, p.targets, c.hists, c.tags, c.any_of, c.none_of), "histories")
    _same(c.item_set.rank_targets(up, it, p.tptr, p.tit, include_history=True, **p.masks),
          expect_rows(scores, p.targets, None, c.tags, c.any_of, c.none_of, c.S), "histories through the set, history included")


def body_store(p):
    c = p.c
    st, scores, lists, targets, seen = p.store()
    _same(st.rank_targets(c.slots, targets, exclude=c.excl), expect_rows(scores, targets, lists), "store: seen ∪ caller's list")
    _same(st.rank_targets(c.slots, targets), expect_rows(scores, targets, seen), "store: seen alone")
    _same(st.rank_targets(c.slots, targets, exclude=c.excl, include_seen=True), expect_rows(scores, targets, c.excl), "store: include_seen")
    _same(st.rank_targets(c.slots, csr(targets), exclude=c.excl, **p.masks), expect_rows(scores, targets, lists, c.tags, c.any_of, c.none_of),
          "store + filter")


def body_store_set_filter(p):
    c = p.c
    st, scores, lists, targets, seen = p.store()
    on = c.item_set.on(st)
    _same(on.rank_targets(c.slots, targets, exclude=c.excl, **p.masks), expect_rows(scores, targets, lists, c.tags, c.any_of, c.none_of, c.S),
          "store + set + filter")
    _same(on.rank_targets(c.slots, targets), expect_rows(scores, targets, seen, members=c.S),
          "store + set")


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
@pytest.mark.parametrize("body", [body_filter, body_set, body_set_filter], ids=lambda f: f.__name__[5:])
def test_against_the_oracle(cases, groups, case, body):
    body(cases(case))


@pytest.mark.parametrize("case", rc.STORE_CASES, ids=rc.case_id)
@pytest.mark.parametrize("body", [body_histories, body_store, body_store_set_filter], ids=lambda f: f.__name__[5:])
def test_stores_against_the_oracle(cases, groups, case, body):
    body(cases(case))


def test_the_targets_meet_every_special_case(cases):
    """the table of targets holds what the docstring promises, so the equalities above are not vacuous"""
    p = cases(rc.CASES[3])
    c = p.c
    assert {len(t) for t in p.targets} == set(COUNTS)
    want = expect_rows(c.scores, p.targets, c.excl, c.tags, c.any_of, c.none_of, c.S)
    assert (want == ITEMS).any() and (want == 1).any() and (want < ITEMS).sum() > 100
    ptr = p.tptr.astype(np.int64)
    double = listed_ok = False
    for u in range(ROWS):
        listed = {int(i) for i in c.excl[u].tolist()}
        forbidden = mask_list(ITEMS, (), c.tags, c.any_of[u], c.none_of[u])
        t = {int(i) for i in p.targets[u].tolist()}
        double |= bool(t & listed & forbidden)
        listed_ok |= bool(t & (listed - forbidden))
        if len(p.targets[u]) >= 16:
            r = want[ptr[u]: ptr[u + 1]]
            assert r[0] == r[1], "a duplicate target has its twin's rank"
    assert double and listed_ok
    assert c.any_of[127] != c.any_of[128] or c.none_of[127] != c.none_of[128]
    assert any(not (set(range(ITEMS)) - mask_list(ITEMS, (), c.tags, a, n)) for a, n in zip(c.any_of, c.none_of)), "a mask that allows nothing"


# ------------------------------------------------------------------------------------------------
# 2. equalities with calls that exist
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [rc.CASES[1], rc.CASES[8]], ids=rc.case_id)
def test_equalities_with_existing_calls(cases, groups, case):
    p = cases(case)
    c = p.c
    zero = np.zeros(ROWS, np.uint32)
    plain = c.g.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=c.excl)
    _same(c.g.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=c.excl, any_of=zero, none_of=zero), plain, "zero masks are the plain call")
    up, it = csr(c.hists)
    _same(c.g.rank_targets(up, it, p.tptr, p.tit, any_of=0, none_of=0), c.g.rank_targets(up, it, p.tptr, p.tit), "zero masks, histories")
    # the contract's own sentence: the parent's call with the mask list M
    got = c.item_set.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=c.excl, **p.masks)
    M = [np.array(sorted(mask_list(ITEMS, c.excl[u], c.tags, c.any_of[u], c.none_of[u], c.S)), np.uint32) for u in range(ROWS)]
    _same(got, c.g.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=M), "rank_targets_reps(exclude=M)")
    # a set of every item is the model's call
    whole = c.g.item_set(np.arange(ITEMS, dtype=np.uint32))
    _same(whole.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=c.excl, **p.masks),
          c.g.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=c.excl, **p.masks), "the full-catalogue set")
    whole.close()
    # the only route there was: one count_above row per target, at the target's own score
    filtered = c.g.rank_targets_reps(c.reps, p.tptr, p.tit, exclude=c.excl, **p.masks)
    ptr = p.tptr.astype(np.int64)
    rows = [u for u in range(ROWS) if len(p.targets[u])][:24]
    per = c.g.score_candidates_reps(c.reps[rows], *csr([p.targets[u] for u in rows]))
    rr, th, ex, an, no, at = [], [], [], [], [], []
    for j, u in enumerate(rows):
        m = mask_list(ITEMS, c.excl[u], c.tags, c.any_of[u], c.none_of[u])
        for e, t in enumerate(p.targets[u].tolist()):
            if t not in m:
                rr.append(c.reps[u]); th.append(per[j][e]); ex.append(c.excl[u]); an.append(c.any_of[u]); no.append(c.none_of[u]); at.append(ptr[u] + e)
    assert len(at) > 20
    counts = c.g.count_above_reps(np.array(rr, np.float32), np.array(th, np.float32), exclude=ex, any_of=np.array(an, np.uint32), none_of=np.array(no, np.uint32))
    _same(filtered[np.array(at)], counts.astype(np.uint32), "count_above_reps at the target's score")


@pytest.mark.parametrize("case", [rc.STORE_CASES[0], rc.STORE_CASES[3]], ids=rc.case_id)
def test_sessions_equal_rank_targets_reps(cases, groups, case):
    p = cases(case)
    c = p.c
    st, _, lists, targets = p.store()[:4]
    tp, ti = csr(targets)
    _same(st.rank_targets(c.slots, targets, exclude=c.excl), c.g.rank_targets_reps(st.representations(c.slots), tp, ti, exclude=lists),
          "Sessions.rank_targets")


# ------------------------------------------------------------------------------------------------
# 3. the same bodies on poisoned scratch and between guard bands
# ------------------------------------------------------------------------------------------------
ALL_BODIES = (body_filter, body_set, body_set_filter, body_histories, body_store, body_store_set_filter)


@pytest.mark.parametrize("pattern", [0xFF, 0x7F], ids=lambda x: f"poison{x:02X}")
@pytest.mark.parametrize("case", [rc.STORE_CASES[1], rc.CASES[4]], ids=rc.case_id)
def test_on_poisoned_scratch(cases, monkeypatch, pattern, case):
    """SBR_TEST_POISON as tests/test_poisoned_scratch_gpu.py sets it (that module proves the hook is live); twice, so that the second
    pass meets what the first left in the arena"""
    monkeypatch.setenv("SBR_TEST_POISON", str(pattern))
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", "3")
    p = cases(case)
    for _ in range(2):
        for body in ALL_BODIES:
            body(p)


@pytest.mark.parametrize("case", [rc.STORE_CASES[1], rc.CASES[4]], ids=rc.case_id)
def test_between_guard_bands(cases, guard, case):
    """SBR_TEST_GUARD=256: the fixture asserts violations == 0 and checked > 0 behind the bodies"""
    p = cases(case)
    for body in ALL_BODIES:
        body(p)


# ------------------------------------------------------------------------------------------------
# 4. errors, each leaving state untouched
# ------------------------------------------------------------------------------------------------
def _small(tags=True):
    rs = np.random.RandomState(5)
    d = 16
    g = Model(hparams(ITEMS, 16, d, int(ModelKind.EWMA), LOSS_HINGE, B=8))
    E = (rs.randn(ITEMS, d) * 0.3).astype(np.float32)
    g.set_param(Param.ITEM_EMBEDDING, E.ravel())
    g.set_param(Param.ITEM_BIAS, (rs.randn(ITEMS) * 0.1).astype(np.float32))
    if tags:
        g.set_item_tags(rs.randint(0, 8, ITEMS).astype(np.uint32))
    reps = (rs.randn(5, d) * 0.5).astype(np.float32)
    targets = [rs.randint(0, ITEMS, 4).astype(np.uint32) for _ in range(5)]
    return g, E, reps, csr(targets)


def test_errors_leave_state_untouched():
    g, E, reps, (tp, ti) = _small()
    S = np.arange(0, ITEMS, 2, dtype=np.uint32)
    s = g.item_set(S)
    st = g.sessions(8, remember=4)
    slots = np.arange(5, dtype=np.uint32)
    st.append(slots, [[1, 2, 3]] * 5)
    good = s.rank_targets_reps(reps, tp, ti, any_of=3)
    good_store = st.rank_targets(slots, (tp, ti), none_of=4)
    # a target id out of range
    bad = ti.copy()
    bad[3] = ITEMS
    with pytest.raises(EngineError):
        g.rank_targets_reps(reps, tp, bad, any_of=1)
    with pytest.raises(ValueError):
        s.rank_targets_reps(reps, tp, bad)
    # include_seen on a store without memory
    plain_store = g.sessions(8)
    with pytest.raises(ValueError):
        plain_store.rank_targets(slots, (tp, ti), include_seen=True)
    plain_store.close()
    _same(s.rank_targets_reps(reps, tp, ti, any_of=3), good, "after the argument errors")
    # a non-finite row outside the set fails nothing; inside it fails the call, allowed by the masks or not
    for item, inside in ((1, False), (2, True)):
        E2 = E.copy()
        E2[item, 0] = np.inf
        g.set_param(Param.ITEM_EMBEDDING, E2.ravel())
        with pytest.raises(ValueError):  # stale: the parameters changed under the set and the store
            s.rank_targets_reps(reps, tp, ti)
        with pytest.raises(EngineError):
            st.rank_targets(slots, (tp, ti))
        s.refresh()
        if inside:
            with pytest.raises(PredictionError.InvalidPredictionValue):
                s.rank_targets_reps(reps, tp, ti, any_of=3)
            with pytest.raises(PredictionError.InvalidPredictionValue):
                s.rank_targets_reps(reps, tp, ti, any_of=1 << 30)  # no item carries the bit: nothing is allowed, the score still fails
        else:
            s.rank_targets_reps(reps, tp, ti, any_of=3)
            with pytest.raises(PredictionError.InvalidPredictionValue):
                g.rank_targets_reps(reps, tp, ti, any_of=3)
    g.set_param(Param.ITEM_EMBEDDING, E.ravel())
    s.refresh()
    _same(s.rank_targets_reps(reps, tp, ti, any_of=3), good, "after the refresh")
    st.reset()  # every slot: the store is current again
    st.append(slots, [[1, 2, 3]] * 5)
    _same(st.rank_targets(slots, (tp, ti), none_of=4), good_store, "the store, rebuilt")
    # an empty set answers on the host
    empty = g.item_set(np.zeros(0, np.uint32))
    assert (empty.rank_targets_reps(reps, tp, ti) == ITEMS).all()
    for x in (empty, s, st):
        x.close()
    g.close()


def test_a_filter_needs_tags():
    g, _, reps, (tp, ti) = _small(tags=False)
    with pytest.raises(EngineError):
        g.rank_targets_reps(reps, tp, ti, any_of=1)
    s = g.item_set(np.arange(10, dtype=np.uint32))
    with pytest.raises(ValueError):
        s.rank_targets_reps(reps, tp, ti, none_of=1)
    assert s.rank_targets_reps(reps, tp, ti).size == ti.size  # without masks the set needs none
    s.close()
    g.close()
