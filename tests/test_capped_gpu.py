"""GPU: sbr_recommend_capped / _reps / sbr_sessions_recommend_capped (the group cap over recommend's pool, capped_select_kernel in
sbr_catalogue.hip) against the contract stated in capped_expect.py over the oracle's scores.  Everything is equality: items and
flags as integers, scores by their f32 bits.  Embeddings and biases are planted as in test_diverse_gpu.py (duplicate rows, biases on
a 0.1 grid), so ties decide orders.  The rankings of a configuration are computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

from capped_expect import NO_GROUP, capped_rows, rankings_from_histories, rankings_from_reps, rule_ordinal
from filter_expect import allowed, masks_of
from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM
from sbr_rs_amd._abi import ModelKind, Param, SbrCapArgs, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, PredictionError

pytestmark = pytest.mark.gpu

_USERS = 70
_T = 8
_KP = ((1, 1), (10, 10), (10, 64), (33, 255), (33, 256), (33, 257), (100, 1024))
_CONFIGS = [(16, 1500, ModelKind.LSTM_NORMAL), (16, 1500, ModelKind.EWMA), (128, 2000, ModelKind.LSTM_NORMAL), (128, 2000, ModelKind.EWMA)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    gi, gs, gc = got
    wi, ws, wc = want
    assert gi.shape == wi.shape, (what, gi.shape, wi.shape)
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: {len(bad)} items differ; first at {bad[0]}: {gi[tuple(bad[0])]} vs {wi[tuple(bad[0])]}"
    assert np.array_equal(_bits(gs), _bits(ws)), what
    assert np.array_equal(np.asarray(gc, dtype=bool), np.asarray(wc, dtype=bool)), (what, np.flatnonzero(np.asarray(gc, bool) != wc))


def _planted(items, d, seed):
    """0.3 * randn with 20 copies of row 0 (exact ties), a zero row, a doubled and a negated row; biases on a 0.1 grid (score
    ties)."""
    rs = np.random.RandomState(seed)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    E[rs.choice(np.arange(10, items), 20, replace=False)] = E[0]
    E[5] = 0.0
    E[7] = 2.0 * E[3]
    E[9] = -E[3]
    bias = np.round(rs.randn(items) * 0.5, 1).astype(np.float32)
    return E, bias


def _pair(items, d, kind, E=None, bias=None):
    hp = hparams(items, _T, d, int(kind), LOSS_HINGE, B=8)
    g, o = Model(hp), OracleModel(hp)
    for m in (g, o):
        if E is not None:
            m.set_param(Param.ITEM_EMBEDDING, E)
        if bias is not None:
            m.set_param(Param.ITEM_BIAS, bias)
    return g, o


class _Case:
    """One configuration: the model pair, the users, and every ranking the tests need, made once."""

    def __init__(self, d, items, kind):
        self.d, self.items = d, items
        E, bias = _planted(items, d, d + items)
        self.g, self.o = _pair(items, d, kind, E, bias)
        self.ptr, self.it = synthetic_interactions(_USERS, items, 3 * _T, seed=d, min_len=0, zipf=True)
        self.reps = self.g.user_representations(self.ptr, self.it)
        rs = np.random.RandomState(d)
        self.excl = [rs.randint(0, items, rs.randint(0, 30)) for _ in range(_USERS)]
        self.excl[0] = np.delete(np.arange(items), 17)  # n == 1
        self.excl[1] = np.arange(5, items)[::-1]         # n == 5: below k from 10 on
        self.excl[2] = np.arange(40, items)              # n == 40: k <= n < pool from (10, 64) on
        self.tags = rs.randint(0, 16, items).astype(np.uint32)
        self.any_of = rs.randint(0, 16, _USERS).astype(np.uint32)
        self.none_of = 8
        a, n = masks_of(self.any_of, _USERS), masks_of(self.none_of, _USERS)
        ok = np.array([allowed(self.tags, a[u], n[u]) for u in range(_USERS)])
        self.ranks = {"masked": rankings_from_histories(self.o, items, self.ptr, self.it),
                      "kept": rankings_from_histories(self.o, items, self.ptr, self.it, include_history=True),
                      "reps": rankings_from_reps(self.o, items, self.reps, self.excl),
                      "tags": rankings_from_reps(self.o, items, self.reps, self.excl, ok)}
        self.g.set_item_tags(self.tags)

    def patterns(self, k, cap):
        """the group patterns of test 1; `binds` is planted on user 5's ranking of the reps form: its k-th entry is the cap-th of
        group 12345 and the two entries behind it belong to that group too, so the cap binds exactly at the k-th kept entry"""
        items = self.items
        rs = np.random.RandomState(k * 31 + cap)
        own = np.arange(items, dtype=np.uint32)
        binds = own.copy() + 100000
        ids = self.ranks["reps"][5][0]
        binds[ids[np.r_[np.arange(cap - 1), k - 1, k, k + 1]]] = 12345
        return {"own": own, "none": np.full(items, NO_GROUP, np.uint32),
                "edge": rs.choice(np.array([0, 0xFFFFFFFE], dtype=np.uint32), items),
                "big": np.where(rs.rand(items) < 0.7, 7, own).astype(np.uint32),  # > 256 entries of one group in a pool of 1 024
                "binds": binds}

    def call(self, form, k, cap, pool, exact=False):
        g = self.g
        if form == "masked":
            return g.recommend_capped(self.ptr, self.it, k, cap, pool, exact=exact)
        if form == "kept":
            return g.recommend_capped(self.ptr, self.it, k, cap, pool, include_history=True, exact=exact)
        if form == "reps":
            return g.recommend_capped_reps(self.reps, k, cap, pool, exclude=self.excl, exact=exact)
        return g.recommend_capped_reps(self.reps, k, cap, pool, exclude=self.excl, any_of=self.any_of, none_of=self.none_of, exact=exact)


@functools.lru_cache(maxsize=None)
def _case(d, items, kind):
    return _Case(d, items, kind)


@pytest.mark.parametrize("d,items,kind", _CONFIGS)
def test_matches_the_c_level_expectation(d, items, kind):
    c = _case(d, items, kind)
    for k, pool in _KP:
        for cap in sorted({1, 2, k}):
            pats = c.patterns(k, cap)
            for name, groups in pats.items():
                c.g.set_item_groups(groups)
                assert np.array_equal(c.g.item_groups(), groups)
                forms = ("reps", "masked", "kept", "tags") if name in ("big", "edge") else ("reps",)
                for form in forms:
                    what = f"k={k} pool={pool} cap={cap} {name} {form}"
                    got = c.call(form, k, cap, pool)
                    _same(got, capped_rows(c.ranks[form], groups, cap, k, pool, rule_ordinal), what)
                    if form in ("reps", "tags") and name != "edge":  # the rows the exclusion lists make short: complete by padding
                        assert got[2][0] and got[0][0, 0] in (17, NO_ITEM) and np.all(got[0][0, 1:] == NO_ITEM) and np.all(np.isneginf(got[1][0, 1:]))
                        assert got[2][1] and np.all(got[0][1, 5:] == NO_ITEM)
                        assert got[2][2] or pool <= 40
            if pool > k + 1:  # the planted row: the cap binds at the k-th kept entry, so the row is the ranking's first k
                c.g.set_item_groups(pats["binds"])
                gi, gs, gc = c.call("reps", k, cap, pool)
                assert np.array_equal(gi[5], c.ranks["reps"][5][0][:k]) and gc[5]


@pytest.mark.parametrize("d,items,kind", _CONFIGS[1:3])
def test_identities(d, items, kind):
    c = _case(d, items, kind)
    for k, pool in _KP:
        plain = c.g.recommend_reps(c.reps, k, exclude=c.excl)
        hist = c.g.recommend(c.ptr, c.it, k)
        pats = c.patterns(k, 1)
        for groups, cap in ((pats["own"], 1), (pats["none"], 1), (pats["edge"], k), (pats["big"], k + 3)):
            c.g.set_item_groups(groups)
            for exact in (False, True):
                gi, gs, gc = c.g.recommend_capped_reps(c.reps, k, cap, pool, exclude=c.excl, exact=exact)
                assert np.array_equal(gi, plain[0]) and np.array_equal(_bits(gs), _bits(plain[1])) and gc.all(), (k, pool, cap)
            gi, gs, gc = c.g.recommend_capped(c.ptr, c.it, k, cap, pool, exact=False)
            assert np.array_equal(gi, hist[0]) and np.array_equal(_bits(gs), _bits(hist[1])) and gc.all()


@pytest.mark.parametrize("d,items,kind", _CONFIGS[:1] + _CONFIGS[3:])
def test_one_large_group_collapsed_and_completed(d, items, kind):
    """cap = 1 with one large group: a pool of 64 settles some rows and not others; exact=True finishes the rest."""
    c = _case(d, items, kind)
    k, pool = 10, 64
    groups = np.where(np.random.RandomState(4).rand(items) < 0.86, 7, np.arange(items)).astype(np.uint32)
    for form in ("masked", "reps", "tags"):
        at_pool = capped_rows(c.ranks[form], groups, 1, k, pool)
        exact = capped_rows(c.ranks[form], groups, 1, k)
        short = ~at_pool[2]
        assert short.sum() >= 5 and at_pool[2].sum() >= 5, (form, int(short.sum()))  # the planted share does what it is there for
        c.g.set_item_groups(groups)
        lib = c.call(form, k, 1, pool, exact=False)
        _same(lib, at_pool, form)
        for u in np.flatnonzero(short):  # a prefix of the exact answer, then padding
            n = int(np.count_nonzero(lib[0][u] != NO_ITEM))
            assert n < k and np.array_equal(lib[0][u, :n], exact[0][u, :n]) and np.all(lib[0][u, n:] == NO_ITEM)
        done = c.call(form, k, 1, pool, exact=True)
        _same(done, exact, form + " exact")
        assert done[2].all()
        for u in range(_USERS):
            n = int(np.count_nonzero(lib[0][u] != NO_ITEM))
            assert np.array_equal(done[0][u, :n], lib[0][u, :n]) and np.array_equal(_bits(done[1][u, :n]), _bits(lib[1][u, :n]))


@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA])
def test_sessions(kind):
    items, d, n, w = 900, 16, 40, 6
    E, bias = _planted(items, d, 5)
    g, _ = _pair(items, d, kind, E, bias)
    rs = np.random.RandomState(9)
    groups = np.where(rs.rand(items) < 0.8, 3, rs.randint(10, 60, items)).astype(np.uint32)
    g.set_item_groups(groups)
    g.set_item_tags(rs.randint(0, 8, items).astype(np.uint32))
    h = [rs.randint(0, items, size=i % 9).astype(np.uint32) for i in range(n)]
    slots = rs.permutation(n + 5)[:n].astype(np.uint32)
    caller = [rs.randint(0, items, size=rs.randint(0, 4)).astype(np.uint32) for _ in range(n)]
    for remember in (w, 0):
        store = g.sessions(n + 5, remember=remember)  # made behind the last set_param: current
        store.append(slots, h)
        reps = store.representations(slots)
        seen = store.seen(slots) if store.seen_capacity else [np.zeros(0, np.uint32)] * n
        both = [np.concatenate([a, b]) for a, b in zip(seen, caller)]
        for k, cap, pool, exact in ((10, 1, 16, False), (10, 1, 16, True), (5, 2, None, False), (20, 1, 64, True)):
            got = store.recommend_capped(slots, k, cap, pool, exclude=caller, exact=exact)
            _same(got, g.recommend_capped_reps(reps, k, cap, pool, exclude=both, exact=exact), f"{k} {cap} {pool} {exact}")
            got = store.recommend_capped(slots, k, cap, pool, any_of=3, none_of=4, exact=exact)
            _same(got, g.recommend_capped_reps(reps, k, cap, pool, exclude=seen, any_of=3, none_of=4, exact=exact), "masks")
            if store.seen_capacity:
                got = store.recommend_capped(slots, k, cap, pool, exclude=caller, include_seen=True, exact=exact)
                _same(got, g.recommend_capped_reps(reps, k, cap, pool, exclude=caller, exact=exact), "include_seen")
            else:
                with pytest.raises(ValueError):
                    store.recommend_capped(slots, k, cap, pool, include_seen=True)
        # a stale store refuses
        g.set_param(Param.ITEM_BIAS, bias)
        with pytest.raises(EngineError) as e:
            store.recommend_capped(slots, 5)
        assert e.value.status == Status.INVALID_ARGUMENT
        store.close()


@pytest.mark.parametrize("forced", [None, "1", "3"])
def test_more_rows_than_one_launch_chunk_and_forced_item_ranges(forced, monkeypatch):
    if forced is not None:
        monkeypatch.setenv("SBR_CATALOGUE_GROUPS", forced)
    items, d, k, cap, pool = 300, 16, 10, 1, 32
    E, bias = _planted(items, d, 8)
    g, o = _pair(items, d, ModelKind.EWMA, E, bias)
    base = (np.random.RandomState(3).randn(_USERS, d) * 0.4).astype(np.float32)
    rows = 8192 + _USERS
    reps = base[np.arange(rows) % _USERS]
    groups = np.where(np.random.RandomState(6).rand(items) < 0.8, 9, np.arange(items)).astype(np.uint32)
    g.set_item_groups(groups)
    want = capped_rows(rankings_from_reps(o, items, base), groups, cap, k, pool)
    assert 0 < want[2].sum() < _USERS
    at = np.arange(rows) % _USERS
    _same(g.recommend_capped_reps(reps, k, cap, pool, exact=False), tuple(w[at] for w in want), f"groups={forced}")
    if forced is None:  # the completion over more rows than one chunk
        exact = capped_rows(rankings_from_reps(o, items, base), groups, cap, k)
        _same(g.recommend_capped_reps(reps, k, cap, pool), tuple(w[at] for w in exact), "exact")


def test_refusals_leave_the_outputs_untouched():
    items, d, n, k = 400, 16, 9, 5
    g, _ = _pair(items, d, ModelKind.EWMA, *_planted(items, d, 2))
    reps = (np.random.RandomState(1).randn(n, d) * 0.5).astype(np.float32)
    ptr, it = synthetic_interactions(n, items, 10, seed=1)
    ptr, it = np.ascontiguousarray(ptr, np.uint64), np.ascontiguousarray(it, np.uint32)
    store = g.sessions(n)
    slots = np.arange(n, dtype=np.uint32)
    store.append(slots, [[1, 2]] * n)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    oi, osc, oc = np.full((n, k), 7, np.uint32), np.full((n, k), 7.0, np.float32), np.full(n, 7, np.uint8)
    mask = np.zeros(n, np.uint32)

    def all_three(ca, any_of=None, none_of=None):
        a = None if any_of is None else vp(any_of)
        b = None if none_of is None else vp(none_of)
        return [g._L.sbr_recommend_capped(g._h, vp(ptr), vp(it), n, k, 0, ca, a, b, vp(oi), vp(osc), vp(oc)),
                g._L.sbr_recommend_capped_reps(g._h, vp(reps), n, k, None, None, ca, a, b, vp(oi), vp(osc), vp(oc)),
                g._L.sbr_sessions_recommend_capped(store._h, vp(slots), n, k, None, None, 0, ca, a, b, vp(oi), vp(osc), vp(oc))]

    def args(cap, pool):
        ca = SbrCapArgs()
        ca.cap, ca.pool = cap, pool
        return C.byref(ca)

    assert all_three(args(1, 0)) == [Status.INVALID_ARGUMENT] * 3  # no groups set
    with pytest.raises(EngineError):
        g.item_groups()
    g.set_item_groups(np.arange(items) % 50)
    for ca in (args(0, 0), args(1, k - 1), args(1, 1025), None):
        assert all_three(ca) == [Status.INVALID_ARGUMENT] * 3
    assert all_three(args(1, 0), mask, mask) == [Status.INVALID_ARGUMENT] * 3  # masks without tags
    assert all_three(args(1, 0), mask) == [Status.INVALID_ARGUMENT] * 3
    assert np.all(oi == 7) and np.all(osc == 7.0) and np.all(oc == 7)
    # the same through the Python layer, and the optional outputs
    for kw in ({"any_of": 1}, {"none_of": mask}):
        with pytest.raises(EngineError) as e:
            g.recommend_capped_reps(reps, k, **kw)
        assert e.value.status == Status.INVALID_ARGUMENT
    assert g._L.sbr_recommend_capped_reps(g._h, vp(reps), n, k, None, None, args(1, 0), None, None, vp(oi), None, None) == Status.OK
    want = g.recommend_capped_reps(reps, k, exact=False)
    assert np.array_equal(oi, want[0]) and np.all(osc == 7.0) and np.all(oc == 7)
    g.set_item_groups(None)
    assert all_three(args(1, 0)) == [Status.INVALID_ARGUMENT] * 3
    store.close()


def test_a_non_finite_score_fails_the_call():
    items, d = 700, 16
    E, bias = _planted(items, d, 1)
    ptr, it = synthetic_interactions(20, items, 10, seed=1)
    for where in ("E", "b"):
        E2, b2 = E.copy(), bias.copy()
        if where == "E":
            E2[123, 3] = np.inf
        else:
            b2[45] = np.inf
        g, _ = _pair(items, d, ModelKind.EWMA, E2, b2)
        g.set_item_groups(np.arange(items) % 9)
        with pytest.raises(PredictionError.InvalidPredictionValue):
            g.recommend(ptr, it, 10)
        with pytest.raises(PredictionError.InvalidPredictionValue):
            g.recommend_capped(ptr, it, 10)
        with pytest.raises(PredictionError.InvalidPredictionValue):
            g.recommend_capped_reps(np.ones((3, d), np.float32), 10, cap=2, pool=10, exact=False)


def test_groups_are_serving_metadata():
    """Setting groups leaves a session store current and recommend's output bit-equal; set_param leaves the groups alone."""
    items, d = 500, 16
    E, bias = _planted(items, d, 6)
    g, _ = _pair(items, d, ModelKind.LSTM_NORMAL, E, bias)
    ptr, it = synthetic_interactions(30, items, 10, seed=2)
    store = g.sessions(4)
    store.append([0, 1], [[1, 2, 3], [4]])
    before = g.recommend(ptr, it, 20)
    sess_before = store.recommend([0, 1], 7)
    groups = (np.arange(items) % 11).astype(np.uint32)
    g.set_item_groups(groups)
    after = g.recommend(ptr, it, 20)
    assert np.array_equal(before[0], after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
    sess_after = store.recommend([0, 1], 7)  # still current
    assert np.array_equal(sess_before[0], sess_after[0])
    gi, _, gc = store.recommend_capped([0, 1], 7)
    assert gc.all() and all(len(set((groups[r]).tolist())) == 7 for r in gi)
    g.set_param(Param.ITEM_BIAS, bias)
    assert np.array_equal(g.item_groups(), groups)
    g.set_item_groups(None)
    with pytest.raises(EngineError):
        g.recommend_capped(ptr, it, 5)
    store.close()
