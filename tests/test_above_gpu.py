"""GPU: the threshold form of the scans — above_gemm_kernel (count, then fill) and above_offsets_kernel of sbr_catalogue.hip behind
sbr_recommend_above / _reps / sbr_sessions_recommend_above and sbr_audience_above / _reps / sbr_sessions_audience_above.  The result
is a set with exact scores, so tests/above_expect.py states the contract a second time in numpy and everything here is equality:
ids and counts as integers, scores by their f32 bits, against that expectation (over the oracle's or designed exact scores) or of
the device with itself.  Shapes, cases and helpers are those of tests/test_sampled_gpu.py; the number of item ranges is forced with
SBR_CATALOGUE_GROUPS as there."""
import ctypes as C

import numpy as np
import pytest

from above_expect import above_expect, counts_expect, transposed
from filter_expect import allowed, equivalent_exclusions, masks_of
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import RECOMMEND_MAX_K
from sbr_rs_amd.errors import EngineError, PredictionError
from test_sampled_gpu import CORE_ITEMS, CORE_T, CORE_USERS, _bits, _core_case, _filter_case, _force, _model, _oracle_of, _random_params, _rep_scores

pytestmark = pytest.mark.gpu

FILL_HOOK = "SBR_ABOVE_FILL_BYTES"


def _same(got, want, what=""):
    """an Above against (ptr, ids, scores): pointers and ids as integers, scores bit for bit"""
    ptr, ids, scores = want
    assert got.ptr.dtype == np.uint64 and got.ids.dtype == np.uint32 and got.scores.dtype == np.float32
    assert np.array_equal(got.ptr, ptr), f"{what}: counts differ; first at row {np.argwhere(np.diff(got.ptr) != np.diff(ptr))[:1]}"
    bad = np.argwhere(got.ids != ids)
    assert bad.size == 0, f"{what}: {len(bad)} ids differ; first at entry {bad[0]}: {got.ids[bad[0][0]]} vs {ids[bad[0][0]]}"
    bad = np.argwhere(_bits(got.scores) != _bits(scores))
    assert bad.size == 0, f"{what}: {len(bad)} score bits differ; first at entry {bad[0]}: {got.scores[bad[0][0]]!r} vs {scores[bad[0][0]]!r}"


def _triple(a):
    return a.ptr, a.ids, a.scores


def _both_orders(call, count, scores, t, excluded=None, allow=None, ids=None, what=""):
    """call(order=...) in both orders against the expectation, and count() against diff(ptr)"""
    for order in ("score", "id"):
        got = call(order=order)
        _same(got, above_expect(scores, t, excluded, allow, order, ids), f"{what} order={order}")
    n = count()
    assert n.dtype == np.uint64 and np.array_equal(n, np.diff(got.ptr)) and np.array_equal(n, counts_expect(scores, t, excluded, allow)), what
    return got


def _quantile_thresholds(scores):
    """Per row its own thresholds: rows return about 5 (u % 3 == 0), about 300 — across several tiles — (1) and all (2) of their
    items; "about": history items among the best are excluded afterwards, and ties pass together."""
    s = -np.sort(-scores.astype(np.float64), axis=1)
    u = np.arange(len(scores))
    return np.where(u % 3 == 0, s[:, 4], np.where(u % 3 == 1, s[:, 299], s[:, -1])).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# core: histories through the recurrent forward, against the oracle's scores
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA], ids=lambda k: k.name)
def test_core_against_the_oracle(monkeypatch, kind, d, groups):
    """1 000 items (32 tiles, the last one ragged) x 130 users (the second row tile nearly empty), per-row thresholds at the row's
    own quantiles, history excluded and included, forced to 1 range and to 3."""
    _force(monkeypatch, groups)
    E, bias, params, ptr, it, hists, scores = _core_case(kind, d)
    g = _model(CORE_ITEMS, CORE_T, d, kind, E, bias)
    for w, v in params.items():
        g.set_param(w, v)
    uniq = [np.unique(h) for h in hists]
    t = _quantile_thresholds(scores)
    for include in (False, True):
        got = _both_orders(lambda order: g.recommend_above(ptr, it, t, include_history=include, order=order),
                           lambda: g.count_above(ptr, it, t, include_history=include), scores, t, None if include else uniq,
                           what=f"include={include}")
        n = got.counts
        assert n[0::3].max() <= 5 and n[1::3].min() > 250 and n[1::3].max() <= 300 and n[2::3].min() >= CORE_ITEMS - 2 * CORE_T
        if include:
            assert np.all(n[0::3] == 5) and np.all(n[1::3] == 300) and np.all(n[2::3] == CORE_ITEMS)


@pytest.mark.parametrize("d", [16, 32, 64, 128, 256])
def test_every_storage_width(d):
    """Every width the kernel is instantiated at, 200 items x 40 rows, with exclusion lists; both orientations."""
    items, users = 200, 40
    E, bias = _random_params(items, d, d)
    rs = np.random.RandomState(d + 1)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    excl = [rs.randint(0, items, u % 7).astype(np.uint32) for u in range(users)]
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps)
    t = np.quantile(scores, 0.8, axis=1).astype(np.float32)
    _both_orders(lambda order: g.recommend_above_reps(reps, t, order=order), lambda: g.count_above_reps(reps, t), scores, t, what=f"d={d}")
    _both_orders(lambda order: g.recommend_above_reps(reps, t, exclude=excl, order=order), lambda: g.count_above_reps(reps, t, exclude=excl),
                 scores, t, excl, what=f"d={d} lists")
    q = rs.permutation(items)[:30].astype(np.uint32)
    qex = [rs.randint(0, users, j % 5).astype(np.uint32) for j in range(len(q))]
    tq = np.quantile(scores.T[q], 0.6, axis=1).astype(np.float32)
    _both_orders(lambda order: g.audience_above_reps(reps, q, tq, exclude=qex, order=order),
                 lambda: g.count_audience_above_reps(reps, q, tq, exclude=qex), np.ascontiguousarray(scores.T[q]), tq, qex, what=f"d={d} audience")


# ------------------------------------------------------------------------------------------------
# designed exact scores
# ------------------------------------------------------------------------------------------------
DES_ITEMS = 1100  # 35 tiles, the last one ragged


def _designed(col0, bias=None, users=4):
    """d = 16, reps[u] = (1, 0, ...), E[i] = (col0[i], 0, ...): the score of every user is bias[i] + col0[i], exact in f32."""
    E = np.zeros((DES_ITEMS, 16), np.float32)
    E[:, 0] = col0
    b = np.zeros(DES_ITEMS, np.float32) if bias is None else np.asarray(bias, np.float32)
    reps = np.zeros((users, 16), np.float32)
    reps[:, 0] = 1.0
    scores = np.tile((b + E[:, 0]).astype(np.float32), (users, 1))
    return _model(DES_ITEMS, 8, 16, ModelKind.EWMA, E, b), reps, scores


@pytest.mark.parametrize("groups", [1, 4])
def test_designed_ties_zeros_and_infinite_thresholds(monkeypatch, groups):
    """Scores on a grid of 1/8 with seven items exactly at the bar 2.0 in different tiles; two zero scores against thresholds +0.0
    and -0.0; t = -inf and t = +inf; an unsorted, repeating exclusion list that holds passing items."""
    _force(monkeypatch, groups)
    rs = np.random.RandomState(2)
    col = (np.round(rs.randn(DES_ITEMS) * 8) / 8).astype(np.float32)
    col[col == 2.0] = 2.125
    col[col == 0.0] = 0.125
    at_bar = np.array([3, 31, 32, 500, 777, 1087, 1099])
    col[at_bar] = 2.0
    b = np.zeros(DES_ITEMS, np.float32)
    col[40], b[40] = -0.0, -0.0  # two zero scores; what sign the chain leaves them is the device's to say (read back below)
    col[41] = 0.0
    col[900] = -1.0  # row 5 excludes it too, and it does not pass
    g, reps, scores = _designed(col, b, users=6)
    dev = g.recommend_above_reps(reps[:1], -np.inf, order="id")
    assert dev.counts[0] == DES_ITEMS and np.array_equal(dev.ids, np.arange(DES_ITEMS))
    scores = np.tile(dev.scores, (6, 1))  # the device's own bits: a zero's sign is whatever the chain computes
    assert np.array_equal(scores[0] == 0, (np.arange(DES_ITEMS) == 40) | (np.arange(DES_ITEMS) == 41))
    assert np.array_equal(np.delete(scores[0], [40, 41]), np.delete(col + b, [40, 41]))
    t = np.array([2.0, 0.0, -0.0, -np.inf, np.inf, 2.0], np.float32)
    excl = [[], [], [], [5, 1099, 5], [], [777, 3, 777, 900, 3]]
    got = _both_orders(lambda order: g.recommend_above_reps(reps, t, exclude=excl, order=order),
                       lambda: g.count_above_reps(reps, t, exclude=excl), scores, t, excl, what="designed")
    above_bar = int(np.count_nonzero(col > 2.0))
    r0 = g.recommend_above_reps(reps, t, exclude=excl).row(0)  # score order: the seven at the bar come last, by id
    assert got.counts[0] == above_bar + 7 and r0[0][-7:].tolist() == at_bar.tolist() and np.all(r0[1][-7:] == 2.0)
    zeros0, zeros1 = got.row(1), got.row(2)
    for ids, sc in (zeros0, zeros1):  # both zeros pass either zero threshold, the lower id first, bits as computed
        z = sc == 0
        assert ids[z].tolist() == [40, 41] and np.array_equal(_bits(sc[z]), _bits(scores[0, [40, 41]]))
    assert got.counts[3] == DES_ITEMS - 2 and got.counts[4] == 0
    assert got.counts[5] == got.counts[0] - 2 and not np.isin([777, 3], got.row(5)[0]).any()
    plain = g.recommend_above_reps(reps[:1], 2.0)
    assert plain.counts[0] == above_bar + 7


def test_negative_zero_score_passes_a_positive_zero_threshold():
    """Item 100 has a -0.0 bias and an embedding row of 1e-30 throughout; row 0 is -1e-30 throughout: every product of the chain
    underflows to -0.0, the chain ends at -0.0 and the score is -0.0 (the oracle says so).  It passes t = +0.0, after the +0.0 score
    of item 50 in id order and tied with it in score order, and its sign bit is reported as computed; item 60 scores -1e-30 * 1.0 * 16
    and does not pass."""
    items, d = 200, 16
    E = np.zeros((items, d), np.float32)
    b = np.full(items, -1.0, np.float32)
    E[100], b[100] = 1e-30, -0.0
    b[50] = 0.0
    E[60], b[60] = 1.0, 0.0
    reps = np.full((2, d), -1e-30, np.float32)
    reps[1] = 0.0
    g = _model(items, 8, d, ModelKind.EWMA, E, b)
    scores = _rep_scores(_oracle_of(g), items, reps)
    assert scores[0, 100] == 0 and np.signbit(scores[0, 100]) and scores[0, 50] == 0 and not np.signbit(scores[0, 50]) and scores[0, 60] < 0
    for t in (np.float32(0.0), np.float32(-0.0)):
        got = _both_orders(lambda order: g.recommend_above_reps(reps, t, order=order), lambda: g.count_above_reps(reps, t), scores, t, what=f"t={t!r}")
        assert got.row(0)[0].tolist() == [50, 100] and np.signbit(got.row(0)[1]).tolist() == [False, True]
        assert g.recommend_above_reps(reps, t).row(0)[0].tolist() == [50, 100]


def test_flat_scores_count_the_allowed_items():
    """All scores 0.25: the count is the allowed count at t <= 0.25 and zero above it; repeats in a list count once."""
    g, reps, scores = _designed(np.zeros(DES_ITEMS, np.float32), np.full(DES_ITEMS, 0.25, np.float32))
    excl = [[], [1, 2, 3], [7, 7, 7, 1099, 0, 1099], list(range(0, DES_ITEMS, 2))]
    n = g.count_above_reps(reps, 0.25, exclude=excl)
    assert n.tolist() == [DES_ITEMS, DES_ITEMS - 3, DES_ITEMS - 3, DES_ITEMS // 2]
    _same(g.recommend_above_reps(reps, 0.25, exclude=excl), above_expect(scores, 0.25, excl), "flat")
    assert g.count_above_reps(reps, np.nextafter(np.float32(0.25), np.float32(1)), exclude=excl).tolist() == [0, 0, 0, 0]


def test_a_row_over_the_top_k_cap(monkeypatch):
    """One row returns 3 000 items in score order, another 1 025: no top-k call can return either (k <= 1 024)."""
    items, d = 4000, 16
    E, bias = _random_params(items, d, 21)
    reps = (np.random.RandomState(22).randn(3, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps)
    s = -np.sort(-scores, axis=1)
    t = np.array([s[0, 2999], s[1, 1024], s[2, 9]], np.float32)
    for groups in (None, 2):
        _force(monkeypatch, groups)
        got = g.recommend_above_reps(reps, t)
        _same(got, above_expect(scores, t), f"over the cap, groups={groups}")
        assert got.counts.tolist() == [3000, 1025, 10] and got.counts[0] > RECOMMEND_MAX_K
        assert np.all(np.diff(got.row(0)[1]) <= 0)
    with pytest.raises(EngineError):
        g.recommend_reps(reps, 1025)


# ------------------------------------------------------------------------------------------------
# against the other calls
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 1024])
def test_first_k_entries_are_the_top_k_rows(k):
    """With t[u] = the k-th score of recommend_reps(k), the first k entries of row u in score order are that call's row, bit for bit
    (the set is an upper set of the one total order); with exclusion lists as well."""
    items, users, d = 3000, 130, 16
    E, bias = _random_params(items, d, 70)
    rs = np.random.RandomState(71)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    excl = [rs.randint(0, items, u % 40).astype(np.uint32) for u in range(users)]
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    for ex in (None, excl):
        top_i, top_s = g.recommend_reps(reps, k, exclude=ex)
        got = g.recommend_above_reps(reps, top_s[:, k - 1].copy(), exclude=ex)
        assert np.all(got.counts >= k)
        for u in range(users):
            ids, sc = got.row(u)
            assert np.array_equal(ids[:k], top_i[u]) and np.array_equal(_bits(sc[:k]), _bits(top_s[u])), u


def test_count_is_the_rank_of_rank_targets():
    """Nothing masked: with t[u] = score_candidates of a target, count_above_reps is rank_targets_reps' rank of that target."""
    items, users, d = 1500, 70, 32
    E, bias = _random_params(items, d, 31)
    rs = np.random.RandomState(32)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    tptr = np.arange(users + 1, dtype=np.uint64)
    targets = rs.randint(0, items, users).astype(np.uint32)
    t = np.concatenate(g.score_candidates_reps(reps, tptr, targets)).astype(np.float32)
    ranks = g.rank_targets_reps(reps, tptr, targets)
    assert np.array_equal(g.count_above_reps(reps, t), ranks.astype(np.uint64)) and ranks.min() >= 1


@pytest.mark.parametrize("groups", [1, None])
def test_tag_filter(monkeypatch, groups):
    """Tag masks of every kind side by side — none, any_of, none_of, a mask that passes 1 % and one that passes nothing — alone and
    with lists: equal to the numpy statement, and to the unfiltered call with the equivalent exclusion lists.  Zero masks equal the
    plain call."""
    _force(monkeypatch, groups)
    g, tags, reps, excl, scores = _filter_case()
    users = len(reps)
    t = np.quantile(scores, 0.7, axis=1).astype(np.float32)
    t[::7] = -np.inf
    any_of = np.zeros(users, np.uint32)
    none_of = np.zeros(users, np.uint32)
    kind = np.arange(users) % 5
    any_of[kind == 1] = 0b1010
    none_of[kind == 2] = 0b0110
    any_of[kind == 3] = 1 << 20
    any_of[kind == 4] = 1 << 30  # no item carries bit 30
    allow = np.array([allowed(tags, a, n) for a, n in zip(masks_of(any_of, users), masks_of(none_of, users))])
    for own in (None, excl):
        got = _both_orders(lambda order: g.recommend_above_reps(reps, t, exclude=own, any_of=any_of, none_of=none_of, order=order),
                           lambda: g.count_above_reps(reps, t, exclude=own, any_of=any_of, none_of=none_of), scores, t, own, allow, what="masks")
        assert np.all(got.counts[kind == 4] == 0)
        equiv = equivalent_exclusions(tags, any_of, none_of, users, own)
        _same(got, _triple(g.recommend_above_reps(reps, t, exclude=equiv, order="id")), "masks as exclusion lists")
    _same(g.recommend_above_reps(reps, t, exclude=excl, any_of=0, none_of=0), _triple(g.recommend_above_reps(reps, t, exclude=excl)), "zero masks")


# ------------------------------------------------------------------------------------------------
# the audience orientation
# ------------------------------------------------------------------------------------------------
def test_audience_is_the_transposed_question(monkeypatch):
    """audience_above_reps(reps, items, t) holds exactly the transposed pairs of recommend_above_reps(reps, t) restricted to the
    query items, scores bit-equal, for a scalar t; per-query thresholds and exclusion lists against the numpy statement; repeated
    queries; forced to 1 range and to 3."""
    items, rows, d = 700, 300, 32
    E, bias = _random_params(items, d, 41)
    rs = np.random.RandomState(42)
    reps = (rs.randn(rows, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps)
    q = np.concatenate([rs.permutation(items)[:150], [5, 5]]).astype(np.uint32)
    t = np.float32(np.quantile(scores, 0.9))
    fwd = g.recommend_above_reps(reps, t, order="id")
    keep = np.isin(fwd.ids, q[:150])
    want = sorted((int(r), int(i), int(b)) for i, r, b in transposed(fwd.ptr, fwd.ids, fwd.scores, rows) if i in set(q[:150].tolist()))
    for groups in (1, 3):
        _force(monkeypatch, groups)
        rev = g.audience_above_reps(reps, q[:150], t, order="id")
        rr, ri, rsc = rev.pairs()
        assert sorted(zip(ri.tolist(), q[:150][rr].tolist(), _bits(rsc).tolist())) == want and len(want) == int(np.count_nonzero(keep))
        tq = np.quantile(scores.T[q], 0.5 + 0.4 * rs.rand(len(q)), axis=1).diagonal().astype(np.float32)
        tq[3], tq[4] = -np.inf, np.inf
        qex = [rs.randint(0, rows, j % 9).astype(np.uint32) for j in range(len(q))]
        tq[151], qex[151] = tq[150], qex[150]  # the repeated query: the same row twice
        sq = np.ascontiguousarray(scores.T[q])
        got = _both_orders(lambda order: g.audience_above_reps(reps, q, tq, exclude=qex, order=order),
                           lambda: g.count_audience_above_reps(reps, q, tq, exclude=qex), sq, tq, qex, what=f"audience groups={groups}")
        assert got.counts[3] == rows - len(np.unique(qex[3])) and got.counts[4] == 0
        assert np.array_equal(got.row(150)[0], got.row(151)[0])


def test_audience_from_histories():
    """audience_above on histories: user_representations, then the reps form with the users whose history holds the query item left
    out — or not, with include_history."""
    E, bias, params, ptr, it, hists, scores = _core_case(ModelKind.LSTM_NORMAL, 16)
    g = _model(CORE_ITEMS, CORE_T, 16, ModelKind.LSTM_NORMAL, E, bias)
    for w, v in params.items():
        g.set_param(w, v)
    first = [int(h[0]) for h in hists if len(h)][:3]
    q = np.array(first + [999, first[0]], np.uint32)
    sq = np.ascontiguousarray(scores.T[q])
    t = np.quantile(sq, 0.5, axis=1).astype(np.float32)
    holders = [[u for u in range(CORE_USERS) if qi in hists[u]] for qi in q]
    assert sum(len(h) for h in holders) > 0
    _both_orders(lambda order: g.audience_above(ptr, it, q, t, order=order), lambda: g.count_audience_above(ptr, it, q, t), sq, t, holders, what="masked")
    _both_orders(lambda order: g.audience_above(ptr, it, q, t, include_history=True, order=order),
                 lambda: g.count_audience_above(ptr, it, q, t, include_history=True), sq, t, what="include_history")


# ------------------------------------------------------------------------------------------------
# sessions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(ModelKind.LSTM_NORMAL, 32), (ModelKind.EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_sessions(kind, d):
    """A store with remember = 8.  recommend_above equals the reps form with exclude = seen + the caller's lists, include_seen leaves
    the memory out.  audience_above with slots=None (every live slot) and with named slots, one of them empty (it reads the
    empty-history row), equals audience_above_reps on the candidates' representations with the host-built "has seen q" lists."""
    items, n = 500, 40
    rs = np.random.RandomState(50 + d)
    E, bias = _random_params(items, d, 60 + d)
    g = _model(items, 8, d, kind, E, bias)
    st = g.sessions(3 * n, remember=8)
    slots = rs.permutation(3 * n)[:n].astype(np.uint32)
    st.append(slots, [rs.randint(0, items, i % 13).astype(np.uint32) for i in range(n)])
    reps = st.representations(slots)
    seen = st.seen(slots)
    assert max(len(s) for s in seen) == 8 and min(len(s) for s in seen) == 0
    own = [rs.randint(0, items, rs.randint(0, 30)).astype(np.uint32) for _ in range(n)]
    both = [np.concatenate([a, b]).astype(np.uint32) for a, b in zip(seen, own)]
    scores = _rep_scores(_oracle_of(g), items, reps)
    t = np.quantile(scores, 0.8, axis=1).astype(np.float32)
    t[::5] = -np.inf
    _both_orders(lambda order: st.recommend_above(slots, t, exclude=own, order=order), lambda: st.count_above(slots, t, exclude=own), scores, t, both,
                 what="seen + lists")
    _same(st.recommend_above(slots, t, exclude=own), _triple(g.recommend_above_reps(reps, t, exclude=both)), "reps form")
    _both_orders(lambda order: st.recommend_above(slots, t, order=order), lambda: st.count_above(slots, t), scores, t, seen, what="seen only")
    _both_orders(lambda order: st.recommend_above(slots, t, exclude=own, include_seen=True, order=order),
                 lambda: st.count_above(slots, t, exclude=own, include_seen=True), scores, t, own, what="include_seen")
    # the reverse question
    q = np.concatenate([rs.permutation(items)[:25], max(seen[: n // 2], key=len)[:3]]).astype(np.uint32)
    live = np.sort(slots[st.lengths(slots) > 0])
    empty = np.setdiff1d(np.arange(3 * n), slots)[:1].astype(np.uint32)
    named = np.concatenate([slots[: n // 2], empty]).astype(np.uint32)
    for cand, arg in ((live, None), (np.sort(named), named)):
        creps = st.representations(cand)
        cseen = st.seen(cand)
        sq = np.ascontiguousarray(_rep_scores(_oracle_of(g), items, creps).T[q])
        tq = np.quantile(sq, 0.6, axis=1).astype(np.float32)
        tq[0] = -np.inf
        has_seen = [[j for j in range(len(cand)) if qi in cseen[j]] for qi in q]
        assert sum(len(h) for h in has_seen) >= 3
        qex_slots = [rs.choice(3 * n, j % 6, replace=False).astype(np.uint32) for j in range(len(q))]  # slot ids; no candidates among them are ignored
        qex_pos = [[int(np.searchsorted(cand, s)) for s in ex if s in cand] for ex in qex_slots]
        union = [sorted(set(a) | set(b)) for a, b in zip(has_seen, qex_pos)]
        got = _both_orders(lambda order: st.audience_above(q, tq, slots=arg, exclude=qex_slots, order=order),
                           lambda: st.count_audience_above(q, tq, slots=arg, exclude=qex_slots), sq, tq, union, ids=cand, what="store audience")
        by_rows = g.audience_above_reps(creps, q, tq, exclude=union, order="id")  # `got` is the id-order result
        _same(got, (by_rows.ptr, cand[by_rows.ids], by_rows.scores), "audience_above_reps on the candidates")
        _both_orders(lambda order: st.audience_above(q, tq, slots=arg, include_seen=True, order=order),
                     lambda: st.count_audience_above(q, tq, slots=arg, include_seen=True), sq, tq, None, ids=cand, what="include_seen")
    st.close()


# ------------------------------------------------------------------------------------------------
# the host paths
# ------------------------------------------------------------------------------------------------
def test_two_host_chunks_and_three_fill_ranges(monkeypatch):
    """8 192 + 200 rows x 64 items are two chunks; SBR_ABOVE_FILL_BYTES small enough cuts a chunk's fill into several row ranges (three
    and more).  Both give the one-shot result, which equals the numpy statement."""
    users, items, d = 8192 + 200, 64, 16
    E, bias = _random_params(items, d, 80)
    reps = (np.random.RandomState(81).randn(users, d) * 0.5).astype(np.float32)
    excl = [np.array([u % items, (7 * u) % items], np.uint32) for u in range(users)]
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps[:300])
    t = np.float32(0.3)
    whole = g.recommend_above_reps(reps, t, exclude=excl, order="id")
    cut = 5000
    a = g.recommend_above_reps(reps[:cut], t, exclude=excl[:cut], order="id")
    b = g.recommend_above_reps(reps[cut:], t, exclude=excl[cut:], order="id")
    _same(whole, (np.concatenate([a.ptr, b.ptr[1:] + a.ptr[-1]]), np.concatenate([a.ids, b.ids]), np.concatenate([a.scores, b.scores])), "two chunks")
    head = g.recommend_above_reps(reps[:300], t, exclude=excl[:300], order="id")
    _same(head, above_expect(scores, t, excl[:300], order="id"), "numpy")
    assert np.array_equal(whole.ptr[:301], head.ptr) and np.array_equal(g.count_above_reps(reps, t, exclude=excl), whole.counts)
    total = int(head.ptr[-1])
    assert total > 1000
    for pieces in (3, 7):
        monkeypatch.setenv(FILL_HOOK, str(8 * (total // pieces + int(head.counts.max()))))
        _same(g.recommend_above_reps(reps[:300], t, exclude=excl[:300], order="id"), _triple(head), f"fill in >= {pieces} ranges")
    monkeypatch.setenv(FILL_HOOK, "1")  # one row per fill range
    _same(g.recommend_above_reps(reps[:40], t, exclude=excl[:40], order="id"),
          (head.ptr[:41], head.ids[: int(head.ptr[40])], head.scores[: int(head.ptr[40])]), "one row per range")
    monkeypatch.delenv(FILL_HOOK)
    q = np.arange(items, dtype=np.uint32)
    rev = g.audience_above_reps(reps, q, t, order="id")
    fwd = g.recommend_above_reps(reps, t, order="id")
    rr, ri, rsc = rev.pairs()
    order = np.lexsort((rr, ri))
    assert np.array_equal(ri[order], fwd.pairs()[0]) and np.array_equal(rr[order], fwd.ids) and np.array_equal(_bits(rsc[order]), _bits(fwd.scores))


# ------------------------------------------------------------------------------------------------
# capacity and errors
# ------------------------------------------------------------------------------------------------
SENTINEL_U32, SENTINEL_F32 = 0xABCDEF01, np.float32(-123.5)


def _raw_reps_call(g, reps, thresholds, capacity, want_scores=True):
    """sbr_recommend_above_reps through ctypes with sentinel-filled outputs -> (status, counts, total, ids, scores)"""
    L = _lib.load()
    reps = np.ascontiguousarray(reps, np.float32)
    th = np.ascontiguousarray(thresholds, np.float32)
    n = reps.shape[0]
    counts = np.full(n, 0xFFFFFFFFFFFFFFFF, np.uint64)
    total = C.c_uint64(0xFFFFFFFFFFFFFFFF)
    ids = np.full(max(capacity, 1) + 8, SENTINEL_U32, np.uint32)
    scores = np.full(max(capacity, 1) + 8, SENTINEL_F32, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = L.sbr_recommend_above_reps(g._h, p(reps), n, p(th), None, None, None, None, p(counts), C.byref(total), capacity, p(ids),
                                    p(scores) if want_scores else None)
    return st, counts, total.value, ids, scores


def test_capacity_and_errors():
    """A capacity below the total leaves the sentinel-filled buffers untouched and still returns the counts, the total and SBR_OK;
    an exact capacity fills exactly that many entries; the Python layer raises a ValueError that names the total.  A NaN threshold
    is an argument error that writes nothing; an inf in one item's embedding fails with PredictionError, as recommend does."""
    items, d, users = 300, 16, 10
    E, bias = _random_params(items, d, 90)
    reps = np.abs(np.random.RandomState(91).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps)
    t = np.quantile(scores, 0.9, axis=1).astype(np.float32)
    want = above_expect(scores, t, order="id")
    total = int(want[0][-1])
    assert total >= 10 * users // 2
    st, counts, tot, ids, sc = _raw_reps_call(g, reps, t, total - 1)
    assert st == Status.OK and tot == total and np.array_equal(counts, np.diff(want[0])) and np.all(ids == SENTINEL_U32) and np.all(sc == SENTINEL_F32)
    st, counts, tot, ids, sc = _raw_reps_call(g, reps, t, 0)
    assert st == Status.OK and tot == total and np.all(ids == SENTINEL_U32)
    st, counts, tot, ids, sc = _raw_reps_call(g, reps, t, total)
    assert st == Status.OK and tot == total and np.array_equal(ids[:total], want[1]) and np.array_equal(_bits(sc[:total]), _bits(want[2]))
    assert np.all(ids[total:] == SENTINEL_U32) and np.all(sc[total:] == SENTINEL_F32)
    st, counts, tot, ids, sc = _raw_reps_call(g, reps, t, total + 5, want_scores=False)
    assert st == Status.OK and np.array_equal(ids[:total], want[1]) and np.all(sc == SENTINEL_F32)
    with pytest.raises(ValueError, match=str(total)):
        g.recommend_above_reps(reps, t, max_results=total - 1)
    assert int(g.recommend_above_reps(reps, t, max_results=total).ptr[-1]) == total
    # a NaN threshold: refused by the library before any launch, and by the Python layer
    bad = t.copy()
    bad[4] = np.nan
    st, counts, tot, ids, sc = _raw_reps_call(g, reps, bad, total)
    assert st == Status.INVALID_ARGUMENT and tot == 0xFFFFFFFFFFFFFFFF and np.all(counts == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(ids == SENTINEL_U32)
    with pytest.raises(ValueError):
        g.recommend_above_reps(reps, bad)
    with pytest.raises(ValueError):
        g.recommend_above_reps(reps, t, order="rank")
    with pytest.raises(EngineError) as e:  # masks on a model without tags, as recommend
        g.recommend_above_reps(reps, t, any_of=1)
    assert e.value.status == Status.INVALID_ARGUMENT
    empty = g.recommend_above_reps(reps[:0], 0.0)
    assert len(empty) == 0 and empty.ids.size == 0 and g.count_above_reps(reps[:0], 0.0).size == 0
    # the non-finite rule
    En = E.copy()
    En[200, 3] = np.inf
    g.set_param(Param.ITEM_EMBEDDING, En)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_reps(reps, 5)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_above_reps(reps, t)
    with pytest.raises(PredictionError.InvalidPredictionValue):  # also when the item is excluded or far below the bar: a scanned pair
        g.count_above_reps(reps, np.inf, exclude=[[200]] * users)
    st, counts, tot, ids, sc = _raw_reps_call(g, reps, t, total)
    assert st == Status.INVALID_PREDICTION and np.all(ids == SENTINEL_U32) and np.all(sc == SENTINEL_F32)
    g.set_param(Param.ITEM_EMBEDDING, E)
    _same(g.recommend_above_reps(reps, t, order="id"), want, "after the errors")


def test_launch_count():
    """The RANK family of the timing ledger: the count form is two launches (scan, offsets), the full call three (the fill)."""
    items, d, users = 300, 16, 10
    E, bias = _random_params(items, d, 95)
    reps = (np.random.RandomState(96).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    g.timing_enable(True)
    g.timing_read()  # the read resets the ledger
    g.count_above_reps(reps, 0.0)
    assert int(g.timing_read()["RANK"][1]) == 2
    g.recommend_above_reps(reps, 0.0)
    assert int(g.timing_read()["RANK"][1]) == 3
    g.timing_enable(False)
