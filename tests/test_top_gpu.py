"""GPU: the budget form of the scans — select_gemm_kernel (8 rounds of a radix select on the score bits) with select_step_kernel
between them, then above_gemm_kernel's count and fill at the cuts and top_trim_kernel, behind sbr_recommend_top / _reps /
sbr_sessions_recommend_top and sbr_audience_top / _reps / sbr_sessions_audience_top.  The result is exact, so tests/top_expect.py
states the contract a second time in numpy and everything here is equality: ids and counts as integers, scores and cuts by their
f32 bits, against that expectation (over the oracle's or designed exact scores) or of the device with itself.  Shapes, cases and
helpers are those of tests/test_above_gpu.py; the number of item ranges is forced with SBR_CATALOGUE_GROUPS as there."""
import ctypes as C

import numpy as np
import pytest

from filter_expect import allowed, equivalent_exclusions, masks_of
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import RECOMMEND_MAX_K
from sbr_rs_amd.errors import EngineError, PredictionError
from test_sampled_gpu import CORE_ITEMS, CORE_T, CORE_USERS, _bits, _core_case, _filter_case, _force, _model, _oracle_of, _random_params, _rep_scores
from top_expect import top_expect

pytestmark = pytest.mark.gpu

FILL_HOOK = "SBR_ABOVE_FILL_BYTES"
NO_ITEM = 0xFFFFFFFF


def _same(got, want, what=""):
    """an Above of a *_top call against (ptr, ids, scores, cuts): pointers and ids as integers, scores and cuts bit for bit"""
    ptr, ids, scores, cuts = want
    assert got.ptr.dtype == np.uint64 and got.ids.dtype == np.uint32 and got.scores.dtype == np.float32 and got.cuts.dtype == np.float32
    assert np.array_equal(got.ptr, ptr), f"{what}: counts differ; first at row {np.argwhere(np.diff(got.ptr) != np.diff(ptr))[:1]}"
    bad = np.argwhere(_bits(got.cuts) != _bits(cuts))
    assert bad.size == 0, f"{what}: {len(bad)} cuts differ; first at row {bad[0]}: {got.cuts[bad[0][0]]!r} vs {cuts[bad[0][0]]!r}"
    bad = np.argwhere(got.ids != ids)
    assert bad.size == 0, f"{what}: {len(bad)} ids differ; first at entry {bad[0]}: {got.ids[bad[0][0]]} vs {ids[bad[0][0]]}"
    bad = np.argwhere(_bits(got.scores) != _bits(scores))
    assert bad.size == 0, f"{what}: {len(bad)} score bits differ; first at entry {bad[0]}: {got.scores[bad[0][0]]!r} vs {scores[bad[0][0]]!r}"


def _quad(a):
    return a.ptr, a.ids, a.scores, a.cuts


def _both_orders(call, nth, scores, n, excluded=None, allow=None, ids=None, what=""):
    """call(order=...) in both orders against the expectation, and nth() — the select alone — against its cuts and counts"""
    for order in ("score", "id"):
        got = call(order=order)
        want = top_expect(scores, n, excluded, allow, order, ids)
        _same(got, want, f"{what} order={order}")
    cuts, counts = nth()
    assert cuts.dtype == np.float32 and counts.dtype == np.uint64
    assert np.array_equal(_bits(cuts), _bits(want[3])) and np.array_equal(counts, np.diff(want[0])), what
    return got


def _mixed_budgets(rows, items, seed):
    """a budget per row that differs by row: zeros, ones, a few, past the top-k calls' 1 024 where the catalogue allows, the whole
    catalogue and past it"""
    rs = np.random.RandomState(seed)
    pool = [0, 1, 2, 7, 33, 100, min(1025, items - 1), items - 1, items, items + 5]
    n = np.array([pool[i % len(pool)] for i in range(rows)], np.uint64)
    n[rs.permutation(rows)[: rows // 4]] = rs.randint(1, items, rows // 4)
    return n


# ------------------------------------------------------------------------------------------------
# against the expectation through the oracle's scores
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA], ids=lambda k: k.name)
def test_core_against_the_oracle(monkeypatch, kind, d, groups):
    """1 000 items (32 tiles, the last one ragged) x 130 users (the second row tile nearly empty): n = 1, 7, items + 5 and a budget
    per row with zeros among them, history excluded and included, forced to 1 range and to 3."""
    _force(monkeypatch, groups)
    E, bias, params, ptr, it, hists, scores = _core_case(kind, d)
    g = _model(CORE_ITEMS, CORE_T, d, kind, E, bias)
    for w, v in params.items():
        g.set_param(w, v)
    uniq = [np.unique(h) for h in hists]
    per_row = _mixed_budgets(CORE_USERS, CORE_ITEMS, d)
    assert (per_row == 0).any() and (per_row > CORE_ITEMS).any()
    for include in (False, True):
        for n in (1, 7, CORE_ITEMS + 5, per_row):
            _both_orders(lambda order: g.recommend_top(ptr, it, n, include_history=include, order=order),
                         lambda: g.nth_score(ptr, it, n, include_history=include), scores, n, None if include else uniq,
                         what=f"include={include} n={n if np.ndim(n) == 0 else 'per row'}")


@pytest.mark.parametrize("d", [32, 128])
def test_past_the_top_k_cap_against_the_oracle(d):
    """3 000 items x 70 rows: n = 1 500 for every row — no top-k call can return it (k <= 1 024) — and a budget per row, with
    exclusion lists; both orientations."""
    items, users = 3000, 70
    E, bias = _random_params(items, d, 21 + d)
    rs = np.random.RandomState(22 + d)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    excl = [rs.randint(0, items, u % 40).astype(np.uint32) for u in range(users)]
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps)
    for n in (1500, _mixed_budgets(users, items, d)):
        got = _both_orders(lambda order: g.recommend_top_reps(reps, n, exclude=excl, order=order), lambda: g.nth_score_reps(reps, n, exclude=excl),
                           scores, n, excl, what=f"d={d}")
    assert got.counts.max() > RECOMMEND_MAX_K
    with pytest.raises(EngineError):
        g.recommend_reps(reps, 1500)
    q = rs.permutation(items)[:40].astype(np.uint32)
    qex = [rs.randint(0, users, j % 5).astype(np.uint32) for j in range(len(q))]
    nq = _mixed_budgets(len(q), users, d + 1)
    sq = np.ascontiguousarray(scores.T[q])
    _both_orders(lambda order: g.audience_top_reps(reps, q, nq, exclude=qex, order=order), lambda: g.nth_audience_score_reps(reps, q, nq, exclude=qex),
                 sq, nq, qex, what=f"d={d} audience")


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
    n = _mixed_budgets(users, items, d)
    _both_orders(lambda order: g.recommend_top_reps(reps, n, exclude=excl, order=order), lambda: g.nth_score_reps(reps, n, exclude=excl),
                 scores, n, excl, what=f"d={d} lists")
    q = rs.permutation(items)[:30].astype(np.uint32)
    qex = [rs.randint(0, users, j % 5).astype(np.uint32) for j in range(len(q))]
    nq = _mixed_budgets(len(q), users, d)
    _both_orders(lambda order: g.audience_top_reps(reps, q, nq, exclude=qex, order=order), lambda: g.nth_audience_score_reps(reps, q, nq, exclude=qex),
                 np.ascontiguousarray(scores.T[q]), nq, qex, what=f"d={d} audience")


# ------------------------------------------------------------------------------------------------
# identities with the other calls
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10, 1024])
def test_identities_with_recommend_and_above(n):
    """recommend_top_reps(n) is recommend_reps(k = n) without padding, and the first n of recommend_above_reps(cuts) in score order;
    count_above_reps(cuts) >= n and count_above_reps(nextafter(cuts, +inf)) < n; order="id" is the same set, ascending.  With
    exclusion lists as well; one row excludes all but 5 items, so its row is short and its cut -inf."""
    items, users, d = 3000, 130, 16
    E, bias = _random_params(items, d, 70)
    rs = np.random.RandomState(71)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    excl = [rs.randint(0, items, u % 40).astype(np.uint32) for u in range(users)]
    excl[9] = np.arange(5, items, dtype=np.uint32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    for ex in (None, excl):
        top_i, top_s = g.recommend_reps(reps, n, exclude=ex)
        got = g.recommend_top_reps(reps, n, exclude=ex)
        by_id = g.recommend_top_reps(reps, n, exclude=ex, order="id")
        over = g.recommend_above_reps(reps, got.cuts, exclude=ex)
        at_cut = g.count_above_reps(reps, got.cuts, exclude=ex)
        past_cut = g.count_above_reps(reps, np.nextafter(got.cuts, np.float32(np.inf)), exclude=ex)
        assert np.array_equal(got.ptr, by_id.ptr) and np.array_equal(_bits(got.cuts), _bits(by_id.cuts))
        for u in range(users):
            ids, sc = got.row(u)
            m = int(np.count_nonzero(top_i[u] != NO_ITEM))
            assert len(ids) == m and np.array_equal(ids, top_i[u, :m]) and np.array_equal(_bits(sc), _bits(top_s[u, :m])), u
            assert np.array_equal(ids, over.row(u)[0][:m]) and np.array_equal(_bits(sc), _bits(over.row(u)[1][:m])), u
            a = np.argsort(ids, kind="stable")
            assert np.array_equal(by_id.row(u)[0], ids[a]) and np.array_equal(_bits(by_id.row(u)[1]), _bits(sc[a])), u
            if m == n:
                assert got.cuts[u] == sc[-1] and at_cut[u] >= n and past_cut[u] < n, u
            else:
                assert got.cuts[u] == -np.inf and at_cut[u] == m, u
        assert np.all(np.delete(got.counts, 9) == n) and got.counts[9] == (n if ex is None else min(n, 5))


# ------------------------------------------------------------------------------------------------
# designed exact scores
# ------------------------------------------------------------------------------------------------
DES_ITEMS = 1100  # 35 tiles, the last one ragged


def _designed(bias, users=4):
    """d = 16, reps[u] = -1e-30 throughout, E[i] = 0: the chain of an item ends at +0.0 and its score is bias[i] + 0.0 = bias[i], bit
    for bit.  Only a -0.0 bias would lose its sign that way, so such an item's row is 1e-30 throughout instead: every product
    underflows to -0.0, the chain ends at -0.0 and the score is -0.0 (tests/test_above_gpu.py's construction).  The oracle says so
    below; the scores of every user are `bias`."""
    b = np.asarray(bias, np.float32).copy()
    assert b.shape == (DES_ITEMS,) and np.all(np.isfinite(b))
    E = np.zeros((DES_ITEMS, 16), np.float32)
    E[(b == 0) & np.signbit(b)] = 1e-30
    reps = np.full((users, 16), -1e-30, np.float32)
    g = _model(DES_ITEMS, 8, 16, ModelKind.EWMA, E, b)
    assert np.array_equal(_bits(_rep_scores(_oracle_of(g), DES_ITEMS, reps[:1])[0]), _bits(b)), "the designed scores are the oracle's, signed zeros included"
    return g, reps, np.tile(b, (users, 1))


@pytest.mark.parametrize("groups", [1, 4])
def test_a_tie_group_straddles_the_cut(monkeypatch, groups):
    """300 distinct positive scores, 400 zeros of both signs and 400 negative scores, shuffled over the ids: with n = 450 the cut is
    zero (written +0.0), exactly 450 come back and the 150 zeros kept are the 150 lowest ids of the group, whatever their sign; n
    at the group's edges (300, 301, 700, 701), 1, 0, everything and more; with an exclusion list that takes some of the group."""
    _force(monkeypatch, groups)
    rs = np.random.RandomState(5)
    b = np.empty(DES_ITEMS, np.float32)
    where = rs.permutation(DES_ITEMS)
    pos, zero, neg = where[:300], np.sort(where[300:700]), where[700:]
    b[pos] = np.arange(1, 301, dtype=np.float32) * 0.5
    b[zero] = np.where(np.arange(400) % 3 == 0, np.float32(-0.0), np.float32(0.0))
    b[neg] = -np.arange(1, 401, dtype=np.float32) * 0.25
    n = np.array([450, 300, 301, 700, 701, 1, 0, DES_ITEMS, DES_ITEMS + 1, 450], np.uint64)
    excl = [[] for _ in n]
    excl[9] = np.concatenate([zero[:50], pos[:10], zero[:5]])  # 50 of the group's lowest ids and 10 better items are gone
    g, reps, scores = _designed(b, users=len(n))
    got = _both_orders(lambda order: g.recommend_top_reps(reps, n, exclude=excl, order=order), lambda: g.nth_score_reps(reps, n, exclude=excl),
                       scores, n, excl, what="tie group")
    assert got.counts.tolist() == [450, 300, 301, 700, 701, 1, 0, DES_ITEMS, DES_ITEMS, 450]
    ids, sc = g.recommend_top_reps(reps, n, exclude=excl).row(0)  # score order: the zeros come last, by id
    assert np.array_equal(ids[300:], zero[:150]) and np.all(sc[300:] == 0) and np.signbit(sc[300:]).any() and not np.signbit(sc[300:]).all()
    assert np.array_equal(_bits(sc[300:]), _bits(b[zero[:150]])) and np.array_equal(_bits(got.cuts[[0, 2, 3]]), _bits(np.zeros(3, np.float32)))
    assert got.cuts[1] == 0.5 and got.cuts[4] == -0.25 and got.cuts[5] == 150.0 and got.cuts[6] == np.inf
    assert got.cuts[7] == -100.0 and got.cuts[8] == -np.inf
    ids9 = g.recommend_top_reps(reps, n, exclude=excl).row(9)[0]
    assert np.array_equal(ids9[290:], zero[50:210]) and not np.isin(excl[9], ids9).any()


def test_all_scores_equal():
    """All scores 0.25: any n returns the n lowest eligible ids, and the cut is 0.25 until n passes the eligible count."""
    g, reps, scores = _designed(np.full(DES_ITEMS, 0.25, np.float32), users=6)
    n = np.array([0, 1, 500, DES_ITEMS, 2000, 300], np.uint64)
    excl = [[], [0, 1, 2], [7, 7, 7, 1099, 0, 1099], [], list(range(0, DES_ITEMS, 2)), list(range(0, DES_ITEMS, 2))]
    got = _both_orders(lambda order: g.recommend_top_reps(reps, n, exclude=excl, order=order), lambda: g.nth_score_reps(reps, n, exclude=excl),
                       scores, n, excl, what="flat")
    assert got.counts.tolist() == [0, 1, 500, DES_ITEMS, DES_ITEMS // 2, 300]
    assert got.row(1)[0].tolist() == [3] and got.row(2)[0][:3].tolist() == [1, 2, 3] and got.row(5)[0].tolist() == list(range(1, 601, 2))
    assert got.cuts.tolist() == [np.inf, 0.25, 0.25, 0.25, -np.inf, 0.25]


@pytest.mark.parametrize("groups", [1, 4])
def test_scores_across_signs_and_exponents(monkeypatch, groups):
    """Scores of both signs whose exponents run from the denormals to 2^127, with random mantissas, a block that differs only in
    its last mantissa bits, and both zeros: every round's digit decides something.  Every n from a coarse grid, the row's maximum
    (n = 1) and its minimum (n = all)."""
    _force(monkeypatch, groups)
    rs = np.random.RandomState(9)
    exps = rs.randint(1, 255, DES_ITEMS).astype(np.uint32)
    exps[:60] = 0  # denormals
    mant = rs.randint(0, 1 << 23, DES_ITEMS).astype(np.uint32)
    sign = rs.randint(0, 2, DES_ITEMS).astype(np.uint32)
    bits = (sign << 31) | (exps << 23) | mant
    bits[100:164] = np.float32(1.5).view(np.uint32) + np.arange(64, dtype=np.uint32)  # neighbours in the last six bits
    bits[200:264] = np.float32(-1.5).view(np.uint32) + rs.permutation(64).astype(np.uint32)
    bits[300], bits[301] = 0x80000000, 0
    b = bits.view(np.float32).copy()
    assert np.all(np.isfinite(b)) and np.unique(bits >> 28).size == 16
    n = np.concatenate([[1, DES_ITEMS], np.arange(2, DES_ITEMS, 37)]).astype(np.uint64)
    g, reps, scores = _designed(b, users=len(n))
    got = _both_orders(lambda order: g.recommend_top_reps(reps, n, order=order), lambda: g.nth_score_reps(reps, n), scores, n, what="exponents")
    assert got.cuts[0] == b.max() and got.cuts[1] == b.min() and np.array_equal(got.counts, n)
    in_block = np.isin(_bits(got.cuts), bits[100:164])
    assert in_block.any(), "a cut among the 64 neighbours: only the last two rounds tell them apart"


# ------------------------------------------------------------------------------------------------
# everything the siblings mask
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, None])
def test_tag_filter(monkeypatch, groups):
    """Tag masks of every kind side by side — none, any_of, none_of, a mask that passes 1 % and one that passes nothing — alone and
    with lists: equal to the numpy statement over the allowed columns, and to the unfiltered call with the equivalent exclusion
    lists.  Zero masks equal the plain call."""
    _force(monkeypatch, groups)
    g, tags, reps, excl, scores = _filter_case()
    users, items = len(reps), scores.shape[1]
    n = _mixed_budgets(users, items, 3)
    any_of = np.zeros(users, np.uint32)
    none_of = np.zeros(users, np.uint32)
    kind = np.arange(users) % 5
    any_of[kind == 1] = 0b1010
    none_of[kind == 2] = 0b0110
    any_of[kind == 3] = 1 << 20
    any_of[kind == 4] = 1 << 30  # no item carries bit 30
    n[kind == 3] = 15  # about 20 items carry bit 20: some rows full, the rows with lists maybe short
    allow = np.array([allowed(tags, a, b) for a, b in zip(masks_of(any_of, users), masks_of(none_of, users))])
    for own in (None, excl):
        got = _both_orders(lambda order: g.recommend_top_reps(reps, n, exclude=own, any_of=any_of, none_of=none_of, order=order),
                           lambda: g.nth_score_reps(reps, n, exclude=own, any_of=any_of, none_of=none_of), scores, n, own, allow, what="masks")
        assert np.all(got.counts[kind == 4] == 0) and np.all(got.cuts[(kind == 4) & (n > 0)] == -np.inf)
        equiv = equivalent_exclusions(tags, any_of, none_of, users, own)
        _same(got, _quad(g.recommend_top_reps(reps, n, exclude=equiv, order="id")), "masks as exclusion lists")
    _same(g.recommend_top_reps(reps, n, exclude=excl, any_of=0, none_of=0), _quad(g.recommend_top_reps(reps, n, exclude=excl)), "zero masks")


@pytest.mark.parametrize("groups", [None, 3])
def test_every_mask_kind_of_the_filtered_suite(monkeypatch, groups):
    """The designed case of tests/test_filtered_gpu.py — 5 007 items whose tags use bits 0 and 31, scores exact and tied in threes,
    130 users cycling through its seven mask kinds: no filter, any_of only, none_of with bit 31, any_of with bit 31 AND a none_of on
    the same row, an any_of bit no item has, none_of = 0xFFFFFFFF (the tag-0 items), any_of = one bit with none_of = every other bit
    (20-odd items) — alone and with its exclusion lists: equal to the numpy statement over the allowed columns and to the unfiltered
    call with the equivalent exclusion lists.  Budgets straddle the short rows' eligible counts."""
    import test_filtered_gpu as tf

    _force(monkeypatch, groups)
    E, reps, tags, any_of, none_of, excl, _ = tf._designed_case()
    users, items = tf.DES_USERS, tf.DES_ITEMS
    scores = (0.0 + reps[:, :1].astype(np.float64) * E[:, 0].astype(np.float64)[None, :]).astype(np.float32)
    assert np.array_equal(scores.astype(np.float64), 0.0 + reps[:, :1].astype(np.float64) * E[:, 0].astype(np.float64)[None, :])
    kind = np.arange(users) % 7
    high = np.uint32(1 << 31)
    assert (tags & high).any() and np.all(none_of[kind == 2] & high) and np.all(any_of[kind == 3] & high) and np.all(none_of[kind == 3] != 0)
    assert np.all(none_of[kind == 5] == tf.ALL) and np.all((any_of[kind == 6] ^ none_of[kind == 6]) == tf.ALL)
    allow = np.array([allowed(tags, a, b) for a, b in zip(masks_of(any_of, users), masks_of(none_of, users))])
    blind = np.array([allowed(tags, a, b) for a, b in zip(masks_of(any_of & ~high, users), masks_of(none_of & ~high, users))])
    assert np.all((allow != blind)[(kind == 2) | (kind == 3)].any(axis=1)), "bit 31 decides columns of every such row"
    tag0, few = int(np.count_nonzero(tags == 0)), int(np.count_nonzero(tags == (1 << tf.FEW_BIT)))
    n = _mixed_budgets(users, items, 11)
    n[kind == 5] = np.resize([tag0 - 1, tag0, 50, 2000, tag0 + 1], np.count_nonzero(kind == 5))
    n[kind == 6] = np.resize([10, few, few + 3, 1, few - 1], np.count_nonzero(kind == 6))
    n[kind == 4] = np.resize([0, 1, 100], np.count_nonzero(kind == 4))
    g = _model(items, 8, 16, ModelKind.EWMA, E, np.zeros(items, np.float32), tags)
    for own in (None, excl):
        got = _both_orders(lambda order: g.recommend_top_reps(reps, n, exclude=own, any_of=any_of, none_of=none_of, order=order),
                           lambda: g.nth_score_reps(reps, n, exclude=own, any_of=any_of, none_of=none_of), scores, n, own, allow,
                           what=f"mask kinds, lists={own is not None}")
        assert np.all(got.counts[kind == 4] == 0) and np.all(got.counts[kind == 6] <= few) and np.all(got.counts[kind == 5] <= tag0)
        if own is None:
            assert np.array_equal(got.counts[kind == 6], np.minimum(n[kind == 6], few)) and np.array_equal(got.counts[kind == 5], np.minimum(n[kind == 5], tag0))
            assert np.all(got.cuts[(kind == 6) & (n > few)] == -np.inf) and np.all(np.isfinite(got.cuts[(kind == 6) & (n <= few)]))
        equiv = equivalent_exclusions(tags, any_of, none_of, users, own)
        _same(got, _quad(g.recommend_top_reps(reps, n, exclude=equiv, order="id")), "mask kinds as exclusion lists")


def test_audience_from_histories():
    """audience_top on histories: user_representations, then the reps form with the users whose history holds the query item left
    out — or not, with include_history."""
    E, bias, params, ptr, it, hists, scores = _core_case(ModelKind.LSTM_NORMAL, 16)
    g = _model(CORE_ITEMS, CORE_T, 16, ModelKind.LSTM_NORMAL, E, bias)
    for w, v in params.items():
        g.set_param(w, v)
    first = [int(h[0]) for h in hists if len(h)][:3]
    q = np.array(first + [999, first[0]], np.uint32)
    sq = np.ascontiguousarray(scores.T[q])
    n = np.array([10, CORE_USERS, CORE_USERS - 1, 0, 50], np.uint64)
    holders = [[u for u in range(CORE_USERS) if qi in hists[u]] for qi in q]
    assert sum(len(h) for h in holders) > 0
    got = _both_orders(lambda order: g.audience_top(ptr, it, q, n, order=order), lambda: g.nth_audience_score(ptr, it, q, n), sq, n, holders, what="masked")
    assert got.cuts[1] == -np.inf  # its holder is left out: fewer than every user
    _both_orders(lambda order: g.audience_top(ptr, it, q, n, include_history=True, order=order),
                 lambda: g.nth_audience_score(ptr, it, q, n, include_history=True), sq, n, what="include_history")


@pytest.mark.parametrize("kind,d", [(ModelKind.LSTM_NORMAL, 32), (ModelKind.EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_sessions(kind, d):
    """A store with remember = 8.  recommend_top equals the reps form with exclude = seen + the caller's lists, include_seen leaves
    the memory out.  audience_top with slots=None (every live slot) and with named slots, one of them empty (it reads the
    empty-history row), equals audience_top_reps on the candidates' representations with the host-built "has seen q" lists."""
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
    want_n = _mixed_budgets(n, items, d)
    _both_orders(lambda order: st.recommend_top(slots, want_n, exclude=own, order=order), lambda: st.nth_score(slots, want_n, exclude=own), scores,
                 want_n, both, what="seen + lists")
    _same(st.recommend_top(slots, want_n, exclude=own), _quad(g.recommend_top_reps(reps, want_n, exclude=both)), "reps form")
    _both_orders(lambda order: st.recommend_top(slots, want_n, order=order), lambda: st.nth_score(slots, want_n), scores, want_n, seen, what="seen only")
    _both_orders(lambda order: st.recommend_top(slots, want_n, exclude=own, include_seen=True, order=order),
                 lambda: st.nth_score(slots, want_n, exclude=own, include_seen=True), scores, want_n, own, what="include_seen")
    # the reverse question
    q = np.concatenate([rs.permutation(items)[:25], max(seen[: n // 2], key=len)[:3]]).astype(np.uint32)
    live = np.sort(slots[st.lengths(slots) > 0])
    empty = np.setdiff1d(np.arange(3 * n), slots)[:1].astype(np.uint32)
    named = np.concatenate([slots[: n // 2], empty]).astype(np.uint32)
    for cand, arg in ((live, None), (np.sort(named), named)):
        creps = st.representations(cand)
        cseen = st.seen(cand)
        sq = np.ascontiguousarray(_rep_scores(_oracle_of(g), items, creps).T[q])
        nq = _mixed_budgets(len(q), len(cand), d + 2)
        has_seen = [[j for j in range(len(cand)) if qi in cseen[j]] for qi in q]
        assert sum(len(h) for h in has_seen) >= 3
        qex_slots = [rs.choice(3 * n, j % 6, replace=False).astype(np.uint32) for j in range(len(q))]  # slot ids; no candidates among them are ignored
        qex_pos = [[int(np.searchsorted(cand, s)) for s in ex if s in cand] for ex in qex_slots]
        union = [sorted(set(a) | set(b)) for a, b in zip(has_seen, qex_pos)]
        got = _both_orders(lambda order: st.audience_top(q, nq, slots=arg, exclude=qex_slots, order=order),
                           lambda: st.nth_audience_score(q, nq, slots=arg, exclude=qex_slots), sq, nq, union, ids=cand, what="store audience")
        by_rows = g.audience_top_reps(creps, q, nq, exclude=union, order="id")  # `got` is the id-order result
        _same(got, (by_rows.ptr, cand[by_rows.ids], by_rows.scores, by_rows.cuts), "audience_top_reps on the candidates")
        _both_orders(lambda order: st.audience_top(q, nq, slots=arg, include_seen=True, order=order),
                     lambda: st.nth_audience_score(q, nq, slots=arg, include_seen=True), sq, nq, None, ids=cand, what="include_seen")
    # a stale store refuses
    g.set_param(Param.ITEM_BIAS, g.get_param(Param.ITEM_BIAS))
    for call in (lambda: st.recommend_top(slots, 5), lambda: st.nth_score(slots, 5), lambda: st.audience_top(q, 5), lambda: st.nth_audience_score(q, 5)):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT
    st.close()


# ------------------------------------------------------------------------------------------------
# the host paths
# ------------------------------------------------------------------------------------------------
def test_two_host_chunks_and_cut_fills(monkeypatch):
    """8 192 + 200 rows x 64 items are two chunks; SBR_ABOVE_FILL_BYTES small enough cuts a chunk's fill into several row ranges,
    down to one row each.  All give the one-shot result, which equals the numpy statement; scores on a grid of 1/4, so most cuts
    fall inside a tie group and every range is trimmed."""
    users, items, d = 8192 + 200, 64, 16
    E, bias = _random_params(items, d, 80)
    E[:, 1:] = 0
    E[:, 0] = np.round(E[:, 0] * 8) / 4
    bias = (np.round(bias * 4) / 4).astype(np.float32)
    rs = np.random.RandomState(81)
    reps = np.zeros((users, d), np.float32)
    reps[:, 0] = rs.randint(-2, 3, users)
    excl = [np.array([u % items, (7 * u) % items], np.uint32) for u in range(users)]
    n = (np.arange(users) % 23).astype(np.uint64)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps[:300])
    whole = g.recommend_top_reps(reps, n, exclude=excl, order="id")
    cut = 5000
    a = g.recommend_top_reps(reps[:cut], n[:cut], exclude=excl[:cut], order="id")
    b = g.recommend_top_reps(reps[cut:], n[cut:], exclude=excl[cut:], order="id")
    _same(whole, (np.concatenate([a.ptr, b.ptr[1:] + a.ptr[-1]]), np.concatenate([a.ids, b.ids]), np.concatenate([a.scores, b.scores]),
                  np.concatenate([a.cuts, b.cuts])), "two chunks")
    head = g.recommend_top_reps(reps[:300], n[:300], exclude=excl[:300], order="id")
    _same(head, top_expect(scores, n[:300], excl[:300], order="id"), "numpy")
    assert np.array_equal(whole.ptr[:301], head.ptr) and np.array_equal(whole.counts, n)  # at least 62 of the 64 items are eligible
    tied = g.count_above_reps(reps[:300], head.cuts, exclude=excl[:300])
    assert int(np.count_nonzero(tied > head.counts)) > 100, "most rows' fills hold more than the row keeps"
    cuts, counts = g.nth_score_reps(reps, n, exclude=excl)
    assert np.array_equal(_bits(cuts), _bits(whole.cuts)) and np.array_equal(counts, whole.counts)
    total = int(tied.sum())
    for pieces in (3, 7):
        monkeypatch.setenv(FILL_HOOK, str(8 * (total // pieces + int(tied.max()))))
        _same(g.recommend_top_reps(reps[:300], n[:300], exclude=excl[:300], order="id"), _quad(head), f"fill in >= {pieces} ranges")
    monkeypatch.setenv(FILL_HOOK, "1")  # one row per fill range
    _same(g.recommend_top_reps(reps[:40], n[:40], exclude=excl[:40], order="id"),
          (head.ptr[:41], head.ids[: int(head.ptr[40])], head.scores[: int(head.ptr[40])], head.cuts[:40]), "one row per range")
    monkeypatch.delenv(FILL_HOOK)
    q = np.arange(items, dtype=np.uint32)  # 64 queries x 8 392 candidates: a row tile of queries, many candidate ranges
    nq = (np.arange(items) * 150).astype(np.uint64)
    rev = g.audience_top_reps(reps, q, nq, order="id")
    full = _rep_scores(_oracle_of(g), items, reps[np.unique(reps[:, 0], return_index=True)[1]])  # five distinct rows of scores
    by_value = {float(v): full[j] for j, v in enumerate(np.unique(reps[:, 0]))}
    sq = np.ascontiguousarray(np.stack([by_value[float(v)] for v in reps[:, 0]]).T)
    _same(rev, top_expect(sq, nq, order="id"), "audience over two chunks' worth of candidates")
    assert rev.counts.tolist() == np.minimum(nq, users).tolist() and rev.counts.max() == users


@pytest.mark.parametrize("groups", [1, 2, 5])
def test_item_ranges_and_row_tiles_give_the_same_bits(monkeypatch, groups):
    """300 rows (three row tiles) x 3 000 items in 1, 2 and 5 forced item ranges and the library's own choice: the same result."""
    items, users, d = 3000, 300, 32
    E, bias = _random_params(items, d, 85)
    rs = np.random.RandomState(86)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    excl = [rs.randint(0, items, u % 30).astype(np.uint32) for u in range(users)]
    n = _mixed_budgets(users, items, 87)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    _force(monkeypatch, None)
    want = g.recommend_top_reps(reps, n, exclude=excl, order="id")
    _force(monkeypatch, groups)
    _same(g.recommend_top_reps(reps, n, exclude=excl, order="id"), _quad(want), f"groups={groups}")
    _same(g.recommend_top_reps(reps[128:], n[128:], exclude=excl[128:], order="id"),
          (want.ptr[128:] - want.ptr[128], want.ids[int(want.ptr[128]):], want.scores[int(want.ptr[128]):], want.cuts[128:]), "rows alone")


# ------------------------------------------------------------------------------------------------
# capacity and errors
# ------------------------------------------------------------------------------------------------
SENTINEL_U32, SENTINEL_F32 = 0xABCDEF01, np.float32(-123.5)


def _raw_reps_call(g, reps, n, capacity, want_scores=True, want_ids=True):
    """sbr_recommend_top_reps through ctypes with sentinel-filled outputs -> (status, cuts, counts, total, ids, scores)"""
    L = _lib.load()
    reps = np.ascontiguousarray(reps, np.float32)
    n = np.ascontiguousarray(n, np.uint64)
    rows = reps.shape[0]
    cuts = np.full(rows, SENTINEL_F32, np.float32)
    counts = np.full(rows, 0xFFFFFFFFFFFFFFFF, np.uint64)
    total = C.c_uint64(0xFFFFFFFFFFFFFFFF)
    ids = np.full(max(capacity, 1) + 8, SENTINEL_U32, np.uint32)
    scores = np.full(max(capacity, 1) + 8, SENTINEL_F32, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = L.sbr_recommend_top_reps(g._h, p(reps), rows, p(n), None, None, None, None, p(cuts), p(counts), C.byref(total), capacity,
                                  p(ids) if want_ids else None, p(scores) if want_scores and want_ids else None)
    return st, cuts, counts, total.value, ids, scores


def test_capacity_and_errors():
    """A capacity below the total leaves the sentinel-filled buffers untouched and still returns the cuts, the counts, the total and
    SBR_OK; an exact capacity fills exactly that many entries; NULL pair outputs run the select alone; the Python layer raises a
    ValueError that names the total.  Out-of-range ids are argument errors; an inf in one item's embedding fails with
    PredictionError, as recommend does."""
    items, d, users = 300, 16, 10
    E, bias = _random_params(items, d, 90)
    reps = np.abs(np.random.RandomState(91).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps)
    n = np.array([30, 0, 1, 299, 300, 301, 7, 7, 100, 2], np.uint64)
    want = top_expect(scores, n, order="id")
    total = int(want[0][-1])
    assert total == int(np.minimum(n, items).sum())
    for cap in (total - 1, 0):
        st, cuts, counts, tot, ids, sc = _raw_reps_call(g, reps, n, cap)
        assert st == Status.OK and tot == total and np.array_equal(counts, np.diff(want[0])) and np.array_equal(_bits(cuts), _bits(want[3]))
        assert np.all(ids == SENTINEL_U32) and np.all(sc == SENTINEL_F32)
    st, cuts, counts, tot, ids, sc = _raw_reps_call(g, reps, n, 0, want_ids=False)
    assert st == Status.OK and tot == total and np.array_equal(counts, np.diff(want[0])) and np.array_equal(_bits(cuts), _bits(want[3]))
    st, cuts, counts, tot, ids, sc = _raw_reps_call(g, reps, n, total)
    assert st == Status.OK and tot == total and np.array_equal(ids[:total], want[1]) and np.array_equal(_bits(sc[:total]), _bits(want[2]))
    assert np.all(ids[total:] == SENTINEL_U32) and np.all(sc[total:] == SENTINEL_F32)
    st, cuts, counts, tot, ids, sc = _raw_reps_call(g, reps, n, total + 5, want_scores=False)
    assert st == Status.OK and np.array_equal(ids[:total], want[1]) and np.all(sc == SENTINEL_F32)
    with pytest.raises(ValueError, match=str(total)):
        g.recommend_top_reps(reps, n, max_results=total - 1)
    cuts, counts = g.nth_score_reps(reps, n)  # what the message points to: still right
    assert np.array_equal(_bits(cuts), _bits(want[3])) and np.array_equal(counts, np.diff(want[0]))
    assert int(g.recommend_top_reps(reps, n, max_results=total).ptr[-1]) == total
    with pytest.raises(ValueError):
        g.recommend_top_reps(reps, -1)
    with pytest.raises(ValueError):
        g.recommend_top_reps(reps, n, order="rank")
    for call in (lambda: g.recommend_top_reps(reps, n, any_of=1),  # masks on a model without tags, as recommend
                 lambda: g.recommend_top_reps(reps, n, exclude=[[items]] * users), lambda: g.audience_top_reps(reps, [items], 3),
                 lambda: g.audience_top_reps(reps, [1], 3, exclude=[[users]]),
                 lambda: g.recommend_top(np.array([0, 1], np.uint64), np.array([items], np.uint32), 3)):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT
    empty = g.recommend_top_reps(reps[:0], 5)
    assert len(empty) == 0 and empty.ids.size == 0 and empty.cuts.size == 0 and g.nth_score_reps(reps[:0], 5)[0].size == 0
    none = g.audience_top_reps(reps[:0], [1, 2], [3, 0])  # nobody to rank
    assert none.counts.tolist() == [0, 0] and none.cuts.tolist() == [-np.inf, np.inf]
    # the non-finite rule
    En = E.copy()
    En[200, 3] = np.inf
    g.set_param(Param.ITEM_EMBEDDING, En)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_reps(reps, 5)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_top_reps(reps, n)
    with pytest.raises(PredictionError.InvalidPredictionValue):  # also when the item is excluded: a scanned pair
        g.nth_score_reps(reps, n, exclude=[[200]] * users)
    st, cuts, counts, tot, ids, sc = _raw_reps_call(g, reps, n, total)
    assert st == Status.INVALID_PREDICTION and np.all(ids == SENTINEL_U32) and np.all(sc == SENTINEL_F32)
    g.set_param(Param.ITEM_EMBEDDING, E)
    _same(g.recommend_top_reps(reps, n, order="id"), want, "after the errors")


def test_launch_count():
    """The RANK family of the timing ledger: the select is 17 launches — 8 scans, 9 steps — whatever n, and the full call adds the
    count's two, the fill and the trim's two: at most 32 / 4 search scans, no launch between them but the step."""
    items, d, users = 300, 16, 10
    E, bias = _random_params(items, d, 95)
    reps = (np.random.RandomState(96).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    g.timing_enable(True)
    g.timing_read()  # the read resets the ledger
    g.nth_score_reps(reps, 50)
    assert int(g.timing_read()["RANK"][1]) == 17
    g.recommend_top_reps(reps, 50)
    assert int(g.timing_read()["RANK"][1]) == 17 + 2 + 1 + 2
    g.timing_enable(False)
