"""GPU: the per-user item-tag filter of the top-k scans (topk_gemm_kernel's TagFilter policy in sbr_catalogue.hip, behind the
any_of= / none_of= keywords and the sbr_*_filtered entry points).  The contract (include/sbr_hip.h, ITEM TAGS): a filtered call
returns, bit for bit, what the plain call returns with every user's exclusion list extended by the items its masks do not allow.
So every comparison is on items and score bits, against one or both of

  (a) the numpy expectation (filter_expect.py: recommend_expect.topk_expectation over exact or oracle scores), and
  (b) the existing plain call with the equivalent exclusion lists (filter_expect.equivalent_exclusions).

Shapes are the smallest that reach each path; the number of item ranges is forced with SBR_CATALOGUE_GROUPS as in
tests/test_catalogue_gpu.py, whose d = 16 small-integer construction of exact scores is used here too."""
import functools

import numpy as np
import pytest

from filter_expect import allowed, equivalent_exclusions, filtered_expect, masks_of
from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, PredictionError

pytestmark = pytest.mark.gpu

KINDS = [ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA]
HOOK = "SBR_CATALOGUE_GROUPS"
ABSENT_BIT = 17  # no item of any test carries it
ALL = 0xFFFFFFFF


def _force(monkeypatch, groups):
    if groups is None:
        monkeypatch.delenv(HOOK, raising=False)
    else:
        monkeypatch.setenv(HOOK, str(groups))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    gi, gs = got
    wi, ws = want
    assert gi.shape == wi.shape, (what, gi.shape, wi.shape)
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: {len(bad)} items differ; first at {bad[0]}: {gi[tuple(bad[0])]} vs {wi[tuple(bad[0])]}"
    bad = np.argwhere(_bits(gs) != _bits(ws))
    assert bad.size == 0, f"{what}: {len(bad)} score bits differ; first at {bad[0]}"


def _random_tags(items, seed, bits_each=4, zero_every=50):
    """About `bits_each` random bits per item out of the 31 bits other than ABSENT_BIT; bits 0 and 31 are in use; every
    `zero_every`-th item has tag 0."""
    rs = np.random.RandomState(seed)
    usable = np.array([b for b in range(32) if b != ABSENT_BIT])
    tags = np.zeros(items, np.uint64)
    for _ in range(bits_each):
        tags |= np.uint64(1) << usable[rs.randint(0, usable.size, items)].astype(np.uint64)
    tags = tags.astype(np.uint32)
    tags[::zero_every] = 0
    assert np.any(tags & 1) and np.any(tags >> 31) and not np.any(tags & (1 << ABSENT_BIT)) and np.any(tags == 0)
    return tags


def _model(items, T, d, kind, E, bias, tags=None):
    g = Model(hparams(items, T, d, int(kind), LOSS_HINGE, B=8))
    g.set_param(Param.ITEM_EMBEDDING, E)
    g.set_param(Param.ITEM_BIAS, bias)
    if tags is not None:
        g.set_item_tags(tags)
    return g


def _oracle(items, T, d, kind, E, bias):
    o = OracleModel(hparams(items, T, d, int(kind), LOSS_HINGE, B=8))
    o.set_param(Param.ITEM_EMBEDDING, E)
    o.set_param(Param.ITEM_BIAS, bias)
    return o


def _rep_scores(o, items, reps):
    all_items = np.arange(items, dtype=np.uint32)
    return np.array([o.predict(r, all_items) for r in np.asarray(reps, np.float32)], np.float32).reshape(len(reps), items)


def _csr(hists):
    ptr = np.zeros(len(hists) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(h) for h in hists])
    it = np.concatenate([np.asarray(h, np.uint32) for h in hists] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return ptr, it


# ------------------------------------------------------------------------------------------------
# designed exact scores: every kind of mask side by side, every k class, every range count
# ------------------------------------------------------------------------------------------------
DES_ITEMS, DES_USERS = 5007, 130
DES_KS = (1, 32, 33, 100, 1024)
S = 2.0 ** -10
FEW_BIT = 9  # the items whose tag is exactly this bit are the "fewer than k" user's whole catalogue


@functools.lru_cache(maxsize=None)
def _designed_case():
    """d = 16, reps[u] = (x_u, 0, ...), E[i] = (i // 3, 0, ...), b = 0: the score x_u * (i // 3) is exact in f32, ascends (x > 0:
    every tile beats the threshold, the worst case for merging) or descends in the id in steps of three tied items, so the id
    breaks ties between allowed and disallowed neighbours.  Masks cycle through seven kinds, user u has kind u % 7."""
    ids = np.arange(DES_ITEMS)
    y = (ids // 3).astype(np.float64)
    u = np.arange(DES_USERS)
    x = np.where(u % 2 == 0, 1.0, -1.0) * (1 + u % 4) * S
    scores = 0.0 + x[:, None] * y[None, :]  # the zero bias is added: -0.0 products score +0.0
    assert np.array_equal(scores.astype(np.float32).astype(np.float64), scores)
    scores = scores.astype(np.float32)
    tags = _random_tags(DES_ITEMS, 5)
    tags[7::251] = 1 << FEW_BIT  # 20 items
    only_few = int(np.count_nonzero(tags == (1 << FEW_BIT)))
    assert 1 < only_few < 32
    any_of = np.zeros(DES_USERS, np.uint32)
    none_of = np.zeros(DES_USERS, np.uint32)
    for i in range(DES_USERS):
        kind = i % 7
        if kind == 1:
            any_of[i] = 1 | (1 << (1 + i % 16))
        elif kind == 2:
            none_of[i] = (1 << 31) | (1 << (2 + i % 11))
        elif kind == 3:
            any_of[i], none_of[i] = (1 << 31) | (1 << 1) | (1 << (20 + i % 8)), 1 | (1 << 2)
        elif kind == 4:
            any_of[i] = 1 << ABSENT_BIT
        elif kind == 5:
            none_of[i] = ALL
        elif kind == 6:
            any_of[i], none_of[i] = 1 << FEW_BIT, ALL ^ (1 << FEW_BIT)
    rs = np.random.RandomState(6)
    excl = [rs.randint(0, DES_ITEMS, rs.randint(0, 40)).astype(np.uint32) for _ in range(DES_USERS)]
    best_first = lambda i: ids[::-1] if x[i] > 0 else ids  # noqa: E731
    excl[0] = best_first(0)[:2000].astype(np.uint32)      # whole staging buffers of excluded candidates under mask (0, 0)
    excl[1] = best_first(1)[:500:2].astype(np.uint32)     # exclusion and any_of interleave among the best
    excl[5] = ids[tags == 0][::2].astype(np.uint32)       # half of the none_of = ALL user's catalogue
    E = np.zeros((DES_ITEMS, 16), np.float32)
    E[:, 0] = y
    reps = np.zeros((DES_USERS, 16), np.float32)
    reps[:, 0] = x
    kmax = max(DES_KS)
    want = {False: filtered_expect(scores, tags, any_of, none_of, None, kmax), True: filtered_expect(scores, tags, any_of, none_of, excl, kmax)}
    for w in want.values():
        for a in w:
            a.setflags(write=False)
    # the rows are what the kinds promise
    wi = want[False][0]
    assert np.all(wi[4] == NO_ITEM) and np.all(wi[0] != NO_ITEM)
    assert set(wi[5][wi[5] != NO_ITEM].tolist()) == set(ids[tags == 0].tolist())
    assert np.count_nonzero(wi[6] != NO_ITEM) == only_few
    return E, reps, tags, any_of, none_of, excl, want


@pytest.mark.parametrize("with_excl", [False, True], ids=["filter", "filter+exclusions"])
@pytest.mark.parametrize("groups", [None, 1, 3, 157])
def test_designed_scores_every_mask_kind(monkeypatch, groups, with_excl):
    """5 007 items (not a multiple of 32) x 130 users (the second user tile holds two), k = 1, 32, 33, 100, 1024, the range count
    unset, 1 (157 tiles per workgroup: many staging overflows), 3 and 157 (one tile per range).  Users cycle through: no filter,
    any_of only, none_of only, both, an any_of bit no item has (a row of padding), none_of = 0xFFFFFFFF (the tag-0 items), a pair
    that leaves 20-odd items.  Again with per-user exclusion lists, so filter and exclusion act together."""
    _force(monkeypatch, groups)
    E, reps, tags, any_of, none_of, excl, want = _designed_case()
    g = _model(DES_ITEMS, 8, 16, ModelKind.EWMA, E, np.zeros(DES_ITEMS, np.float32), tags)
    own = excl if with_excl else None
    equiv = equivalent_exclusions(tags, any_of, none_of, DES_USERS, own)
    wi, ws = want[with_excl]
    for k in DES_KS:
        got = g.recommend_reps(reps, k, exclude=own, any_of=any_of, none_of=none_of)
        _same(got, (wi[:, :k], ws[:, :k]), f"k={k} numpy")
        _same(got, g.recommend_reps(reps, k, exclude=equiv), f"k={k} exclusion lists")


# ------------------------------------------------------------------------------------------------
# heavy ties: the id tie-break among the allowed items only
# ------------------------------------------------------------------------------------------------
def _tied_params(items, d, seed):
    """E rows drawn from 50 distinct rows (the r-th with weight 1 / (r + 1)) and biases from 4 values: at most 200 score
    classes, the largest of hundreds of items."""
    rs = np.random.RandomState(seed)
    rows = (rs.randn(50, d) * 0.3).astype(np.float32)
    p = 1.0 / np.arange(1, 51)
    E = np.ascontiguousarray(rows[rs.choice(50, size=items, p=p / p.sum())])
    bias = np.array([-0.5, 0.0, 0.25, 0.5], np.float32)[rs.randint(0, 4, items)]
    return E, bias


@pytest.mark.parametrize("groups", [1, None])
def test_heavy_ties_break_among_the_allowed(monkeypatch, groups):
    """2 003 items of at most 200 score classes, 70 users, d = 16, k = 10 and 100; bit 0 of the tags is a coin, so with any_of = 1
    (even users) or none_of = 1 (odd users) the score class of the k-th place holds allowed and disallowed items for nearly
    every user (asserted): the lower id among the ALLOWED ones must win."""
    _force(monkeypatch, groups)
    items, d, users = 2003, 16, 70
    E, bias = _tied_params(items, d, 9)
    rs = np.random.RandomState(10)
    tags = (_random_tags(items, 11) & ~np.uint32(1)) | rs.randint(0, 2, items).astype(np.uint32)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    any_of = np.where(np.arange(users) % 2 == 0, 1, 0).astype(np.uint32)
    none_of = np.where(np.arange(users) % 2 == 1, 1, 0).astype(np.uint32)
    scores = _rep_scores(_oracle(items, 8, d, ModelKind.EWMA, E, bias), items, reps)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias, tags)
    equiv = equivalent_exclusions(tags, any_of, none_of, users)
    for k in (10, 100):
        want = filtered_expect(scores, tags, any_of, none_of, None, k)
        mixed = 0
        for u in range(users):
            cls = scores[u] == want[1][u, k - 1]
            ok = allowed(tags, any_of[u], none_of[u])
            mixed += bool(np.any(cls & ok) and np.any(cls & ~ok))
        assert mixed >= users * 0.9, mixed
        got = g.recommend_reps(reps, k, any_of=any_of, none_of=none_of)
        _same(got, want, f"k={k} numpy")
        _same(got, g.recommend_reps(reps, k, exclude=equiv), f"k={k} exclusion lists")


# ------------------------------------------------------------------------------------------------
# every storage width
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 32, 64, 128, 256])
def test_every_storage_width(d):
    """300 items, 70 users, random parameters at each storage width (D > 128 has its own launch bound), k = 7 and 64, against the
    oracle's predict scores."""
    items, users = 300, 70
    rs = np.random.RandomState(d)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    bias = (rs.randn(items) * 0.5).astype(np.float32)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    tags = _random_tags(items, d + 1, zero_every=37)
    pool = np.array([0, 1, 1 << 31, (1 << 3) | (1 << 12), 1 << ABSENT_BIT, ALL], np.uint32)
    any_of = pool[rs.randint(0, 5, users)]
    none_of = pool[rs.randint(0, 6, users)]
    scores = _rep_scores(_oracle(items, 8, d, ModelKind.EWMA, E, bias), items, reps)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias, tags)
    equiv = equivalent_exclusions(tags, any_of, none_of, users)
    for k in (7, 64):
        got = g.recommend_reps(reps, k, any_of=any_of, none_of=none_of)
        _same(got, filtered_expect(scores, tags, any_of, none_of, None, k), f"k={k} numpy")
        _same(got, g.recommend_reps(reps, k, exclude=equiv), f"k={k} exclusion lists")


# ------------------------------------------------------------------------------------------------
# histories: the masks go with the call's user, not with its row of H
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
def test_histories_carry_their_users_masks(kind):
    """60 users over 20 distinct histories (user i has history i % 20, one of them empty), so call-users that share a history —
    and a row of H if the forward pass shares it — carry different masks.  recommend(histories) must equal recommend_reps on
    user_representations with the history as exclusions (not at all with include_history), and the numpy expectation."""
    items, d, T, users, k = 700, 32, 8, 60, 25
    rs = np.random.RandomState(int(kind) + 3)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    bias = (rs.randn(items) * 0.5).astype(np.float32)
    tags = _random_tags(items, 21)
    base = [rs.randint(0, items, i % (2 * T)).astype(np.uint32) for i in range(20)]
    hists = [base[i % 20] for i in range(users)]
    ptr, it = _csr(hists)
    any_of = (np.uint32(1) << (np.arange(users) % 29).astype(np.uint32)).astype(np.uint32)
    any_of[::5] = 0
    none_of = (np.uint32(1) << ((np.arange(users) // 3) % 31).astype(np.uint32)).astype(np.uint32)
    none_of[1::4] = 0
    g = _model(items, T, d, kind, E, bias, tags)
    o = OracleModel(g.hp)
    for which in (Param.ITEM_EMBEDDING, Param.ITEM_BIAS, Param.LSTM_W, Param.LSTM_B, Param.EWMA_ALPHA):
        if g.param_count(which):
            o.set_param(which, g.get_param(which))
    reps = g.user_representations(ptr, it)
    scores = _rep_scores(o, items, [o.user_representation(h) for h in hists])
    a, b = g.recommend(ptr, it, k, any_of=any_of, none_of=none_of), g.recommend(ptr, it, k, any_of=any_of[20:40].tolist() * 3, none_of=none_of)
    assert np.any(a[0][:20] != a[0][20:40]) and np.any(a[0] != b[0])  # one history, two masks, two rows
    for include in (False, True):
        own = None if include else hists
        got = g.recommend(ptr, it, k, include_history=include, any_of=any_of, none_of=none_of)
        _same(got, g.recommend_reps(reps, k, exclude=own, any_of=any_of, none_of=none_of), f"include={include} reps form")
        _same(got, g.recommend_reps(reps, k, exclude=equivalent_exclusions(tags, any_of, none_of, users, own)), f"include={include} exclusion lists")
        _same(got, filtered_expect(scores, tags, any_of, none_of, own, k), f"include={include} numpy")


# ------------------------------------------------------------------------------------------------
# the host's chunking over users
# ------------------------------------------------------------------------------------------------
def test_two_chunks_keep_each_users_masks():
    """8 192 + 200 users x 700 items, d = 16, k = 100: two launches.  Exact designed scores, distinct per user, and a mask pair of
    each user's own, so a mask read at the wrong chunk offset changes the last 200 rows (asserted on the expectation)."""
    users, items, k = 8192 + 200, 700, 100
    ids = np.arange(items)
    x = (np.arange(users) - users // 2) * 2.0 ** -12
    b = (ids % 5) * 0.25
    scores = b[None, :] + x[:, None] * ids[None, :].astype(np.float64)
    assert np.array_equal(scores.astype(np.float32).astype(np.float64), scores)
    scores = scores.astype(np.float32)
    tags = _random_tags(items, 31)
    u = np.arange(users)
    any_of = ((np.uint32(1) << (u % 13).astype(np.uint32)) | (np.uint32(1) << (18 + (u // 13) % 11).astype(np.uint32))).astype(np.uint32)
    none_of = (np.uint32(1) << (u % 7 + 24).astype(np.uint32)).astype(np.uint32)
    none_of[::3] = 0
    E = np.zeros((items, 16), np.float32)
    E[:, 0] = ids
    reps = np.zeros((users, 16), np.float32)
    reps[:, 0] = x
    g = _model(items, 8, 16, ModelKind.EWMA, E, b.astype(np.float32), tags)
    want = filtered_expect(scores, tags, any_of, none_of, None, k)
    shifted = filtered_expect(scores[8192:], tags, any_of[:200], none_of[:200], None, k)
    assert np.count_nonzero(np.any(shifted[0] != want[0][8192:], axis=1)) >= 190
    got = g.recommend_reps(reps, k, any_of=any_of, none_of=none_of)
    _same(got, want, "numpy")
    _same(got, g.recommend_reps(reps, k, exclude=equivalent_exclusions(tags, any_of, none_of, users)), "exclusion lists")


# ------------------------------------------------------------------------------------------------
# sessions, diverse, similar items
# ------------------------------------------------------------------------------------------------
def _random_case(items, d, users, seed, kind=ModelKind.EWMA):
    rs = np.random.RandomState(seed)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    E[rs.choice(np.arange(10, items), 12, replace=False)] = E[0]
    bias = np.round(rs.randn(items) * 0.5, 1).astype(np.float32)
    tags = _random_tags(items, seed + 1, zero_every=41)
    pool = np.array([0, 1, 1 << 31, (1 << 3) | (1 << 12) | (1 << 25), 1 << ABSENT_BIT, ALL, (1 << 6) | (1 << 7) | (1 << 8)], np.uint32)
    any_of = pool[rs.randint(0, 5, users)]
    none_of = pool[[0, 1, 2, 3, 5, 6]][rs.randint(0, 6, users)]
    any_of[0], none_of[0] = 0, 0
    any_of[1], none_of[1] = 1 << ABSENT_BIT, 0
    excl = [rs.randint(0, items, rs.randint(0, 30)).astype(np.uint32) for _ in range(users)]
    return _model(items, 8, d, kind, E, bias, tags), tags, any_of, none_of, excl, rs


@pytest.mark.parametrize("kind,d", [(ModelKind.LSTM_NORMAL, 32), (ModelKind.EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_sessions_recommend_filtered(kind, d):
    """store.recommend(slots, k, any_of=, none_of=) equals recommend_reps on store.representations(slots) with the same masks, and
    the plain session call with the equivalent exclusion lists; slots out of order in a larger store; with exclusions too.  The
    diverse form likewise."""
    items, n, k = 500, 40, 20
    g, tags, any_of, none_of, excl, rs = _random_case(items, d, n, 50 + d, kind)
    st = g.sessions(3 * n)
    slots = rs.permutation(3 * n)[:n].astype(np.uint32)
    st.append(slots, [rs.randint(0, items, i % 9).astype(np.uint32) for i in range(n)])
    reps = st.representations(slots)
    for own in (None, excl):
        got = st.recommend(slots, k, exclude=own, any_of=any_of, none_of=none_of)
        _same(got, g.recommend_reps(reps, k, exclude=own, any_of=any_of, none_of=none_of), "reps form")
        _same(got, st.recommend(slots, k, exclude=equivalent_exclusions(tags, any_of, none_of, n, own)), "exclusion lists")
        got = st.recommend_diverse(slots, 8, 32, 0.3, exclude=own, any_of=any_of, none_of=none_of)
        _same(got, g.recommend_diverse_reps(reps, 8, 32, 0.3, exclude=own, any_of=any_of, none_of=none_of), "diverse reps form")
        _same(got, st.recommend_diverse(slots, 8, 32, 0.3, exclude=equivalent_exclusions(tags, any_of, none_of, n, own)), "diverse exclusion lists")
    assert np.all(got[0][1] == NO_ITEM)
    st.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("d", [16, 128])
def test_diverse_filtered(d, metric):
    """recommend_diverse_reps / recommend_diverse with masks equal the plain calls with the equivalent exclusion lists (the pool is
    the filtered row at k = pool), and with trade_off = 1 the filtered recommend(k)."""
    items, users, T = 600, 50, 8
    g, tags, any_of, none_of, excl, rs = _random_case(items, d, users, 70 + d)
    ptr, it = synthetic_interactions(users, items, 2 * T, seed=d, min_len=0)
    hists = [it[int(ptr[u]): int(ptr[u + 1])] for u in range(users)]
    reps = g.user_representations(ptr, it)
    for k, pool, t in ((10, 10, 0.3), (10, 64, 0.3), (33, 65, 0.0), (12, 40, 1.0)):
        what = f"k={k} pool={pool} t={t}"
        for own in (None, excl):
            got = g.recommend_diverse_reps(reps, k, pool, t, metric, exclude=own, any_of=any_of, none_of=none_of)
            _same(got, g.recommend_diverse_reps(reps, k, pool, t, metric, exclude=equivalent_exclusions(tags, any_of, none_of, users, own)), what)
            if t == 1.0:
                _same(got, g.recommend_reps(reps, k, exclude=own, any_of=any_of, none_of=none_of), what + " is recommend")
        got = g.recommend_diverse(ptr, it, k, pool, t, metric, any_of=any_of, none_of=none_of)
        _same(got, g.recommend_diverse_reps(reps, k, pool, t, metric, exclude=equivalent_exclusions(tags, any_of, none_of, users, hists)), what + " histories")
        if t == 1.0:
            _same(got, g.recommend(ptr, it, k, any_of=any_of, none_of=none_of), what + " histories is recommend")


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_similar_items_filtered(metric):
    """Masks per query — "the same category": any_of = the query's own tag word — and random pairs; the query's own exclusion,
    include_self and the caller's lists are intact: everything equals the plain call with the equivalent exclusion lists."""
    items, d, k = 900, 64, 30
    g, tags, _, _, _, rs = _random_case(items, d, 2, 90)
    query = np.concatenate([rs.randint(0, items, 150), [0, 41, 41]]).astype(np.uint32)  # repeats; 0 and 41 have tag 0
    nq = query.size
    same_cat = tags[query]
    rnd_any = (np.uint32(1) << rs.randint(0, 32, nq).astype(np.uint32)).astype(np.uint32)
    rnd_none = (np.uint32(1) << rs.randint(0, 32, nq).astype(np.uint32)).astype(np.uint32)
    excl = [rs.randint(0, items, rs.randint(0, 20)).astype(np.uint32) for _ in range(nq)]
    for any_of, none_of in ((same_cat, None), (rnd_any, rnd_none), (None, 1 << 31)):
        equiv = lambda own: equivalent_exclusions(tags, any_of, none_of, nq, own)  # noqa: E731
        for include_self in (False, True):
            for own in (None, excl):
                got = g.similar_items(query, k, metric, include_self=include_self, exclude=own, any_of=any_of, none_of=none_of)
                _same(got, g.similar_items(query, k, metric, include_self=include_self, exclude=equiv(own)), f"self={include_self}")
                ok = np.array([allowed(tags, a, n) for a, n in zip(masks_of(any_of, nq), masks_of(none_of, nq))])
                for j in range(nq):
                    row = got[0][j][got[0][j] != NO_ITEM]
                    assert np.all(ok[j][row]) and (include_self or query[j] not in row)
    got = g.similar_items(query, k, metric, include_self=True, any_of=same_cat)
    assert np.all(got[0][-3:] != NO_ITEM)  # any_of == 0 (a tag-0 query) filters nothing


# ------------------------------------------------------------------------------------------------
# lifecycle and errors
# ------------------------------------------------------------------------------------------------
def test_tags_lifecycle():
    """set / get round trip; a filtered call before any tags, and after clearing them, is the argument error; fit and set_param
    leave the tags in place; a session store stays usable across set_item_tags; the unfiltered calls return the same bits
    before and after tags are set."""
    items, d, users, k = 400, 16, 30, 15
    rs = np.random.RandomState(1)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    bias = (rs.randn(items) * 0.5).astype(np.float32)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    tags = _random_tags(items, 2)

    def refused(call):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT

    refused(g.item_tags)
    refused(lambda: g.recommend_reps(reps, k, any_of=1))
    refused(lambda: g.recommend_reps(reps, k, any_of=0, none_of=0))  # a filtered call even with all-zero masks
    refused(lambda: g.similar_items([1, 2], k, none_of=1))
    st = g.sessions(8)
    st.append([3, 1], [[5, 6], [7]])
    refused(lambda: st.recommend([3, 1], k, any_of=1))
    before = (g.recommend_reps(reps, k), g.similar_items([1, 2, 3], k), st.recommend([1, 3], k))
    g.set_item_tags(tags)
    assert np.array_equal(g.item_tags(), tags)
    after = (g.recommend_reps(reps, k), g.similar_items([1, 2, 3], k), st.recommend([1, 3], k))  # the store is not stale
    for x, y in zip(before, after):
        _same(x, y, "unfiltered calls do not see the tags")
    _same(g.recommend_reps(reps, k, any_of=0, none_of=0), before[0], "all-zero masks are no filter")
    _same(st.recommend([1, 3], k, any_of=0), before[2], "all-zero masks are no filter (sessions)")
    filtered = g.recommend_reps(reps, k, none_of=1)
    assert np.any(filtered[0] != before[0][0])
    # other tags replace the first ones
    g.set_item_tags(tags ^ np.uint32(1))
    assert np.array_equal(g.item_tags(), tags ^ np.uint32(1))
    assert np.any(g.recommend_reps(reps, k, none_of=1)[0] != filtered[0])
    g.set_item_tags(tags)
    # parameters change, the tags stay
    g.set_param(Param.ITEM_BIAS, bias)
    ptr, it = synthetic_interactions(20, items, 8, seed=3, min_len=2)
    g.fit(ptr, it)
    assert np.array_equal(g.item_tags(), tags)
    got = g.recommend_reps(reps, k, none_of=1)
    _same(got, g.recommend_reps(reps, k, exclude=equivalent_exclusions(tags, None, 1, users)), "after fit")
    st.close()
    g.set_item_tags(None)
    refused(g.item_tags)
    refused(lambda: g.recommend_reps(reps, k, none_of=1))
    with pytest.raises(ValueError):
        g.set_item_tags(tags[:-1])


def test_non_finite_score_of_a_filtered_out_item_still_fails():
    """One item row is +inf and that item is filtered out for every user: the filtered call raises the prediction error exactly as
    the plain call with the equivalent exclusion lists does; with a finite row both succeed and agree."""
    items, d, users, k = 300, 16, 10, 5
    rs = np.random.RandomState(4)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    bias = np.zeros(items, np.float32)
    reps = np.abs(rs.randn(users, d) * 0.5).astype(np.float32)
    tags = _random_tags(items, 5) & ~np.uint32(1 << 4)
    tags[123] |= 1 << 4
    equiv = equivalent_exclusions(tags, None, 1 << 4, users)
    assert all(e.tolist() == [123] for e in equiv)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias, tags)
    _same(g.recommend_reps(reps, k, none_of=1 << 4), g.recommend_reps(reps, k, exclude=equiv), "finite")
    E[123] = np.inf
    g.set_param(Param.ITEM_EMBEDDING, E)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_reps(reps, k, exclude=equiv)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_reps(reps, k, none_of=1 << 4)
