"""GPU: recommend_sampled — topk_gemm_kernel's GumbelBias policy in sbr_catalogue.hip behind sbr_recommend_sampled /
sbr_recommend_sampled_reps / sbr_sessions_recommend_sampled.  The noise is a counter-keyed function of (seed, stream, item) built
from correctly rounded operations, so tests/sampled_expect.py states it a second time in numpy and everything here is BIT equality
of items, keys and plain scores with that expectation (over the oracle's or designed exact scores), or of the device with itself:
no tolerance anywhere.  The kernel's two pruning bounds may never change a result; the designed cases put them where they prune
everything (T small), nothing (T large, flat scores) and something.  The number of item ranges is forced with
SBR_CATALOGUE_GROUPS as in tests/test_catalogue_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from filter_expect import equivalent_exclusions
from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM
from sampled_expect import noise, sampled_expect
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ModelKind, Param, SbrSampleArgs, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, PredictionError

pytestmark = pytest.mark.gpu

HOOK = "SBR_CATALOGUE_GROUPS"


def _force(monkeypatch, groups):
    if groups is None:
        monkeypatch.delenv(HOOK, raising=False)
    else:
        monkeypatch.setenv(HOOK, str(groups))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    """items, plain scores and keys, bit for bit"""
    assert len(got) == 3 and len(want) == 3
    gi, wi = got[0], want[0]
    assert gi.shape == wi.shape, (what, gi.shape, wi.shape)
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: {len(bad)} items differ; first at {bad[0]}: {gi[tuple(bad[0])]} vs {wi[tuple(bad[0])]}"
    for name, g, w in (("score", got[1], want[1]), ("key", got[2], want[2])):
        bad = np.argwhere(_bits(g) != _bits(w))
        assert bad.size == 0, f"{what}: {len(bad)} {name} bits differ; first at {bad[0]}: {g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r}"


def _cut(want, k):
    return tuple(w[:, :k] for w in want)


def _csr(hists):
    ptr = np.zeros(len(hists) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(h) for h in hists])
    it = np.concatenate([np.asarray(h, np.uint32) for h in hists] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return ptr, it


def _model(items, T, d, kind, E, bias, tags=None):
    g = Model(hparams(items, T, d, int(kind), LOSS_HINGE, B=8))
    g.set_param(Param.ITEM_EMBEDDING, E)
    g.set_param(Param.ITEM_BIAS, bias)
    if tags is not None:
        g.set_item_tags(tags)
    return g


def _oracle_of(g):
    o = OracleModel(g.hp)
    for which in (Param.ITEM_EMBEDDING, Param.ITEM_BIAS, Param.LSTM_W, Param.LSTM_B, Param.EWMA_ALPHA):
        if g.param_count(which):
            o.set_param(which, g.get_param(which))
    return o


def _rep_scores(o, items, reps):
    all_items = np.arange(items, dtype=np.uint32)
    return np.array([o.predict(r, all_items) for r in np.asarray(reps, np.float32)], np.float32).reshape(len(reps), items)


def _random_params(items, d, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(items, d) * 0.3).astype(np.float32), (rs.randn(items) * 0.5).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# core: histories through the recurrent forward, against the oracle's scores
# ------------------------------------------------------------------------------------------------
CORE_ITEMS, CORE_USERS, CORE_T = 1000, 130, 8
CORE_KS, CORE_TEMPS, CORE_SEED = (1, 10, 100), (0.5, 1.0, 4.0), 20261019


@functools.lru_cache(maxsize=None)
def _core_case(kind, d):
    """Parameters, histories and — computed once, read-only — the oracle's scores and the rows' noise."""
    E, bias = _random_params(CORE_ITEMS, d, 7 * d + int(kind))
    ptr, it = synthetic_interactions(CORE_USERS, CORE_ITEMS, 2 * CORE_T, seed=d, min_len=0)
    hists = [np.asarray(it[int(ptr[u]): int(ptr[u + 1])], np.uint32) for u in range(CORE_USERS)]
    g = _model(CORE_ITEMS, CORE_T, d, kind, E, bias)
    o = _oracle_of(g)
    params = {w: g.get_param(w) for w in (Param.LSTM_W, Param.LSTM_B, Param.EWMA_ALPHA) if g.param_count(w)}
    g.close()
    scores = _rep_scores(o, CORE_ITEMS, [o.user_representation(h) for h in hists])
    scores.setflags(write=False)
    return E, bias, params, ptr, it, hists, scores


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA], ids=lambda k: k.name)
def test_core_against_the_oracle(monkeypatch, kind, d, groups):
    """1 000 items (32 tiles, the last one ragged) x 130 users (the second user tile nearly empty), k = 1, 10, 100, T = 0.5, 1, 4,
    history excluded and included, forced to 1 range and to 3."""
    _force(monkeypatch, groups)
    E, bias, params, ptr, it, hists, scores = _core_case(kind, d)
    g = _model(CORE_ITEMS, CORE_T, d, kind, E, bias)
    for w, v in params.items():
        g.set_param(w, v)
    uniq = [np.unique(h) for h in hists]
    for temp in CORE_TEMPS:
        for include in (False, True):
            want = sampled_expect(scores, None if include else uniq, max(CORE_KS), temp, CORE_SEED)
            for k in CORE_KS:
                got = g.recommend_sampled(ptr, it, k, temperature=temp, seed=CORE_SEED, include_history=include)
                _same(got, _cut(want, k), f"T={temp} include={include} k={k}")


@pytest.mark.parametrize("d", [16, 32, 64, 128, 256])
def test_every_storage_width(d):
    """Every width the kernel is instantiated at, 200 items x 40 users, k = 10."""
    items, users, k = 200, 40, 10
    E, bias = _random_params(items, d, d)
    reps = (np.random.RandomState(d + 1).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps)
    _same(g.recommend_sampled_reps(reps, k, temperature=1.0, seed=d), sampled_expect(scores, None, k, 1.0, d), f"d={d}")


# ------------------------------------------------------------------------------------------------
# designed exact scores: staging overflow and re-offer, and the pruning bounds at their extremes
# ------------------------------------------------------------------------------------------------
DES_ITEMS, DES_USERS, S = 4096, 70, 2.0 ** -10


@functools.lru_cache(maxsize=None)
def _rising_case():
    """d = 16, reps[u] = (x_u, 0, ...), E[i] = (i, 0, ...), b = 0: the score x_u * i is exact in f32 and rises with the id (x > 0):
    with keys that follow the scores every tile beats the threshold, the worst case for staging and merging.  Every fourth user
    falls instead."""
    u = np.arange(DES_USERS)
    x = np.where(u % 4 == 3, -1.0, 1.0) * (1 + u % 3) * S
    ids = np.arange(DES_ITEMS, dtype=np.float64)
    scores = 0.0 + x[:, None] * ids[None, :]
    assert np.array_equal(scores.astype(np.float32).astype(np.float64), scores)
    scores = scores.astype(np.float32)
    scores.setflags(write=False)
    E = np.zeros((DES_ITEMS, 16), np.float32)
    E[:, 0] = ids
    reps = np.zeros((DES_USERS, 16), np.float32)
    reps[:, 0] = x
    return E, reps, scores


@pytest.mark.parametrize("temp", [0.05, 1.0, 50.0])
def test_rising_scores_one_range(monkeypatch, temp):
    """4 096 items in one forced range (128 tiles per workgroup), k = 5 and 64.  T = 0.05: the keys follow the scores (steps of
    0.02 .. 0.06 against noise of a few units: long rising runs), so staging buffers overflow and candidates are offered again.
    T = 1: score steps of 1e-3, the first bound prunes most items and the second some.  T = 50: the keys are noise, neither bound
    prunes until the list's threshold is high."""
    _force(monkeypatch, 1)
    E, reps, scores = _rising_case()
    g = _model(DES_ITEMS, 8, 16, ModelKind.EWMA, E, np.zeros(DES_ITEMS, np.float32))
    want = sampled_expect(scores, None, 64, temp, seed=3)
    if temp == 0.05:  # the keys follow the scores: a step is 0.0195 per item for user 0 and the noise spans less than 19.5, so
        assert np.all(want[0][0] > DES_ITEMS - 64 - 1000)  # nothing further than 1 000 items below the 64th can be drawn
    for k in (5, 64):
        _same(g.recommend_sampled_reps(reps, k, temperature=temp, seed=3), _cut(want, k), f"T={temp} k={k}")


@pytest.mark.parametrize("groups", [1, None])
def test_flat_scores_are_pure_noise(monkeypatch, groups):
    """All scores equal (0.25): the order is the noise's alone, k = 100 of 4 096 items; identical keys would go to the lower id."""
    _force(monkeypatch, groups)
    users = 40
    g = _model(DES_ITEMS, 8, 16, ModelKind.EWMA, np.zeros((DES_ITEMS, 16), np.float32), np.full(DES_ITEMS, 0.25, np.float32))
    reps = np.zeros((users, 16), np.float32)
    reps[:, 0] = 1.0
    scores = np.full((users, DES_ITEMS), 0.25, np.float32)
    want = sampled_expect(scores, None, 100, 1.0, seed=8)
    got = g.recommend_sampled_reps(reps, 100, temperature=1.0, seed=8)
    _same(got, want, "flat")
    assert np.all(got[1] == np.float32(0.25)) and len({tuple(r) for r in got[0].tolist()}) == users


def test_tie_to_the_exact_path():
    """Score gaps of 0.05 at T = 1e-3: gap / T = 50 exceeds the noise's whole range (19.5), so the draw is recommend's row: the same
    items, and plain scores with recommend's bits."""
    items, users, k = 1500, 50, 40
    rs = np.random.RandomState(5)
    order = rs.permutation(items)
    bias = (order * 0.05).astype(np.float32)
    E = np.zeros((items, 16), np.float32)
    E[:, 0] = order * 0.05
    reps = np.zeros((users, 16), np.float32)
    reps[::2, 0] = 1.0  # even users: gaps of 0.1 (bias + E), odd users: the bias alone
    g = _model(items, 8, 16, ModelKind.EWMA, E, bias)
    plain = g.recommend_reps(reps, k)
    assert np.all(np.diff(plain[1].astype(np.float64), axis=1) < -0.049)
    got = g.recommend_sampled_reps(reps, k, temperature=1e-3, seed=11)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(_bits(got[1]), _bits(plain[1]))
    assert np.all(np.diff(got[2], axis=1) <= 0)


# ------------------------------------------------------------------------------------------------
# eligibility: exclusion lists, tag masks, sessions with seen-item memory
# ------------------------------------------------------------------------------------------------
def _filter_case(seed=40):
    items, d, users = 2000, 32, 60
    rs = np.random.RandomState(seed)
    E, bias = _random_params(items, d, seed)
    tags = (np.uint32(1) << rs.randint(0, 8, items).astype(np.uint32)).astype(np.uint32)
    tags[rs.choice(items, items // 100, replace=False)] |= np.uint32(1 << 20)  # the mask that passes 1 %
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    excl = [rs.randint(0, items, rs.randint(0, 50)).astype(np.uint32) for _ in range(users)]
    excl[3] = np.arange(0, items, 2, dtype=np.uint32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias, tags)
    return g, tags, reps, excl, _rep_scores(_oracle_of(g), items, reps)


@pytest.mark.parametrize("groups", [1, None])
def test_exclusion_lists_and_tag_masks(monkeypatch, groups):
    """Exclusion lists (the _reps form); tag masks of every kind side by side — none, any_of, none_of, a mask that passes 1 % of the
    catalogue (fewer than k: a short row) and one that passes nothing (a row of padding) — alone and with the lists.  An item
    that is not eligible draws no slot and changes no other item's noise: the expectation is the unfiltered keys with the
    ineligible items struck out."""
    _force(monkeypatch, groups)
    g, tags, reps, excl, scores = _filter_case()
    users, k, temp, seed = len(reps), 30, 0.8, 77
    _same(g.recommend_sampled_reps(reps, k, temperature=temp, seed=seed, exclude=excl), sampled_expect(scores, excl, k, temp, seed), "lists")
    any_of = np.zeros(users, np.uint32)
    none_of = np.zeros(users, np.uint32)
    kind = np.arange(users) % 5
    any_of[kind == 1] = 0b1010
    none_of[kind == 2] = 0b0110
    any_of[kind == 3] = 1 << 20
    any_of[kind == 4] = 1 << 30  # no item carries bit 30
    for own in (None, excl):
        equiv = equivalent_exclusions(tags, any_of, none_of, users, own)
        want = sampled_expect(scores, equiv, k, temp, seed)
        assert np.all(want[0][4] == NO_ITEM) and 0 < np.count_nonzero(want[0][3] != NO_ITEM) < k
        got = g.recommend_sampled_reps(reps, k, temperature=temp, seed=seed, exclude=own, any_of=any_of, none_of=none_of)
        _same(got, want, "masks numpy")
        assert np.all(np.isneginf(got[1][4])) and np.all(np.isneginf(got[2][4]))
        _same(got, g.recommend_sampled_reps(reps, k, temperature=temp, seed=seed, exclude=equiv), "masks as exclusion lists")


@pytest.mark.parametrize("kind,d", [(ModelKind.LSTM_NORMAL, 32), (ModelKind.EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_sessions_recommend_sampled(kind, d):
    """A store with remember = 8: store.recommend_sampled(slots, ...) equals recommend_sampled_reps on the slots' representations
    with exclude = seen + the caller's lists and streams = the slot ids (the store's default); include_seen leaves the memory out;
    explicit streams are taken; a slot's row does not depend on who else is in the call."""
    items, n, k, temp, seed = 500, 40, 20, 1.5, 99
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
    got = st.recommend_sampled(slots, k, temperature=temp, seed=seed, exclude=own)
    _same(got, g.recommend_sampled_reps(reps, k, temperature=temp, seed=seed, streams=slots, exclude=both), "reps form")
    _same(got, sampled_expect(scores, both, k, temp, seed, streams=slots), "numpy")
    _same(st.recommend_sampled(slots, k, temperature=temp, seed=seed), sampled_expect(scores, seen, k, temp, seed, streams=slots), "seen only")
    _same(st.recommend_sampled(slots, k, temperature=temp, seed=seed, exclude=own, include_seen=True),
          sampled_expect(scores, own, k, temp, seed, streams=slots), "include_seen")
    other = (slots.astype(np.uint64) << np.uint64(33)) + np.uint64(5)
    _same(st.recommend_sampled(slots, k, temperature=temp, seed=seed, streams=other), sampled_expect(scores, seen, k, temp, seed, streams=other),
          "explicit streams")
    alone = st.recommend_sampled(slots[7:8], k, temperature=temp, seed=seed, exclude=own[7:8])
    _same(alone, tuple(x[7:8] for x in got), "a slot alone")
    st.close()


# ------------------------------------------------------------------------------------------------
# invariances, device against device
# ------------------------------------------------------------------------------------------------
def test_invariances(monkeypatch):
    """130 users x 3 000 items, d = 16: rows asked for alone with their streams passed explicitly; k = 5 is the prefix of k = 50;
    1, 2 and 5 item ranges; the same (seed, streams) twice; another seed."""
    items, users, d = 3000, 130, 16
    E, bias = _random_params(items, d, 70)
    reps = (np.random.RandomState(71).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    call = lambda r=reps, k=50, seed=5, **kw: g.recommend_sampled_reps(r, k, temperature=0.7, seed=seed, **kw)  # noqa: E731
    _force(monkeypatch, None)
    base = call()
    _same(call(), base, "the same call twice")
    rows = np.array([0, 1, 64, 127, 128, 129])
    _same(call(reps[rows], streams=rows), tuple(x[rows] for x in base), "rows alone, streams explicit")
    for r in (3, 129):
        _same(call(reps[r:r + 1], streams=[r]), tuple(x[r:r + 1] for x in base), f"row {r} alone")
    assert np.any(call(reps[3:4])[0] != base[0][3:4])  # its default stream alone is 0, another draw
    _same(call(k=5), _cut(base, 5), "k = 5 is a prefix of k = 50")
    for groups in (1, 2, 5):
        _force(monkeypatch, groups)
        _same(call(), base, f"{groups} ranges")
    _force(monkeypatch, None)
    other = call(seed=6)
    assert np.all(np.any(other[0] != base[0], axis=1))  # every row is another draw
    # the streams are 64 bits wide
    hi = call(reps[:4], streams=np.arange(4, dtype=np.uint64) + (np.uint64(1) << np.uint64(40)))
    assert np.all(np.any(hi[0] != base[0][:4], axis=1))


def test_two_host_chunks_equal_the_unsplit_calls():
    """8 192 + 200 users at k = 10 are two launches (recommend_users_cap): the call equals its two halves asked for separately with
    their streams passed explicitly, so a row's noise does not depend on its chunk or its position in it.  300 items, d = 16."""
    users, items, d, k = 8192 + 200, 300, 16, 10
    E, bias = _random_params(items, d, 80)
    reps = (np.random.RandomState(81).randn(users, d) * 0.5).astype(np.float32)
    excl = [np.array([u % items, (7 * u) % items], np.uint32) for u in range(users)]
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    whole = g.recommend_sampled_reps(reps, k, temperature=2.0, seed=9, exclude=excl)
    cut = 5000
    a = g.recommend_sampled_reps(reps[:cut], k, temperature=2.0, seed=9, exclude=excl[:cut], streams=np.arange(cut))
    b = g.recommend_sampled_reps(reps[cut:], k, temperature=2.0, seed=9, exclude=excl[cut:], streams=np.arange(cut, users))
    _same(whole, tuple(np.concatenate([x, y]) for x, y in zip(a, b)), "two chunks")
    tail = np.arange(8192, users)
    scores = _rep_scores(_oracle_of(g), items, reps[tail])
    _same(tuple(x[tail] for x in whole), sampled_expect(scores, [excl[u] for u in tail], k, 2.0, 9, streams=tail), "second chunk numpy")


# ------------------------------------------------------------------------------------------------
# errors
# ------------------------------------------------------------------------------------------------
SENTINEL_U32, SENTINEL_F32 = 0xABCDEF01, np.float32(-123.5)


def _raw_reps_call(g, reps, k, temperature, seed=0, any_of=None):
    """sbr_recommend_sampled_reps through ctypes with sentinel-filled outputs -> (status, items, scores, keys)"""
    L = _lib.load()
    reps = np.ascontiguousarray(reps, np.float32)
    n = reps.shape[0]
    items = np.full((n, max(k, 1)), SENTINEL_U32, np.uint32)
    scores = np.full((n, max(k, 1)), SENTINEL_F32, np.float32)
    keys = np.full((n, max(k, 1)), SENTINEL_F32, np.float32)
    sa = SbrSampleArgs()
    sa.temperature, sa.seed, sa.streams = temperature, seed, None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = L.sbr_recommend_sampled_reps(g._h, p(reps), n, k, None, None, C.byref(sa), p(any_of), None, p(items), p(scores), p(keys))
    return st, items, scores, keys


def _untouched(out):
    _, items, scores, keys = out
    return np.all(items == SENTINEL_U32) and np.all(scores == SENTINEL_F32) and np.all(keys == SENTINEL_F32)


def test_errors_leave_outputs_and_model_untouched():
    """Temperature 0, negative, NaN, inf and 1e-39 (its reciprocal is not finite in f32); k = 0 and 1 025; streams of the wrong
    length; masks on a model without tags; the non-finite rule — an item bias of 3e38 at T = 0.5 (the key overflows while the
    score is finite) and a NaN embedding row.  Each is the error recommend raises for its counterpart, writes nothing, and leaves
    the model as it was."""
    items, d, users, k = 300, 16, 10, 5
    E, bias = _random_params(items, d, 90)
    reps = np.abs(np.random.RandomState(91).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    before = g.recommend_sampled_reps(reps, k, temperature=0.5, seed=1)
    plain_before = g.recommend_reps(reps, k)

    def refused(call):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT

    for temp in (0.0, -1.0, float("nan"), float("inf"), 1e-39):
        refused(lambda: g.recommend_sampled_reps(reps, k, temperature=temp))
        out = _raw_reps_call(g, reps, k, temp)
        assert out[0] == Status.INVALID_ARGUMENT and _untouched(out), temp
    ptr, it = synthetic_interactions(users, items, 8, seed=1, min_len=1)
    refused(lambda: g.recommend_sampled(ptr, it, k, temperature=0.0))
    assert np.isfinite(np.float32(1.0) / np.float32(3e38)) and g.recommend_sampled_reps(reps, k, temperature=3e38)[0].shape == (users, k)
    for bad_k in (0, 1025):
        refused(lambda: g.recommend_sampled_reps(reps, bad_k))
        refused(lambda: g.recommend_reps(reps, bad_k))  # the counterpart
        out = _raw_reps_call(g, reps, bad_k, 1.0)
        assert out[0] == Status.INVALID_ARGUMENT and _untouched(out), bad_k
    assert g.recommend_sampled_reps(reps, 1024)[0].shape == (users, 1024)
    with pytest.raises(ValueError):
        g.recommend_sampled_reps(reps, k, streams=np.arange(users + 1))
    with pytest.raises(ValueError):
        g.recommend_sampled(ptr, it, k, streams=np.arange(users - 1))
    refused(lambda: g.recommend_sampled_reps(reps, k, any_of=1))
    refused(lambda: g.recommend_reps(reps, k, any_of=1))  # the counterpart
    out = _raw_reps_call(g, reps, k, 1.0, any_of=np.ones(users, np.uint32))
    assert out[0] == Status.INVALID_ARGUMENT and _untouched(out)
    st = g.sessions(4)
    st.append([0, 1], [[1, 2], [3]])
    refused(lambda: st.recommend_sampled([0, 1], k, temperature=-2.0))
    refused(lambda: st.recommend_sampled([0, 1], k, none_of=1))
    with pytest.raises(ValueError):
        st.recommend_sampled([0, 1], k, include_seen=True)  # a store without memory, as Sessions.recommend
    with pytest.raises(ValueError):
        st.recommend_sampled([0, 1], k, streams=[1])
    st.close()
    _same(g.recommend_sampled_reps(reps, k, temperature=0.5, seed=1), before, "after the argument errors")
    # the non-finite rule: a key that overflows although every score is finite
    big = bias.copy()
    big[123] = 3e38
    g.set_param(Param.ITEM_BIAS, big)
    assert np.all(np.isfinite(g.recommend_reps(reps, k)[1]))
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_sampled_reps(reps, k, temperature=0.5)
    with pytest.raises(PredictionError.InvalidPredictionValue):  # also when the item is excluded: it is a scanned pair
        g.recommend_sampled_reps(reps, k, temperature=0.5, exclude=[[123]] * users)
    out = _raw_reps_call(g, reps, k, 0.5)
    assert out[0] == Status.INVALID_PREDICTION and _untouched(out)
    assert g.recommend_sampled_reps(reps, k, temperature=2.0)[0].shape == (users, k)  # 1.5e38 is a key like any other
    g.set_param(Param.ITEM_BIAS, bias)
    # a NaN embedding row fails recommend and recommend_sampled alike
    En = E.copy()
    En[200] = np.nan
    g.set_param(Param.ITEM_EMBEDDING, En)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_reps(reps, k)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_sampled_reps(reps, k, temperature=0.5)
    out = _raw_reps_call(g, reps, k, 1.0)
    assert out[0] == Status.INVALID_PREDICTION and _untouched(out)
    assert np.array_equal(_bits(g.get_param(Param.ITEM_BIAS)), _bits(bias))
    g.set_param(Param.ITEM_EMBEDDING, E)
    _same(g.recommend_sampled_reps(reps, k, temperature=0.5, seed=1), before, "after the prediction errors")
    after = g.recommend_reps(reps, k)
    assert np.array_equal(after[0], plain_before[0]) and np.array_equal(_bits(after[1]), _bits(plain_before[1]))


def test_launch_count():
    """The RANK family of the timing ledger counts six launches for one chunk: keys, scan, merge, pairs, scores, padding."""
    items, d, users = 300, 16, 10
    E, bias = _random_params(items, d, 95)
    reps = (np.random.RandomState(96).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    g.timing_enable(True)
    g.timing_read()  # the read resets the ledger
    g.recommend_sampled_reps(reps, 5)
    assert int(g.timing_read()["RANK"][1]) == 6
    g.timing_enable(False)
