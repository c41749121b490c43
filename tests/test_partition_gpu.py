"""GPU: log_partition — the k = 1 scan, partition_gemm_kernel and partition_finish_kernel of sbr_catalogue.hip behind
sbr_log_partition / sbr_log_partition_reps / sbr_sessions_log_partition.  The mass is a sum of integers, so
tests/partition_expect.py states the whole contract a second time in numpy and everything here is equality: the shift's f32 bits
and the mass as an integer, against that expectation (over the oracle's or designed exact scores) or of the device with itself.
Shapes, cases and helpers are those of tests/test_sampled_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from filter_expect import equivalent_exclusions
from helpers import synthetic_interactions
from partition_expect import frac_bits, log_z_expect, partition_expect, slate_log_prob_expect
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import softmax_weights
from sbr_rs_amd.errors import EngineError, PredictionError
from test_sampled_gpu import (CORE_ITEMS, CORE_T, CORE_TEMPS, _bits, _core_case, _filter_case, _force, _model, _oracle_of, _random_params,
                              _rep_scores)

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    """a Partition against (shift f32, mass u64): the shift's bits and the mass as an integer"""
    shift, mass = want
    assert got.shift.dtype == np.float32 and got.mass.dtype == np.uint64 and got.shift.shape == shift.shape and got.mass.shape == mass.shape
    bad = np.argwhere(_bits(got.shift) != _bits(shift))
    assert bad.size == 0, f"{what}: {len(bad)} shifts differ; first at row {bad[0]}: {got.shift[bad[0][0]]!r} vs {shift[bad[0][0]]!r}"
    bad = np.argwhere(got.mass != mass)
    assert bad.size == 0, f"{what}: {len(bad)} masses differ; first at row {bad[0]}: {got.mass[bad[0][0]]} vs {mass[bad[0][0]]}"


def _pair(p):
    return p.shift, p.mass


# ------------------------------------------------------------------------------------------------
# core: histories through the recurrent forward, against the oracle's scores
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA], ids=lambda k: k.name)
def test_core_against_the_oracle(monkeypatch, kind, d, groups):
    """1 000 items (32 tiles, the last one ragged) x 130 users (the second user tile nearly empty), T = 0.5, 1, 4, history excluded
    and included, forced to 1 range and to 3."""
    _force(monkeypatch, groups)
    E, bias, params, ptr, it, hists, scores = _core_case(kind, d)
    g = _model(CORE_ITEMS, CORE_T, d, kind, E, bias)
    for w, v in params.items():
        g.set_param(w, v)
    uniq = [np.unique(h) for h in hists]
    for temp in CORE_TEMPS:
        for include in (False, True):
            got = g.log_partition(ptr, it, temperature=temp, include_history=include)
            assert got.frac_bits == frac_bits(CORE_ITEMS) == 40
            _same(got, partition_expect(scores, None if include else uniq, temp), f"T={temp} include={include}")
            assert np.array_equal(got.log_z, log_z_expect(got.shift, got.mass, 40)) and np.all(got.mass >= np.uint64(1 << 40))


@pytest.mark.parametrize("d", [16, 32, 64, 128, 256])
def test_every_storage_width(d):
    """Every width the kernel is instantiated at, 200 items x 40 users, with exclusion lists."""
    items, users = 200, 40
    E, bias = _random_params(items, d, d)
    rs = np.random.RandomState(d + 1)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    excl = [rs.randint(0, items, u % 7).astype(np.uint32) for u in range(users)]
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    scores = _rep_scores(_oracle_of(g), items, reps)
    _same(g.log_partition_reps(reps, 1.0), partition_expect(scores, None, 1.0), f"d={d}")
    _same(g.log_partition_reps(reps, 0.7, exclude=excl), partition_expect(scores, excl, 0.7), f"d={d} lists")


# ------------------------------------------------------------------------------------------------
# designed rows
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
def test_an_excluded_item_holds_the_highest_score(monkeypatch, groups):
    """Item 700 outscores everything by 5 and is excluded for rows 1 and 2 (row 2 repeats it, unsorted, beside others): its d is
    positive against the row's shift, so the scan's clamp never added it and the finish subtracts nothing for it; rows 0 and 3 keep
    it as their arg-max."""
    _force(monkeypatch, groups)
    rs = np.random.RandomState(1)
    col = rs.randn(DES_ITEMS).astype(np.float32)
    col[700] = 9.0
    g, reps, scores = _designed(col)
    excl = [[], [700], [900, 700, 3, 700, 900, 3], [5]]
    got = g.log_partition_reps(reps, 1.0, exclude=excl)
    _same(got, partition_expect(scores, excl, 1.0), "excluded arg-max")
    assert got.shift[0] == np.float32(9.0) and got.shift[1] < np.float32(4.5) and got.shift[1] == got.shift[2]
    assert got.mass[1] > got.mass[2] >= np.uint64(1 << 40)


def test_flat_scores_count_the_allowed_items():
    """All scores 0.25: mass == n_allowed 2^F at any T; repeats in a list count once."""
    g, reps, _ = _designed(np.zeros(DES_ITEMS, np.float32), np.full(DES_ITEMS, 0.25, np.float32))
    excl = [[], [1, 2, 3], [7, 7, 7, 1099, 0, 1099], list(range(0, DES_ITEMS, 2))]
    for temp in (1.0, 3.0):
        got = g.log_partition_reps(reps, temp, exclude=excl)
        assert [int(m) >> 40 for m in got.mass] == [DES_ITEMS, DES_ITEMS - 3, DES_ITEMS - 3, DES_ITEMS // 2] and not np.any(got.mass & np.uint64((1 << 40) - 1))
        assert np.array_equal(_bits(got.shift), _bits(np.float32(0.25) * (np.float32(1) / np.float32(temp)) * np.ones(4, np.float32)))
        assert np.allclose(got.log_z, got.shift + np.log([DES_ITEMS, DES_ITEMS - 3, DES_ITEMS - 3, DES_ITEMS // 2]), rtol=0, atol=1e-12)


def test_tiny_temperature_leaves_the_argmax_alone():
    """Score gaps of 0.05 at T = 1e-3: every other item lies 50 or more below the shift, under the 2^-40 resolution (27.7), and
    below -64 from the second gap on: mass == 2^F exactly, log_z == shift."""
    order = np.random.RandomState(5).permutation(DES_ITEMS)
    g, reps, scores = _designed(order * 0.05)
    got = g.log_partition_reps(reps, 1e-3, exclude=[[], [int(np.argmax(order))], [], []])
    _same(got, partition_expect(scores, [[], [int(np.argmax(order))], [], []], 1e-3), "tiny T")
    assert np.all(got.mass == np.uint64(1 << 40)) and np.array_equal(got.log_z, got.shift.astype(np.float64))
    assert got.shift[1] < got.shift[0]


def test_rows_that_may_see_nothing():
    """Every item excluded, or masked: shift -inf, mass 0, log_z -inf; the rows beside them are not disturbed."""
    rs = np.random.RandomState(2)
    col = rs.randn(DES_ITEMS).astype(np.float32)
    g, reps, scores = _designed(col)
    g.set_item_tags(np.ones(DES_ITEMS, np.uint32))
    everything = np.arange(DES_ITEMS, dtype=np.uint32)
    got = g.log_partition_reps(reps, 1.0, exclude=[everything, [], everything[::-1], [4]])
    _same(got, partition_expect(scores, [everything, [], everything, [4]], 1.0), "all excluded")
    assert np.isneginf(got.shift[0]) and got.mass[0] == 0 and np.isneginf(got.log_z[0]) and np.isneginf(got.log_z[2]) and np.isfinite(got.log_z[1])
    masked = g.log_partition_reps(reps, 1.0, any_of=np.array([2, 1, 0, 0], np.uint32), none_of=np.array([0, 0, 1, 0], np.uint32))
    assert np.isneginf(masked.shift[[0, 2]]).all() and not masked.mass[[0, 2]].any() and np.isneginf(masked.log_z[[0, 2]]).all()
    plain = g.log_partition_reps(reps, 1.0)
    assert masked.mass[1] == plain.mass[1] == masked.mass[3] and np.isnan(masked.slate_log_prob(scores[:, :3])[0]).all()


# ------------------------------------------------------------------------------------------------
# tags
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, None])
def test_tag_masks_equal_their_exclusion_lists(monkeypatch, groups):
    """Masks of every kind side by side — none, any_of, none_of, one that passes 1 % and one that passes nothing — alone and with
    exclusion lists whose entries the masks already remove (no double subtraction): the filtered call equals the unfiltered call
    given filter_expect.equivalent_exclusions, and the numpy statement."""
    _force(monkeypatch, groups)
    g, tags, reps, excl, scores = _filter_case()
    users, temp = len(reps), 0.8
    _same(g.log_partition_reps(reps, temp, exclude=excl), partition_expect(scores, excl, temp), "lists")
    any_of = np.zeros(users, np.uint32)
    none_of = np.zeros(users, np.uint32)
    kind = np.arange(users) % 5
    any_of[kind == 1] = 0b1010
    none_of[kind == 2] = 0b0110
    any_of[kind == 3] = 1 << 20
    any_of[kind == 4] = 1 << 30  # no item carries bit 30
    removed = [np.flatnonzero((tags & none_of[u]) != 0)[:40].astype(np.uint32) for u in range(users)]
    for own in (None, excl, [np.concatenate([a, b]).astype(np.uint32) for a, b in zip(excl, removed)]):
        equiv = equivalent_exclusions(tags, any_of, none_of, users, own)
        got = g.log_partition_reps(reps, temp, exclude=own, any_of=any_of, none_of=none_of)
        _same(got, partition_expect(scores, equiv, temp), "masks numpy")
        _same(got, partition_expect(scores, own, temp, tags=tags, any_of=any_of, none_of=none_of), "masks numpy, by tag")
        _same(got, _pair(g.log_partition_reps(reps, temp, exclude=equiv)), "masks as exclusion lists")
        assert got.mass[4] == 0 and np.isneginf(got.shift[4])


# ------------------------------------------------------------------------------------------------
# invariances, device against device
# ------------------------------------------------------------------------------------------------
def test_invariances(monkeypatch):
    """130 users x 3 000 items, d = 16, with exclusion lists: a permutation of the rows, rows asked for alone, 1 / 3 / 7 item ranges."""
    items, users, d = 3000, 130, 16
    E, bias = _random_params(items, d, 70)
    rs = np.random.RandomState(71)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    excl = [rs.randint(0, items, u % 40).astype(np.uint32) for u in range(users)]
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    _force(monkeypatch, None)
    base = g.log_partition_reps(reps, 0.7, exclude=excl)
    _same(g.log_partition_reps(reps, 0.7, exclude=excl), _pair(base), "the same call twice")
    perm = rs.permutation(users)
    _same(g.log_partition_reps(reps[perm], 0.7, exclude=[excl[u] for u in perm]), (base.shift[perm], base.mass[perm]), "rows permuted")
    for r in (3, 127, 129):
        _same(g.log_partition_reps(reps[r:r + 1], 0.7, exclude=excl[r:r + 1]), (base.shift[r:r + 1], base.mass[r:r + 1]), f"row {r} alone")
    for groups in (1, 3, 7):
        _force(monkeypatch, groups)
        _same(g.log_partition_reps(reps, 0.7, exclude=excl), _pair(base), f"{groups} ranges")
    _force(monkeypatch, None)
    scores = _rep_scores(_oracle_of(g), items, reps[:8])
    _same(g.log_partition_reps(reps[:8], 0.7, exclude=excl[:8]), partition_expect(scores, excl[:8], 0.7), "numpy")


def test_two_host_chunks_equal_the_unsplit_calls():
    """8 192 + 200 users are two launches: the call equals its two halves asked for separately.  300 items, d = 16."""
    users, items, d = 8192 + 200, 300, 16
    E, bias = _random_params(items, d, 80)
    reps = (np.random.RandomState(81).randn(users, d) * 0.5).astype(np.float32)
    excl = [np.array([u % items, (7 * u) % items], np.uint32) for u in range(users)]
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    whole = g.log_partition_reps(reps, 2.0, exclude=excl)
    cut = 5000
    a = g.log_partition_reps(reps[:cut], 2.0, exclude=excl[:cut])
    b = g.log_partition_reps(reps[cut:], 2.0, exclude=excl[cut:])
    _same(whole, (np.concatenate([a.shift, b.shift]), np.concatenate([a.mass, b.mass])), "two chunks")
    tail = np.arange(8192, users)
    scores = _rep_scores(_oracle_of(g), items, reps[tail])
    _same(g.log_partition_reps(reps[tail], 2.0, exclude=[excl[u] for u in tail]), partition_expect(scores, [excl[u] for u in tail], 2.0),
          "second chunk numpy")
    assert np.array_equal(whole.mass[tail], partition_expect(scores, [excl[u] for u in tail], 2.0)[1])


# ------------------------------------------------------------------------------------------------
# closure on the device, sessions, log_prob=True
# ------------------------------------------------------------------------------------------------
def test_the_mass_is_the_sum_of_the_allowed_items_weights():
    """For a few rows: sum(sbr_softmax_weights(score_candidates(every allowed item))) == mass exactly, the scores the device's own."""
    g, tags, reps, excl, _ = _filter_case()
    items, rows, temp = len(tags), [0, 3, 7, 11], 1.3
    any_of = np.array([0, 0, 0b1010, 1 << 20], np.uint32)
    part = g.log_partition_reps(reps[rows], temp, exclude=[excl[u] for u in rows], any_of=any_of)
    allowed = []
    for j, u in enumerate(rows):
        ok = np.ones(items, bool)
        ok[excl[u]] = False
        if any_of[j]:
            ok &= (tags & any_of[j]) != 0
        allowed.append(np.flatnonzero(ok).astype(np.uint32))
    ptr = np.zeros(len(rows) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(a) for a in allowed])
    sc = g.score_candidates_reps(reps[rows], ptr, np.concatenate(allowed))
    for j in range(len(rows)):
        w = softmax_weights(np.asarray(sc[j], np.float32), temp, part.shift[j], part.frac_bits)
        assert sum(int(x) for x in w) == int(part.mass[j]) and int(w.max()) == 1 << part.frac_bits


@pytest.mark.parametrize("kind,d", [(ModelKind.LSTM_NORMAL, 32), (ModelKind.EWMA, 20)], ids=lambda v: getattr(v, "name", str(v)))
def test_sessions_log_partition(kind, d):
    """A store with remember = 8 (the device-made lists keep repeats and padding): store.log_partition(slots) equals
    log_partition_reps on the slots' representations with exclude = seen + the caller's lists; include_seen leaves the memory out."""
    items, n, temp = 500, 40, 1.5
    rs = np.random.RandomState(50 + d)
    E, bias = _random_params(items, d, 60 + d)
    g = _model(items, 8, d, kind, E, bias)
    st = g.sessions(3 * n, remember=8)
    slots = rs.permutation(3 * n)[:n].astype(np.uint32)
    st.append(slots, [rs.randint(0, 40, i % 13).astype(np.uint32) for i in range(n)])  # few distinct items: repeats in the memory
    reps = st.representations(slots)
    seen = st.seen(slots)
    assert any(len(set(s.tolist())) < len(s) for s in seen)
    own = [rs.randint(0, items, rs.randint(0, 30)).astype(np.uint32) for _ in range(n)]
    both = [np.concatenate([a, b]).astype(np.uint32) for a, b in zip(seen, own)]
    scores = _rep_scores(_oracle_of(g), items, reps)
    got = st.log_partition(slots, temp, exclude=own)
    _same(got, _pair(g.log_partition_reps(reps, temp, exclude=both)), "reps form")
    _same(got, partition_expect(scores, both, temp), "numpy")
    _same(st.log_partition(slots, temp), partition_expect(scores, seen, temp), "seen only")
    _same(st.log_partition(slots, temp, exclude=own, include_seen=True), _pair(g.log_partition_reps(reps, temp, exclude=own)), "include_seen")
    _same(st.log_partition(slots, temp, include_seen=True), _pair(g.log_partition_reps(reps, temp)), "include_seen, no lists")
    _same(st.log_partition(slots[7:8], temp, exclude=own[7:8]), (got.shift[7:8], got.mass[7:8]), "a slot alone")
    st.close()


def test_log_prob_is_a_fourth_output():
    """recommend_sampled(..., log_prob=True) on a model, from representations and on a store: items, scores and keys are the plain
    call's bit for bit, and log_prob is slate_log_prob_expect of the partition with the same arguments, to 1e-12."""
    g, tags, reps, excl, scores = _filter_case()
    users, k, temp = len(reps), 30, 0.8
    any_of = np.where(np.arange(users) % 5 == 3, 1 << 20, 0).astype(np.uint32)  # every fifth row is short: padding
    kw = dict(temperature=temp, seed=77, exclude=excl, any_of=any_of)
    plain = g.recommend_sampled_reps(reps, k, **kw)
    got = g.recommend_sampled_reps(reps, k, log_prob=True, **kw)
    assert len(plain) == 3 and len(got) == 4 and got[3].dtype == np.float64 and got[3].shape == (users, k)
    for a, b in zip(plain, got):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    shift, mass = partition_expect(scores, excl, temp, tags=tags, any_of=any_of)
    want = slate_log_prob_expect(plain[1], temp, shift, mass, frac_bits(len(tags)))
    assert np.array_equal(np.isnan(got[3]), np.isnan(want)) and np.nanmax(np.abs(got[3] - want)) <= 1e-12
    assert np.isnan(got[3][3]).any() and not np.isnan(got[3][0]).any() and np.all(got[3][0] < 0)
    ptr, it = synthetic_interactions(users, len(tags), 8, seed=1, min_len=1)
    h3, h4 = g.recommend_sampled(ptr, it, 5, temperature=2.0, seed=1), g.recommend_sampled(ptr, it, 5, temperature=2.0, seed=1, log_prob=True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(h3, h4))
    assert np.array_equal(h4[3], g.log_partition(ptr, it, 2.0).slate_log_prob(h3[1]))
    st = g.sessions(users, remember=4)
    st.append(np.arange(users), [excl[u][:6] for u in range(users)])
    s3, s4 = st.recommend_sampled(np.arange(users), 5, seed=2), st.recommend_sampled(np.arange(users), 5, seed=2, log_prob=True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(s3, s4))
    assert np.array_equal(s4[3], st.log_partition(np.arange(users), 1.0).slate_log_prob(s3[1])) and np.all(s4[3] < 0)
    st.close()


# ------------------------------------------------------------------------------------------------
# errors, the ledger
# ------------------------------------------------------------------------------------------------
SENTINEL_F32, SENTINEL_U64, SENTINEL_U32 = np.float32(-123.5), np.uint64(0xABCDEF0123456789), 0xABCDEF01


def _raw_reps_call(g, reps, temperature, any_of=None):
    """sbr_log_partition_reps through ctypes with sentinel-filled outputs -> (status, untouched)"""
    L = _lib.load()
    reps = np.ascontiguousarray(reps, np.float32)
    n = reps.shape[0]
    shift, mass, fb = np.full(n, SENTINEL_F32, np.float32), np.full(n, SENTINEL_U64, np.uint64), C.c_uint32(SENTINEL_U32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = L.sbr_log_partition_reps(g._h, p(reps), n, None, None, temperature, p(any_of), None, p(shift), p(mass), C.byref(fb))
    return st, bool(np.all(shift == SENTINEL_F32) and np.all(mass == SENTINEL_U64) and fb.value == SENTINEL_U32)


def test_errors_leave_outputs_and_model_untouched():
    """Temperature 0, negative, NaN, inf and 1e-39; masks on a model without tags; the non-finite rule — an item bias of 3e38 at
    T = 0.5 (t overflows while the score is finite), also when the item is excluded, and a NaN embedding row — with recommend's
    status.  Each writes nothing and leaves the model as it was."""
    items, d, users = 300, 16, 10
    E, bias = _random_params(items, d, 90)
    reps = np.abs(np.random.RandomState(91).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    before = g.log_partition_reps(reps, 0.5)

    def refused(call):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.INVALID_ARGUMENT

    ptr, it = synthetic_interactions(users, items, 8, seed=1, min_len=1)
    st = g.sessions(4)
    st.append([0, 1], [[1, 2], [3]])
    for temp in (0.0, -1.0, float("nan"), float("inf"), 1e-39):
        refused(lambda: g.log_partition_reps(reps, temp))
        refused(lambda: g.log_partition(ptr, it, temp))
        refused(lambda: st.log_partition([0, 1], temp))
        assert _raw_reps_call(g, reps, temp) == (Status.INVALID_ARGUMENT, True), temp
    assert g.log_partition_reps(reps, 3e38).mass.shape == (users,)
    refused(lambda: g.log_partition_reps(reps, 1.0, any_of=1))
    refused(lambda: g.recommend_reps(reps, 5, any_of=1))  # the counterpart
    refused(lambda: st.log_partition([0, 1], 1.0, none_of=1))
    assert _raw_reps_call(g, reps, 1.0, any_of=np.ones(users, np.uint32)) == (Status.INVALID_ARGUMENT, True)
    with pytest.raises(ValueError):
        st.log_partition([0, 1], 1.0, include_seen=True)  # a store without memory, as Sessions.recommend
    st.close()
    big = bias.copy()
    big[123] = 3e38
    g.set_param(Param.ITEM_BIAS, big)
    assert np.all(np.isfinite(g.recommend_reps(reps, 5)[1]))
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.log_partition_reps(reps, 0.5)
    with pytest.raises(PredictionError.InvalidPredictionValue):  # also when the item is excluded: it is a scanned pair
        g.log_partition_reps(reps, 0.5, exclude=[[123]] * users)
    assert _raw_reps_call(g, reps, 0.5) == (Status.INVALID_PREDICTION, True)
    assert np.all(g.log_partition_reps(reps, 2.0).mass == np.uint64(1 << 40))  # 1.5e38 is a shift like any other
    g.set_param(Param.ITEM_BIAS, bias)
    En = E.copy()
    En[200] = np.nan
    g.set_param(Param.ITEM_EMBEDDING, En)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.recommend_reps(reps, 5)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.log_partition_reps(reps, 0.5)
    assert _raw_reps_call(g, reps, 1.0) == (Status.INVALID_PREDICTION, True)
    g.set_param(Param.ITEM_EMBEDDING, E)
    _same(g.log_partition_reps(reps, 0.5), _pair(before), "after the errors")


def test_launch_count():
    """The RANK family of the timing ledger counts four launches for one chunk — scan, merge, shift, sum scan — and the finish as a
    fifth where there are exclusion lists."""
    items, d, users = 300, 16, 10
    E, bias = _random_params(items, d, 95)
    reps = (np.random.RandomState(96).randn(users, d) * 0.5).astype(np.float32)
    g = _model(items, 8, d, ModelKind.EWMA, E, bias)
    g.timing_enable(True)
    g.timing_read()  # the read resets the ledger
    g.log_partition_reps(reps, 1.0)
    assert int(g.timing_read()["RANK"][1]) == 4
    g.log_partition_reps(reps, 1.0, exclude=[[1]] * users)
    assert int(g.timing_read()["RANK"][1]) == 5
    g.timing_enable(False)
