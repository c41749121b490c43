"""GPU: every call family on POISONED scratch memory (SBR_TEST_POISON, include/sbr_hip.h).  The engine's scratch comes
from a process-wide cache that hands blocks of finished calls out again and from a serving arena that every call carves anew out of
what the previous call left there; the rest of the suite almost always meets that memory fresh.  Here every block the cache hands
out and every carve of the arena is first filled with one byte, so a kernel that relies on zeros, or on the leftovers of the last
call, loses bit-parity with its expectation.  Every test runs under three patterns:

    0xFF  every f32 a NaN; every u32 0xFFFFFFFF — NO_ITEM / TK_NONE, and the largest count; every flag set
    0x7F  every f32 3.39e38: finite, passes every >=, overflows a sum to inf; every i32 huge and positive
    0x80  every f32 -1.2e-38; every i32 negative, which prev_row reads as "first step"

The module fixture `hook_is_live` proves, through sbr_selftest_scratch / sbr_selftest_arena, that the build fills device blocks,
pinned host blocks and the arena on the first AND on the re-used allocation: a build without the hook fails there, not vacuously.

Every comparison is equality — ids, counts, f32 bits — with the oracle or the numpy statement the family's clean test uses
(recommend_expect, rank_expect, similar_expect, diverse_expect, filter_expect, sampled_expect, partition_expect, above_expect,
top_expect, capped_expect, audience_expect, seen_expect, the oracle's fit).  No family is compared with an unpoisoned GPU run.
recommend_sampled's log_prob, a float64 the host computes from the partition, is held to the same host function applied to the
expected shift and mass.

Shapes: test_sampled_gpu._core_case — 1 000 items (32 tiles, the last ragged) x 130 rows (the second row tile nearly empty) — at
d = 16 and d = 100 (stored as 128: the padded columns), SBR_CATALOGUE_GROUPS=3 (several tiles per range; merge and offsets run).
The groups of a GPU run, in the order they are meant to be run: -k selftest, -k sort, -k serving, -k sessions, -k training."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import audience_expect as ae
import test_numerics_gpu
import test_parity_gpu as parity
from above_expect import above_expect, counts_expect
from capped_expect import capped_rows, ranking
from diverse_expect import DiverseExpectation
from filter_expect import equivalent_exclusions, filtered_expect
from helpers import LOSS_BPR, LOSS_HINGE, LOSS_WARP, OPT_ADAM, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from partition_expect import frac_bits, partition_expect
from rank_expect import expect_all
from recommend_expect import NO_ITEM, topk_expectation
from sampled_expect import sampled_expect
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ModelKind
from sbr_rs_amd.engine import Model, Partition
from seen_expect import SeenModel
from test_above_gpu import _both_orders as _above_both_orders
from test_above_gpu import _quantile_thresholds
from test_capped_gpu import _same as _same_capped
from test_partition_gpu import _same as _same_partition
from test_sampled_gpu import CORE_ITEMS, CORE_T, CORE_USERS, _bits, _core_case, _model, _oracle_of, _rep_scores
from test_sampled_gpu import _same as _same_sampled
from test_sessions_gpu import ITEMS as S_ITEMS
from test_sessions_gpu import append_ragged, random_params
from test_top_gpu import _both_orders as _top_both_orders
from test_top_gpu import _mixed_budgets
from top_expect import top_expect

pytestmark = pytest.mark.gpu

HOOK, GROUPS_HOOK, FILL_HOOK = "SBR_TEST_POISON", "SBR_CATALOGUE_GROUPS", "SBR_ABOVE_FILL_BYTES"
PATTERNS = [0xFF, 0x7F, 0x80]
NORMAL, COUPLED, EWMA = ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA
CASES = [(NORMAL, 16), (NORMAL, 100), (EWMA, 16), (EWMA, 100)]
case_ids = lambda v: getattr(v, "name", str(v))  # noqa: E731


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------
# the hook
# ------------------------------------------------------------------------------------------------
def _selftest_copies(pattern, big=True):
    """{what: the bytes of the first and of the re-used allocation} under SBR_TEST_POISON=pattern (None: unset); big: also blocks
    past the cache's 64 MiB, which go to the driver and back"""
    L = _lib.load()
    before = os.environ.get(HOOK)
    if pattern is None:
        os.environ.pop(HOOK, None)
    else:
        os.environ[HOOK] = str(pattern)
    try:
        out = {}
        for kind, what in ((0, "device"), (1, "pinned")):
            for nbytes in (4096 + 100, (64 << 20) + 4096)[: 2 if big else 1]:  # a cached size (no multiple of 256); past the cache
                buf = np.zeros(2 * nbytes, np.uint8)
                assert L.sbr_selftest_scratch(kind, nbytes, _p(buf)) == 0
                out[f"{what} {nbytes}"] = buf
        g = Model(hparams(50, 8, 16, int(EWMA), LOSS_HINGE))
        for nbytes in (70_000, 300):  # the second carve pair is smaller than what the arena holds by then
            buf = np.zeros(2 * nbytes, np.uint8)
            assert L.sbr_selftest_arena(g._h, nbytes, _p(buf)) == 0
            out[f"arena {nbytes}"] = buf
        g.close()
        return out
    finally:
        if before is None:
            os.environ.pop(HOOK, None)
        else:
            os.environ[HOOK] = before


@pytest.fixture(scope="module")
def hook_is_live():
    """Every byte of every copy equals the pattern — device, pinned and arena memory, first and re-used allocation — for each of the
    three patterns: the tests below run on poisoned memory or not at all."""
    for pattern in PATTERNS:
        for what, buf in _selftest_copies(pattern).items():
            bad = np.flatnonzero(buf != pattern)
            assert bad.size == 0, f"SBR_TEST_POISON={pattern:#x}: {what}: {bad.size} bytes are not the pattern, first at {bad[0]}: {buf[bad[0]]:#x}"
    return True


@pytest.fixture(params=PATTERNS, ids=lambda p: f"poison{p:02X}")
def poison(request, monkeypatch, hook_is_live):
    monkeypatch.setenv(HOOK, str(request.param))
    monkeypatch.setenv(GROUPS_HOOK, "3")
    return request.param


def test_selftest_hook_fills_first_and_reused_allocations(poison):
    """The fixture's proof as a test of its own, and the other half: with the hook off the second carve of the arena comes back as
    the zeros the selftest wrote into the first (so the second copy above was the same memory, not fresh memory)."""
    for what, buf in _selftest_copies(poison, big=False).items():
        assert np.all(buf == poison), what
    for what, buf in _selftest_copies(None, big=False).items():
        if what.startswith("arena"):
            assert not np.any(buf[buf.size // 2:]), f"hook off: {what}: the second carve holds the zeros written into the first"


@pytest.mark.parametrize("kind", [EWMA, NORMAL, COUPLED], ids=case_ids)
@pytest.mark.parametrize("d", [24, 100])
def test_selftest_model_creation_matches_the_oracle(poison, kind, d):
    """Parameter arrays come through the same allocator: a new model's parameters and accumulators, padded widths included, are
    the oracle's."""
    parity.test_init_matches(kind, d)


# ------------------------------------------------------------------------------------------------
# sort: the radix passes live on scratch histograms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small,items", [("0", None), ("0", "64")])
@pytest.mark.parametrize("n,row_bits,dist", [(4097, 6, "uniform"), (100_000, 11, "zipf")])
def test_sort_on_poisoned_histograms(poison, monkeypatch, n, row_bits, dist, small, items):
    test_numerics_gpu.test_key_ordering_is_a_stable_sort_by_row(_lib.load(), monkeypatch, n, row_bits, dist, small, items)


# ------------------------------------------------------------------------------------------------
# serving: the core case and what the families' expectations need of it, made once and read only
# ------------------------------------------------------------------------------------------------
class _Case:
    def __init__(self, kind, d):
        self.kind, self.d = kind, d
        self.E, self.bias, self.params, self.ptr, self.it, self.hists, self.scores = _core_case(kind, d)
        g = self.model()
        self.o = _oracle_of(g)
        g.close()
        self.uniq = [np.unique(h) for h in self.hists]
        self.reps = np.array([self.o.user_representation(h) for h in self.hists], np.float32)
        assert np.array_equal(_bits(_rep_scores(self.o, CORE_ITEMS, self.reps[:3])), _bits(self.scores[:3]))
        rs = np.random.RandomState(1000 * int(kind) + d)
        self.excl = [rs.randint(0, CORE_ITEMS, rs.randint(0, 50)).astype(np.uint32) for _ in range(CORE_USERS)]
        self.excl[3] = np.arange(0, CORE_ITEMS, 2, dtype=np.uint32)
        self.excl[5] = np.delete(np.arange(CORE_ITEMS, dtype=np.uint32), [17, 400, 999])  # three eligible items: short rows
        self.tags = (np.uint32(1) << rs.randint(0, 8, CORE_ITEMS).astype(np.uint32)).astype(np.uint32)
        self.any_of = np.where(np.arange(CORE_USERS) % 4 == 1, 0b1010, 0).astype(np.uint32)
        self.none_of = np.where(np.arange(CORE_USERS) % 4 == 2, 0b0110, 0).astype(np.uint32)
        self.any_of[7] = 1 << 30  # no item carries it: a row of padding
        self.groups = np.where(rs.rand(CORE_ITEMS) < 0.7, 7, np.arange(CORE_ITEMS) + 100).astype(np.uint32)  # one large group
        self.queries = np.concatenate([rs.permutation(CORE_ITEMS)[:38], [0, CORE_ITEMS - 1]]).astype(np.uint32)
        self.queries[30:35] = self.queries[0:5]  # repeats
        self.qexcl = [rs.randint(0, CORE_USERS, j % 5).astype(np.uint32) for j in range(len(self.queries))]
        self.holders = [[u for u in range(CORE_USERS) if int(q) in self.uniq[u].tolist()] for q in self.queries]
        self.tscores = np.ascontiguousarray(self.scores.T[self.queries])  # [queries, users]

    def model(self, tags=None, groups=None):
        g = _model(CORE_ITEMS, CORE_T, self.d, self.kind, self.E, self.bias, tags)
        for w, v in self.params.items():
            g.set_param(w, v)
        if groups is not None:
            g.set_item_groups(groups)
        return g

    def topk(self, excl, k, rows=None):
        rows = range(CORE_USERS) if rows is None else rows
        out = [topk_expectation(self.scores[u], () if excl is None else excl[u], k) for u in rows]
        return np.array([r[0] for r in out], np.uint32).reshape(-1, k), np.array([r[1] for r in out], np.float32).reshape(-1, k)


@functools.lru_cache(maxsize=None)
def _case(kind, d):
    return _Case(kind, d)


def _same_rows(got, want, what=""):
    """(ids [n, k] u32, scores [n, k] f32): the ids as integers, the scores bit for bit"""
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float32 and got[0].shape == want[0].shape, what
    bad = np.argwhere(got[0] != want[0])
    assert bad.size == 0, f"{what}: {len(bad)} ids differ; first at {bad[0]}: {got[0][tuple(bad[0])]} vs {want[0][tuple(bad[0])]}"
    bad = np.argwhere(_bits(got[1]) != _bits(want[1]))
    assert bad.size == 0, f"{what}: {len(bad)} score bits differ; first at {bad[0]}: {got[1][tuple(bad[0])]!r} vs {want[1][tuple(bad[0])]!r}"


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, np.uint32) for x in lists] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return ptr, flat


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_recommend(poison, kind, d):
    """recommend over histories and recommend_reps with exclusion lists (one of them leaves three items), k = 10 and 1 024 (past the
    catalogue: padded rows)."""
    c = _case(kind, d)
    g = c.model()
    for k in (10, 1024):
        _same_rows(g.recommend(c.ptr, c.it, k), c.topk(c.uniq, k), f"recommend k={k}")
        _same_rows(g.recommend_reps(c.reps, k, exclude=c.excl), c.topk(c.excl, k), f"recommend_reps k={k}")
    _same_rows(g.recommend(c.ptr, c.it, 10, include_history=True), c.topk(None, 10), "include_history")
    g.close()


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_mrr_score_and_rank_targets(poison, kind, d):
    """mrr_score against the oracle's; rank_targets with 0 .. 20 targets per user (more than a scan-user's 16: two scan-users), the
    history masked and not, and the _reps form with exclusion lists."""
    c = _case(kind, d)
    g = c.model()
    mg, rg = g.mrr_score(c.ptr, c.it)
    mo, ro = c.o.mrr_score(c.ptr, c.it)
    assert np.array_equal(rg, ro) and mg == mo
    rs = np.random.RandomState(d)
    targets = [rs.randint(0, CORE_ITEMS, u % 21).astype(np.uint32) for u in range(CORE_USERS)]
    for u in range(0, CORE_USERS, 7):  # targets inside the history: masked to f32::MIN
        if len(c.hists[u]) and len(targets[u]):
            targets[u][0] = c.hists[u][0]
    tptr, tit = _csr(targets)
    for include in (False, True):
        want = np.concatenate(expect_all(c.scores, c.hists, targets, mask_history=not include))
        assert np.array_equal(g.rank_targets(c.ptr, c.it, tptr, tit, include_history=include), want), f"include={include}"
    want = np.concatenate(expect_all(c.scores, c.excl, targets))
    assert np.array_equal(g.rank_targets_reps(c.reps, tptr, tit, exclude=c.excl), want), "reps form"
    g.close()


@functools.lru_cache(maxsize=None)
def _diverse(kind, d, metric):
    return DiverseExpectation(_case(kind, d).E, metric)


def _similar(kind, d, metric):
    return _diverse(kind, d, metric).sim


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("kind,d", [(EWMA, 16), (EWMA, 100)], ids=case_ids)
def test_serving_similar_items(poison, kind, d, metric):
    c = _case(kind, d)
    g = c.model()
    want = _similar(kind, d, metric)
    qex = [c.excl[j] for j in range(len(c.queries))]
    for k in (10, 1024):
        _same_rows(g.similar_items(c.queries, k, metric=metric), want.rows(c.queries, k), f"k={k}")
    _same_rows(g.similar_items(c.queries, 10, metric=metric, include_self=True, exclude=qex), want.rows(c.queries, 10, True, qex), "lists")
    g.close()


@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 100)], ids=case_ids)
def test_serving_recommend_diverse(poison, kind, d):
    c = _case(kind, d)
    g = c.model()
    for metric in ("cosine", "dot"):
        want = _diverse(kind, d, metric)
        for k, pool in ((10, 64), (33, 65)):
            _same_rows(g.recommend_diverse(c.ptr, c.it, k, pool, 0.3, metric), want.rows(c.topk(c.uniq, pool), k, 0.3), f"{metric} {k}/{pool}")
            _same_rows(g.recommend_diverse_reps(c.reps, k, pool, 0.3, metric, exclude=c.excl), want.rows(c.topk(c.excl, pool), k, 0.3),
                       f"{metric} {k}/{pool} reps")
    g.close()


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_candidates(poison, kind, d):
    """recommend(among=) over a subset of 300 items (the sub-table is gathered into the arena), score_candidates and
    user_representations."""
    c = _case(kind, d)
    g = c.model()
    rs = np.random.RandomState(d + 1)
    subset = rs.permutation(CORE_ITEMS)[:300].astype(np.uint32)
    outside = np.setdiff1d(np.arange(CORE_ITEMS), subset)
    for k in (10, 301):
        want = c.topk([np.concatenate([outside, c.uniq[u]]) for u in range(CORE_USERS)], k)
        _same_rows(g.recommend_among(c.ptr, c.it, k, subset), want, f"among k={k}")
    want = c.topk([np.concatenate([outside, c.excl[u]]) for u in range(CORE_USERS)], 10)
    _same_rows(g.recommend_among_reps(c.reps, 10, subset, exclude=c.excl), want, "among reps")
    cands = [rs.randint(0, CORE_ITEMS, u % 37).astype(np.uint32) for u in range(CORE_USERS)]
    cptr, cit = _csr(cands)
    for got in (g.score_candidates(c.ptr, c.it, cptr, cit), g.score_candidates_reps(c.reps, cptr, cit)):
        assert len(got) == CORE_USERS
        for u in range(CORE_USERS):
            assert np.array_equal(_bits(got[u]), _bits(c.scores[u][cands[u]])), u
    assert np.array_equal(_bits(g.user_representations(c.ptr, c.it)), _bits(c.reps))
    g.close()


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_filtered(poison, kind, d):
    """The tag filter of recommend, recommend_reps, similar_items and recommend_diverse: any_of, none_of, neither, and a mask no item
    carries."""
    c = _case(kind, d)
    g = c.model(tags=c.tags)
    for k in (10, 1024):
        _same_rows(g.recommend(c.ptr, c.it, k, any_of=c.any_of, none_of=c.none_of), filtered_expect(c.scores, c.tags, c.any_of, c.none_of, c.uniq, k),
                   f"recommend k={k}")
    got = g.recommend_reps(c.reps, 10, exclude=c.excl, any_of=c.any_of, none_of=c.none_of)
    _same_rows(got, filtered_expect(c.scores, c.tags, c.any_of, c.none_of, c.excl, 10), "recommend_reps")
    assert np.all(got[0][7] == NO_ITEM)
    equiv = equivalent_exclusions(c.tags, c.any_of, c.none_of, CORE_USERS, c.excl)
    want = _diverse(kind, d, "dot")
    _same_rows(g.recommend_diverse_reps(c.reps, 10, 64, 0.3, "dot", exclude=c.excl, any_of=c.any_of, none_of=c.none_of),
               want.rows(c.topk(equiv, 64), 10, 0.3), "diverse")
    nq = len(c.queries)
    qequiv = equivalent_exclusions(c.tags, c.any_of[:nq], c.none_of[:nq], nq)
    _same_rows(g.similar_items(c.queries, 10, metric="dot", any_of=c.any_of[:nq], none_of=c.none_of[:nq]), want.sim.rows(c.queries, 10, False, qequiv),
               "similar_items")
    g.close()


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_recommend_sampled(poison, kind, d):
    """recommend_sampled with log_prob=True: items, plain scores and keys against the numpy restatement of the noise; the
    propensities are the host's function of the expected partition."""
    c = _case(kind, d)
    g = c.model()
    k, temp, seed = 100, 0.5, 20261020
    for what, got, excl in (("histories", g.recommend_sampled(c.ptr, c.it, k, temperature=temp, seed=seed, log_prob=True), c.uniq),
                            ("reps", g.recommend_sampled_reps(c.reps, k, temperature=temp, seed=seed, exclude=c.excl, log_prob=True), c.excl)):
        assert len(got) == 4
        want = sampled_expect(c.scores, excl, k, temp, seed)
        _same_sampled(got[:3], want, what)
        shift, mass = partition_expect(c.scores, excl, temp)
        lp = Partition(temp, shift, mass, frac_bits(CORE_ITEMS)).slate_log_prob(want[1])
        assert got[3].dtype == np.float64 and np.array_equal(got[3], lp, equal_nan=True), what
    g.close()


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_log_partition(poison, kind, d):
    """log_partition over histories, and from representations with exclusion lists and tag masks (a row that may see nothing has
    mass 0)."""
    c = _case(kind, d)
    g = c.model(tags=c.tags)
    for temp in (0.5, 4.0):
        _same_partition(g.log_partition(c.ptr, c.it, temperature=temp), partition_expect(c.scores, c.uniq, temp), f"T={temp}")
        got = g.log_partition_reps(c.reps, temperature=temp, exclude=c.excl, any_of=c.any_of, none_of=c.none_of)
        _same_partition(got, partition_expect(c.scores, c.excl, temp, tags=c.tags, any_of=c.any_of, none_of=c.none_of), f"T={temp} masks")
        assert got.mass[7] == 0 and got.frac_bits == frac_bits(CORE_ITEMS)
    g.close()


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_above(poison, monkeypatch, kind, d):
    """recommend_above / count_above (about 56 000 pairs) and audience_above with the fill cut into three ranges and more."""
    c = _case(kind, d)
    g = c.model()
    t = _quantile_thresholds(c.scores)
    total = int(counts_expect(c.scores, t, c.uniq).sum())
    monkeypatch.setenv(FILL_HOOK, str(8 * (total // 3 - 1000)))
    assert total > 30_000
    _above_both_orders(lambda order: g.recommend_above(c.ptr, c.it, t, order=order), lambda: g.count_above(c.ptr, c.it, t), c.scores, t, c.uniq,
                       what="histories")
    _above_both_orders(lambda order: g.recommend_above_reps(c.reps, t, exclude=c.excl, order=order),
                       lambda: g.count_above_reps(c.reps, t, exclude=c.excl), c.scores, t, c.excl, what="reps")
    tq = np.quantile(c.tscores, 0.6, axis=1).astype(np.float32)
    monkeypatch.setenv(FILL_HOOK, str(8 * (int(counts_expect(c.tscores, tq, c.holders).sum()) // 3 - 50)))
    _above_both_orders(lambda order: g.audience_above(c.ptr, c.it, c.queries, tq, order=order),
                       lambda: g.count_audience_above(c.ptr, c.it, c.queries, tq), c.tscores, tq, c.holders, what="audience")
    _above_both_orders(lambda order: g.audience_above_reps(c.reps, c.queries, tq, exclude=c.qexcl, order=order),
                       lambda: g.count_audience_above_reps(c.reps, c.queries, tq, exclude=c.qexcl), c.tscores, tq, c.qexcl, what="audience reps")
    g.close()


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_top(poison, monkeypatch, kind, d):
    """recommend_top / nth_score and audience_top with a budget per row: zeros, values past the catalogue, everything between."""
    c = _case(kind, d)
    g = c.model()
    n = _mixed_budgets(CORE_USERS, CORE_ITEMS, d)
    assert (n == 0).any() and (n > CORE_ITEMS).any()
    monkeypatch.setenv(FILL_HOOK, "80000")  # 10 000 entries a range: the rows that take the whole catalogue go about nine to a range
    _top_both_orders(lambda order: g.recommend_top(c.ptr, c.it, n, order=order), lambda: g.nth_score(c.ptr, c.it, n), c.scores, n, c.uniq,
                     what="histories")
    _top_both_orders(lambda order: g.recommend_top_reps(c.reps, n, exclude=c.excl, order=order), lambda: g.nth_score_reps(c.reps, n, exclude=c.excl),
                     c.scores, n, c.excl, what="reps")
    nq = _mixed_budgets(len(c.queries), CORE_USERS, d + 1)
    monkeypatch.setenv(FILL_HOOK, "4000")
    _top_both_orders(lambda order: g.audience_top(c.ptr, c.it, c.queries, nq, order=order), lambda: g.nth_audience_score(c.ptr, c.it, c.queries, nq),
                     c.tscores, nq, c.holders, what="audience")
    _top_both_orders(lambda order: g.audience_top_reps(c.reps, c.queries, nq, exclude=c.qexcl, order=order),
                     lambda: g.nth_audience_score_reps(c.reps, c.queries, nq, exclude=c.qexcl), c.tscores, nq, c.qexcl, what="audience reps")
    g.close()


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_recommend_capped(poison, kind, d):
    """70 % of the catalogue in one group at cap 2: the device's pool of 64 keeps about twenty entries of 33, so the completion
    (recommend_top at a growing n, the rule on the host) runs for nearly every row; and the device's own rows and flags at that pool."""
    c = _case(kind, d)
    g = c.model(groups=c.groups)
    k, cap, pool = 33, 2, 64
    for what, excl, call in (("histories", c.uniq, lambda exact: g.recommend_capped(c.ptr, c.it, k, cap, pool, exact=exact)),
                             ("reps", c.excl, lambda exact: g.recommend_capped_reps(c.reps, k, cap, pool, exclude=c.excl, exact=exact))):
        ranks = [ranking(c.scores[u], excl[u]) for u in range(CORE_USERS)]
        device = capped_rows(ranks, c.groups, cap, k, pool)
        assert np.count_nonzero(~device[2]) > CORE_USERS // 2
        _same_capped(call(False), device, what + " device")
        _same_capped(call(True), capped_rows(ranks, c.groups, cap, k), what + " exact")
    g.close()


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_audience(poison, kind, d):
    """audience_reps with the caller's exclusion lists, and audience over histories (the holders of a query item left out), k = 10
    and past the 130 candidates."""
    c = _case(kind, d)
    g = c.model()
    ids = np.arange(CORE_USERS, dtype=np.uint32)
    for k in (10, CORE_USERS + 7):
        for what, got, excl in (("reps", g.audience_reps(c.reps, c.queries, k, exclude=c.qexcl), c.qexcl),
                                ("histories", g.audience(c.ptr, c.it, c.queries, k), c.holders)):
            rows, score_bits = ae.expected_rows(_bits(c.tscores), ids, k, excl)
            assert np.array_equal(got[0], rows) and np.array_equal(_bits(got[1]), score_bits), (what, k)
    g.close()


# ------------------------------------------------------------------------------------------------
# interleaved calls on one model, hook off and on: the arena is re-carved under another layout by every call
# ------------------------------------------------------------------------------------------------
MIX_ROWS = 300


@functools.lru_cache(maxsize=None)
def _mix_case():
    """(the core case of LSTM d = 16, 300 representation rows — its 130 and 170 random ones — and the oracle's scores of them)"""
    c = _case(NORMAL, 16)
    extra = (np.random.RandomState(77).randn(MIX_ROWS - CORE_USERS, 16) * 0.5).astype(np.float32)
    reps = np.concatenate([c.reps, extra])
    scores = np.concatenate([c.scores, _rep_scores(c.o, CORE_ITEMS, extra)])
    rs = np.random.RandomState(78)
    excl = list(c.excl) + [rs.randint(0, CORE_ITEMS, rs.randint(0, 50)).astype(np.uint32) for _ in range(MIX_ROWS - CORE_USERS)]
    return c, reps, scores, excl


def _mix_call(g, spec):
    """one call of the mix -> something comparable by _mix_equal"""
    c, reps, scores, excl = _mix_case()
    family, rows, arg = spec
    r, x = reps[:rows], excl[:rows]
    if family == "recommend_reps":
        return g.recommend_reps(r, arg, exclude=x)
    if family == "recommend":
        return g.recommend(c.ptr[: rows + 1], c.it, arg)
    if family == "rank_targets_reps":
        tptr, tit = _csr([np.arange(u % arg, dtype=np.uint32) * 7 for u in range(rows)])
        return (g.rank_targets_reps(r, tptr, tit, exclude=x),)
    if family == "similar_items":
        return g.similar_items(np.arange(rows, dtype=np.uint32) * 3, arg, metric="dot")
    if family == "above":
        a = g.recommend_above_reps(r, np.float32(arg), exclude=x, order="id")
        return a.ptr, a.ids, a.scores
    if family == "count_above":
        return (g.count_above_reps(r, np.float32(arg), exclude=x),)
    if family == "top":
        a = g.recommend_top_reps(r, arg, exclude=x)
        return a.ptr, a.ids, a.scores, a.cuts
    if family == "partition":
        p = g.log_partition_reps(r, arg, exclude=x)
        return p.shift, p.mass
    if family == "sampled":
        return g.recommend_sampled_reps(r, arg, temperature=0.7, seed=5, exclude=x)
    if family == "capped":
        return g.recommend_capped_reps(r, arg, 2, 64, exclude=x, exact=False)
    if family == "audience":
        return g.audience_reps(r, c.queries, arg)
    if family == "candidates":
        cptr, cit = _csr([np.arange(u % arg + 1, dtype=np.uint32) * 11 for u in range(rows)])
        return (np.concatenate(g.score_candidates_reps(r, cptr, cit) + [np.zeros(0, np.float32)]),)
    raise AssertionError(family)


@functools.lru_cache(maxsize=None)
def _mix_want(spec):
    """the expectation of a distinct call, computed once"""
    c, reps, scores, excl = _mix_case()
    family, rows, arg = spec
    s, x = scores[:rows], excl[:rows]

    def topk(sc, ex, k):
        out = [topk_expectation(sc[u], ex[u], k) for u in range(len(sc))]
        return np.array([o[0] for o in out], np.uint32).reshape(-1, k), np.array([o[1] for o in out], np.float32).reshape(-1, k)

    if family == "recommend_reps":
        return topk(s, x, arg)
    if family == "recommend":
        return topk(s, c.uniq[:rows], arg)
    if family == "rank_targets_reps":
        return (np.concatenate(expect_all(s, x, [np.arange(u % arg, dtype=np.uint32) * 7 for u in range(rows)]) + [np.zeros(0, np.uint32)]),)
    if family == "similar_items":
        return _similar(NORMAL, 16, "dot").rows(np.arange(rows) * 3, arg)
    if family == "above":
        return above_expect(s, np.float32(arg), x, None, "id")
    if family == "count_above":
        return (counts_expect(s, np.float32(arg), x),)
    if family == "top":
        return top_expect(s, arg, x)
    if family == "partition":
        return partition_expect(s, x, arg)
    if family == "sampled":
        return sampled_expect(s, x, arg, 0.7, 5)
    if family == "capped":
        return capped_rows([ranking(s[u], x[u]) for u in range(rows)], c.groups, 2, arg, 64)
    if family == "audience":
        rows_, bits_ = ae.expected_rows(_bits(np.ascontiguousarray(s.T[c.queries])), np.arange(rows, dtype=np.uint32), arg)
        return rows_, bits_.view(np.float32)
    if family == "candidates":
        return (np.concatenate([s[u][np.arange(u % arg + 1) * 11] for u in range(rows)] + [np.zeros(0, np.float32)]).astype(np.float32),)
    raise AssertionError(family)


def _mix_equal(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        if a.dtype == np.float32:
            assert np.array_equal(_bits(a), _bits(b)), (what, i, np.argwhere(_bits(a) != _bits(b))[:3].tolist())
        else:
            assert np.array_equal(a, b.astype(a.dtype)), (what, i, np.argwhere(a != b.astype(a.dtype))[:3].tolist())


MIX_SPECS = [
    ("recommend_reps", 1, 10), ("recommend_reps", 300, 10), ("recommend_reps", 33, 1024), ("recommend", 130, 100), ("recommend", 33, 1),
    ("rank_targets_reps", 130, 21), ("rank_targets_reps", 300, 5), ("similar_items", 33, 50), ("similar_items", 300, 7),
    ("above", 300, 0.5), ("above", 33, -1.0), ("above", 1, -np.inf), ("count_above", 130, 0.25), ("top", 300, 40), ("top", 33, 1500), ("top", 1, 0),
    ("partition", 300, 1.0), ("partition", 33, 0.25), ("sampled", 130, 100), ("sampled", 300, 3), ("capped", 130, 33), ("capped", 1, 5),
    ("audience", 300, 10), ("audience", 33, 40), ("candidates", 300, 37), ("candidates", 1, 2),
]


@pytest.mark.parametrize("pattern", [None] + PATTERNS, ids=lambda p: "clean" if p is None else f"poison{p:02X}")
def test_serving_interleaved_calls_on_one_model(monkeypatch, hook_is_live, pattern):
    """52 calls — every distinct call of MIX_SPECS twice, in a fixed-seed shuffle — on ONE model, rows 1, 33, 130 and 300, the item
    ranges forced to 1, to 3, or left to the library: the arena grows and is carved under another layout by every call, and with the
    hook off what a call finds there is the previous call's real data — ids, counts, offsets, scores.  Every result equals its
    expectation."""
    if pattern is None:
        monkeypatch.delenv(HOOK, raising=False)
    else:
        monkeypatch.setenv(HOOK, str(pattern))
    c = _mix_case()[0]
    g = c.model(groups=c.groups)
    rs = np.random.RandomState(20261020)
    order = rs.permutation(2 * len(MIX_SPECS))
    assert len(order) >= 40
    for step, i in enumerate(order):
        spec = MIX_SPECS[i % len(MIX_SPECS)]
        groups = (1, 3, None)[int(rs.randint(0, 3))]
        if groups is None:
            monkeypatch.delenv(GROUPS_HOOK, raising=False)
        else:
            monkeypatch.setenv(GROUPS_HOOK, str(groups))
        _mix_equal(_mix_call(g, spec), _mix_want(spec), f"call {step}: {spec} groups={groups}")
    g.close()


# ------------------------------------------------------------------------------------------------
# sessions
# ------------------------------------------------------------------------------------------------
S_T, S_CAP, S_W = 16, 90, 5


def _session_pair(kind, d):
    g = Model(hparams(S_ITEMS, S_T, d, int(kind), LOSS_HINGE))
    o = OracleModel(g.hp)
    for which, v in random_params(kind, d, 1000 * int(kind) + d).items():
        g.set_param(which, v)
        o.set_param(which, v)
    return g, o


@pytest.mark.parametrize("kind,d", [(NORMAL, 32), (EWMA, 20)], ids=case_ids)
def test_sessions_on_poisoned_stores(poison, kind, d):
    """A store with remember = 5 created under poison; ragged appends over 40 shuffled slots of 90 (lengths 0 .. 12, so some named
    slots stay empty and 50 are never touched).  lengths, representations (the oracle's user_representation), seen (seen_expect);
    recommend with the seen items and the caller's lists excluded; audience with the seen lists inverted on the device (the pair
    sort) and the caller's lists; the state / set_state / set_seen round trip into a second poisoned store; replay()."""
    g, o = _session_pair(kind, d)
    rs = np.random.RandomState(50 + d)
    slots = rs.permutation(S_CAP)[:40].astype(np.uint32)
    hists = [rs.randint(0, 40 if i % 2 else S_ITEMS, size=i % 13).astype(np.uint32) for i in range(40)]
    st = g.sessions(S_CAP, remember=S_W)
    model = SeenModel(S_CAP, S_W)
    append_ragged(st, slots, hists, np.random.RandomState(d))
    model.append(slots, hists)
    everyone = np.arange(S_CAP, dtype=np.uint32)
    all_items = np.arange(S_ITEMS, dtype=np.uint32)
    told = {int(s): h for s, h in zip(slots, hists)}
    full = [told.get(s, np.zeros(0, np.uint32)) for s in range(S_CAP)]

    def check(store, lists, seen_model, what):
        """every slot of `store` holds the state of lists[slot] and the memory of seen_model"""
        assert store.lengths(everyone).tolist() == [len(x) for x in lists], what
        want_reps = np.array([o.user_representation(x) for x in lists], np.float32)
        assert np.array_equal(_bits(store.representations(everyone)), _bits(want_reps)), what
        seen = store.seen(everyone)
        want_seen = seen_model.seen(everyone)
        assert all(np.array_equal(a, b) for a, b in zip(seen, want_seen)), what
        scores = _rep_scores(o, S_ITEMS, want_reps)
        own = [rs.randint(0, S_ITEMS, s % 7).astype(np.uint32) for s in range(S_CAP)]
        both = seen_model.excluded(everyone, own)
        for k in (10, 1024):
            rows = [topk_expectation(scores[s], both[s], k) for s in range(S_CAP)]
            want = np.array([r[0] for r in rows], np.uint32), np.array([r[1] for r in rows], np.float32)
            _same_rows(store.recommend(everyone, k, exclude=own), want, f"{what}: recommend k={k}")
        live = np.array([s for s in range(S_CAP) if len(lists[s])], np.uint32)  # slots=None: the slots of length > 0, ascending
        queries = np.concatenate([np.arange(40), [S_ITEMS - 1, 3, 3]]).astype(np.uint32)
        tbits = _bits(np.ascontiguousarray(scores[live].T[queries]))
        qex = [rs.choice(live, size=j % 4, replace=False) for j in range(len(queries))]
        excluded = ae.unite(ae.seen_excluded(seen_model, live, queries), qex)
        assert any(len(x) for x in ae.seen_excluded(seen_model, live, queries))
        for k in (10, len(live) + 3):
            rows, score_bits = ae.expected_rows(tbits, live, k, excluded)
            got = store.audience(queries, k, exclude=qex)
            assert np.array_equal(got[0], rows) and np.array_equal(_bits(got[1]), score_bits), f"{what}: audience k={k}"
        return want_reps

    check(st, full, model, "appended")
    assert sum(1 for s in range(S_CAP) if not len(full[s])) >= 50
    # the checkpoint of every slot into a second store made under poison: never-told slots arrive, and read, as empty
    st2 = g.sessions(S_CAP, remember=S_W)
    h, cstate, n = st.state(slots)
    st2.set_state(slots, h, cstate, n)
    st2.set_seen(slots, st.seen(slots))
    check(st2, full, model, "restored")
    st2.close()
    # replay: every slot becomes what append of its memory makes of a fresh one
    live_memories = sum(1 for x in model.seen(everyone) if len(x))
    assert st.replay() == live_memories
    check(st, model.seen(everyone), model, "replayed")
    st.close()
    g.close()


# ------------------------------------------------------------------------------------------------
# training: whole fits against the oracle
# ------------------------------------------------------------------------------------------------
def _fit(kind, loss, d, items=150, users=60, T=20, B=64, opt=0, fusion=None, calls=1, data=None):
    """Two epochs (and `calls` fit calls) on `users` histories of up to T + 5 items (or on data = (ptr, items), which
    tests/test_guarded_scratch_gpu.py shapes to a step's row count) against the oracle: every parameter and accumulator bit for
    bit, the lagged loss figure, the reported loss to 1e-6 (an order-free f64 sum), mrr_score's ranks."""
    ptr, it = data if data is not None else synthetic_interactions(users, items, T + 5, seed=23, zipf=True)
    hp = hparams(items, T, d, int(kind), loss, B=B, epochs=2, opt=opt, lr=0.02 if opt else 0.16)
    g, o = parity.make_pair(hp)
    if fusion is not None:
        g.set_step_fusion(fusion)
    for call in range(calls):
        lg, lo = g.fit(ptr, it), o.fit(ptr, it)
        parity.assert_params_equal(g, o, kind, f"fit call {call}")
        if opt:
            for p in parity.ADAM_BLOCKS[kind]:
                parity.assert_same_bits(g.get_param(p), o.get_param(p), f"adam moment {p.name}")
        assert lg == pytest.approx(lo, rel=1e-6)
        parity.assert_lagged_equal(g, o, f"fit call {call}")
    mg, rg = g.mrr_score(ptr, it)
    mo, ro = o.mrr_score(ptr, it)
    assert np.array_equal(rg, ro) and mg == mo
    g.close()


def test_training_shapes_leave_pad_rows():
    """The rows a step of _fit's default shape packs are no multiple of SBR_DW_CHUNK_ROWS = 1 024: the last dense-gradient chunk has
    pad rows (a throwaway model: opening a plan draws from the model's generator)."""
    ptr, it = synthetic_interactions(60, 150, 25, seed=23, zipf=True)
    g = Model(hparams(150, 20, 64, int(NORMAL), LOSS_WARP, B=64, epochs=2))
    plan = g.fit_begin(ptr, it)
    rows = [plan.minibatch_rows(mb) for mb in range(plan.epoch_prepare())]
    plan.close()
    g.close()
    assert rows and all(r % 1024 for r in rows), rows


def test_training_ewma_hinge_d32(poison):
    _fit(EWMA, LOSS_HINGE, 32)


def test_training_lstm_warp_d64_full_tile_dw_on_the_address_path(poison):
    """d = 64: the full-tile dW kernel on 64-bit addresses — the path whose dZ pad rows are cleared by the launcher."""
    _fit(NORMAL, LOSS_WARP, 64, calls=2)


@pytest.mark.parametrize("wide", [False, True], ids=["buffer", "wide"])
def test_training_coupled_bpr_d128(poison, monkeypatch, wide):
    """d = 128 through buffer resources (the pad rows are out of range and read as zeros), and with SBR_DW_WIDE_ADDRESSES=1 on the
    address path."""
    if wide:
        monkeypatch.setenv("SBR_DW_WIDE_ADDRESSES", "1")
    _fit(COUPLED, LOSS_BPR, 128)


@pytest.mark.parametrize("kind,loss", [(NORMAL, LOSS_WARP), (EWMA, LOSS_BPR)], ids=case_ids)
def test_training_padded_width_d24(poison, kind, loss):
    _fit(kind, loss, 24)


@pytest.mark.parametrize("min_tiles", ["1", "1000000"])
def test_training_d256_both_bptt_forms(poison, monkeypatch, min_tiles):
    monkeypatch.setenv("SBR_BWD256_MIN_TILES", min_tiles)
    _fit(NORMAL, LOSS_WARP, 256, items=120, users=70, T=9, B=70)


@pytest.mark.parametrize("fusion", [2, 0])
@pytest.mark.parametrize("kind,loss", [(EWMA, LOSS_HINGE), (COUPLED, LOSS_BPR)], ids=case_ids)
def test_training_one_sequence_steps_d16(poison, kind, loss, fusion):
    _fit(kind, loss, 16, items=97, users=14, T=20, B=1, fusion=fusion, calls=2)


def test_training_adam(poison):
    _fit(NORMAL, LOSS_WARP, 64, B=9, opt=OPT_ADAM, calls=2)


def test_training_hot_rows_take_the_chunked_reduction(poison):
    parity.test_hot_rows_take_the_chunked_reduction(EWMA, LOSS_HINGE, 32, "single", 9, 0)


@pytest.mark.parametrize("exchange", ["owner", "gradient"])
def test_training_two_ranks_on_one_gpu(poison, exchange):
    parity.test_multi_device_halves_on_one_gpu(EWMA, LOSS_WARP, 32, 2, exchange)
