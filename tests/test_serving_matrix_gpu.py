"""GPU: every cell of tests/serving_matrix.py against the CPU oracle, bit for bit — ids, f32 score bits, keys, masses as integers,
counts, CSR pointers and padding — through the families' own expectation modules; nothing here restates a contract.  The matrix
is stored width (16, 32, 64, 128, 256, with embedding_dim = the width, and one padded dim per width: 9, 24, 48, 100, 200, where
the oracle never sees the padding columns, so parity shows they take no part) x score policy and filter x model kind.

One cell is one public call (or the few calls that share its kernels) on the smallest shape at which the kernels can go wrong:
130 rows (two row tiles, the second of two rows) over 229 items with SBR_CATALOGUE_GROUPS=3 (ranges of 96, 96 and 37 items: several
32-item tiles per range, a ragged last tile, a short last range), k = 10, thresholds and budgets that put a row's cut inside the
second range; the audience orientation is 130 query items over 229 candidate rows.  E = 0.3 randn and b = 0.1 randn through
set_param; items (31, 32) and (95, 96) are planted pairs with one row and one bias — across a tile edge and across a range edge —
and rows 0 and 1 point at them, so the tie goes to the lower id inside a top-10 at every width; candidate rows 31 / 32 and 95 / 96
are pairs in the same way.  Exclusion lists cycle through none, a few, and all but seven items (a padded row); tag masks cycle
through tests/test_filtered_gpu.py's seven kinds.  One model per (kind, dim), made once for the module."""
import functools

import numpy as np
import pytest

import audience_expect as ae
import serving_matrix as sm
from above_expect import above_expect, counts_expect
from beam_expect import beam_expect
from candidates_expect import AmongExpectation
from capped_expect import capped_rows, ranking
from diverse_expect import DiverseExpectation
from filter_expect import allowed as tag_allowed
from filter_expect import equivalent_exclusions
from helpers import LOSS_HINGE, hparams
from oracle.oracle import OracleModel
from partition_expect import frac_bits, partition_expect
from rank_expect import assert_ranks_equal, expect_all
from recommend_expect import NO_ITEM, topk_expectation
from rollout_expect import rollout_expect
from sampled_expect import sampled_expect
from sbr_rs_amd._abi import ModelKind, Param
from sbr_rs_amd.engine import NO_GROUP, Model
from seen_expect import SeenModel
from sequence_expect import csr, expect_sequence_ranks, oracle_score_fn, rows_of
from sequence_partition_expect import expect_sequence_partition, flat
from similar_expect import SimilarExpectation
from test_beam_gpu import _memo
from test_beam_gpu import _same as _same_beams
from test_filtered_gpu import ABSENT_BIT, ALL, FEW_BIT, _random_tags
from test_item_set_gpu import _same_above, _same_partition, _same_rows
from test_item_set_rollout_gpu import _same_rollout_expect
from test_sequence_partition_gpu import _assert_same as _same_sequence_partition
from test_sequence_ranks_gpu import _sequences
from test_sessions_gpu import append_ragged
from top_expect import top_expect

pytestmark = pytest.mark.gpu

ITEMS, ROWS, K = sm.ITEMS, sm.ROWS, sm.K
T, HIST, ROLL_STEPS, BEAM_STEPS, BEAM_W = 16, 6, 8, 3, 3  # a history of at most 6 items and 8 steps stay inside the oracle's window
TEMP, SEED = 0.7, 20261021
KIND = {sm.NORMAL: ModelKind.LSTM_NORMAL, sm.COUPLED: ModelKind.LSTM_COUPLED, sm.EWMA: ModelKind.EWMA}


@pytest.fixture(autouse=True)
def _groups(monkeypatch):
    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", str(sm.GROUPS))  # the scans read the hook per call


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _topk_rows(scores, excl, k):
    rows = [topk_expectation(scores[u], () if excl is None else excl[u], k) for u in range(len(scores))]
    return np.array([r[0] for r in rows], np.uint32).reshape(-1, k), np.array([r[1] for r in rows], np.float32).reshape(-1, k)


def _cycled_lists(rs, rows, columns):
    """one list per row: none, a few, all but seven (the row is padded), in turn"""
    out = []
    for u in range(rows):
        if u % 3 == 0:
            out.append(np.zeros(0, np.uint32))
        elif u % 3 == 1:
            out.append(rs.randint(0, columns, 5).astype(np.uint32))
        else:
            out.append(np.delete(np.arange(columns, dtype=np.uint32), rs.choice(columns, 7, replace=False)))
    return out


def _cycled_masks(rows):
    """tests/test_filtered_gpu.py's seven kinds of mask pair, row u has kind u % 7: none, any_of, none_of, both, a bit no item
    carries (a row of padding), none_of = all bits (the tag-0 items), and the pair that leaves the FEW_BIT items"""
    any_of, none_of = np.zeros(rows, np.uint32), np.zeros(rows, np.uint32)
    for i in range(rows):
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
    return any_of, none_of


class Case:
    """One (kind, dim): the engine model and the oracle with the same parameters, and everything the cells' expectations share —
    made once, read only."""

    def __init__(self, kind, dim):
        self.kind, self.dim = kind, dim
        rs = np.random.RandomState(1000 * int(kind) + dim)
        E = (rs.randn(ITEMS, dim) * 0.3).astype(np.float32)
        b = (rs.randn(ITEMS) * 0.1).astype(np.float32)
        for lo, hi in sm.TIES:
            E[hi], b[hi] = E[lo], b[lo]
        self.E, self.b = E, b
        hp = hparams(ITEMS, T, dim, int(kind), LOSS_HINGE, B=8)
        self.g, self.o = Model(hp), OracleModel(hp)
        ng = {ModelKind.LSTM_NORMAL: 4, ModelKind.LSTM_COUPLED: 3, ModelKind.EWMA: 0}[kind]
        params = {Param.ITEM_EMBEDDING: E, Param.ITEM_BIAS: b}
        if ng:
            params[Param.LSTM_W] = (rs.randn(2 * dim, ng * dim) * 0.3 / np.sqrt(dim / 16)).astype(np.float32)
            params[Param.LSTM_B] = (rs.randn(ng * dim) * 0.5).astype(np.float32)
        else:
            params[Param.EWMA_ALPHA] = rs.randn(dim).astype(np.float32)
        for m in (self.g, self.o):
            for which, v in params.items():
                m.set_param(which, np.ascontiguousarray(v).ravel())
        # the item side: 229 rows (the audience's candidates), the first 130 of them the rows of every other call
        R = (rs.randn(ITEMS, dim) * 0.5).astype(np.float32)
        R[0], R[1] = E[sm.TIES[0][0]] * np.float32(4.0), E[sm.TIES[1][0]] * np.float32(4.0)  # the planted pairs lead rows 0 and 1
        for lo, hi in sm.TIES:
            R[hi] = R[lo]
        self.R, self.reps = R, R[:ROWS]
        self.tags = _random_tags(ITEMS, dim)
        self.tags[7::50] = 1 << FEW_BIT
        self.any_of, self.none_of = _cycled_masks(ROWS)
        self.excl = _cycled_lists(rs, ROWS, ITEMS)
        self.queries = rs.permutation(ITEMS)[:ROWS].astype(np.uint32)
        self.queries[:4] = (31, 32, 95, 96)
        self.qexcl = _cycled_lists(rs, ROWS, ITEMS)  # candidate rows left out of a query's audience
        self.groups = rs.randint(0, 8, ITEMS).astype(np.uint32)
        self.groups[rs.rand(ITEMS) < 0.1] = NO_GROUP
        self.S = np.array([i for i in range(ITEMS) if i % 3], np.uint32)  # an item set with 95 and without its twin 96
        self.outside = np.setdiff1d(np.arange(ITEMS, dtype=np.uint32), self.S)
        self.g.set_item_tags(self.tags)
        self.g.set_item_groups(self.groups)
        # the recurrent side: 130 histories of 0 .. 6 items behind slots that are not the rows' indices
        self.hists = [rs.randint(0, ITEMS, u % (HIST + 1)).astype(np.uint32) for u in range(ROWS)]
        self.slots = np.arange(ROWS, dtype=np.uint32) * 2 + 1
        self.hexcl = _cycled_lists(rs, ROWS, ITEMS)
        self.hexcl[1] = np.arange(ITEMS, dtype=np.uint32)  # may see nothing: ends at step 0
        self.rep, self.scores_of = _memo(self.o, ITEMS)
        self._closing = []

    # ---- shared expectations ----------------------------------------------------------------------------------------------
    @functools.cached_property
    def all_scores(self):
        """the oracle's score of every (candidate row, item): [229, 229]"""
        items = np.arange(ITEMS, dtype=np.uint32)
        s = np.array([self.o.predict(r, items) for r in self.R], np.float32).reshape(ITEMS, ITEMS)
        top = _topk_rows(s[:2], None, K)[0]
        assert set(sm.TIES[0]) <= set(top[0].tolist()) and set(sm.TIES[1]) <= set(top[1].tolist()), "the planted pairs are inside a top-10"
        s.setflags(write=False)
        return s

    @property
    def scores(self):
        return self.all_scores[:ROWS]

    @functools.cached_property
    def tscores(self):
        """[130 queries, 229 candidates]"""
        return np.ascontiguousarray(self.all_scores.T[self.queries])

    def lists(self, filtered, excl=None, rows=ROWS):
        """the rows' exclusion lists, with the items their mask pair bars appended under a filter"""
        excl = self.excl if excl is None else excl
        return equivalent_exclusions(self.tags, self.any_of[:rows], self.none_of[:rows], rows, excl) if filtered else excl

    def masks(self, filtered, rows=ROWS):
        return dict(any_of=self.any_of[:rows], none_of=self.none_of[:rows]) if filtered else {}

    def allowed(self, filtered):
        return np.array([tag_allowed(self.tags, a, n) for a, n in zip(self.any_of, self.none_of)]) if filtered else None

    @functools.cached_property
    def item_set(self):
        return self.g.item_set(self.S[::-1])

    def joined(self, lists):
        return [np.concatenate([np.asarray(x, np.uint32), self.outside]) for x in lists]

    @functools.cached_property
    def store(self):
        """the 130 histories in a store without memory"""
        st = self.g.sessions(2 * ROWS + 5)
        st.append(self.slots, self.hists)
        self._closing.append(st)
        return st

    def close(self):
        for st in self._closing:
            st.close()
        self.g.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(cell):
        key = (cell.kind, cell.dim)
        if key not in made:
            made[key] = Case(KIND[cell.kind], cell.dim)
        return made[key]

    yield get
    for c in made.values():
        c.close()


# ------------------------------------------------------------------------------------------------
# the catalogue calls
# ------------------------------------------------------------------------------------------------
def run_recommend(c, f):
    _same_rows(c.g.recommend_reps(c.reps, K, exclude=c.excl, **c.masks(f)), _topk_rows(c.scores, c.lists(f), K), "recommend_reps")


def _similar(c, f, metric):
    want = SimilarExpectation(c.E, metric)
    qex = c.lists(f, [x[:40] for x in c.excl])  # the queries' own lists: none, a few, forty
    got = c.g.similar_items(c.queries, K, metric=metric, exclude=[x[:40] for x in c.excl], **c.masks(f))
    _same_rows(got, want.rows(c.queries, K, False, qex), f"similar_items {metric}")
    got = c.g.similar_items(c.queries[:8], K, metric=metric, include_self=True, **c.masks(f, 8))
    _same_rows(got, want.rows(c.queries[:8], K, True, c.lists(f, [()] * 8, 8)), f"similar_items {metric} include_self")
    if not f:
        assert got[0][0, :2].tolist() == [31, 32], "the planted twin follows its query: the tie goes to the lower id"


def run_similar_cosine(c, f):
    _similar(c, f, "cosine")


def run_similar_dot(c, f):
    _similar(c, f, "dot")


def run_audience(c, f):
    rows, bits = ae.expected_rows(_bits(c.tscores), np.arange(ITEMS, dtype=np.uint32), K, c.qexcl)
    got = c.g.audience_reps(c.R, c.queries, K, exclude=c.qexcl)
    assert np.array_equal(got[0], rows) and np.array_equal(_bits(got[1]), bits)
    assert np.any(rows == ae.NO_ROW) and np.any(np.diff(rows.astype(np.int64), axis=1)[bits[:, 1:] == bits[:, :-1]] > 0)  # padding; a tie


def run_sampled(c, f):
    got = c.g.recommend_sampled_reps(c.reps, K, temperature=TEMP, seed=SEED, exclude=c.excl, **c.masks(f))
    _same_rows(got, sampled_expect(c.scores, c.lists(f), K, TEMP, SEED), "recommend_sampled_reps")


def run_set_sampled(c, f):
    streams = (np.arange(ROWS, dtype=np.uint64) * 977 + 13) % 311
    got = c.item_set.recommend_sampled_reps(c.reps, K, temperature=TEMP, seed=SEED, streams=streams, exclude=c.excl, **c.masks(f))
    _same_rows(got, sampled_expect(c.scores, c.joined(c.lists(f)), K, TEMP, SEED, streams), "sampled through the item set")
    assert np.all(np.isin(got[0][got[0] != NO_ITEM], c.S))


def run_log_partition(c, f):
    got = c.g.log_partition_reps(c.reps, TEMP, exclude=c.excl, **c.masks(f))
    kw = dict(tags=c.tags, any_of=c.any_of, none_of=c.none_of) if f else {}
    _same_partition(got, partition_expect(c.scores, c.excl, TEMP, **kw), "log_partition_reps")
    assert got.frac_bits == frac_bits(ITEMS)
    _same_partition(c.g.log_partition_reps(c.reps, TEMP, **c.masks(f)), partition_expect(c.scores, None, TEMP, **kw), "no lists: no finish")


def _thresholds(scores):
    """about 126 of 229 columns pass: a row's count runs past its first range and ends inside the second"""
    return np.quantile(scores, 0.45, axis=1).astype(np.float32)


def run_above(c, f):
    th = _thresholds(c.scores)
    for order in ("score", "id"):
        got = c.g.recommend_above_reps(c.reps, th, exclude=c.excl, order=order, **c.masks(f))
        _same_above(got, above_expect(c.scores, th, c.excl, c.allowed(f), order), f"recommend_above_reps {order}")
    want = counts_expect(c.scores, th, c.excl, c.allowed(f))
    assert np.array_equal(c.g.count_above_reps(c.reps, th, exclude=c.excl, **c.masks(f)), want)
    if not f:  # the rows without a list: more than the first range holds, fewer than the first two
        assert ((want[::3] > 96) & (want[::3] <= 192)).all()


def run_audience_above(c, f):
    th = _thresholds(c.tscores)
    ids = np.arange(ITEMS, dtype=np.uint32)
    for order in ("score", "id"):
        got = c.g.audience_above_reps(c.R, c.queries, th, exclude=c.qexcl, order=order)
        _same_above(got, above_expect(c.tscores, th, c.qexcl, None, order, ids), f"audience_above_reps {order}")
    assert np.array_equal(c.g.count_audience_above_reps(c.R, c.queries, th, exclude=c.qexcl), counts_expect(c.tscores, th, c.qexcl))


def _budgets(rows):
    """100 .. 159: past the first range's 96 items, inside the second's"""
    return (100 + np.arange(rows) % 60).astype(np.uint64)


def run_top(c, f):
    n = _budgets(ROWS)
    for order in ("score", "id"):
        got = c.g.recommend_top_reps(c.reps, n, exclude=c.excl, order=order, **c.masks(f))
        _same_above(got, top_expect(c.scores, n, c.excl, c.allowed(f), order), f"recommend_top_reps {order}", cuts=True)
    cuts, counts = c.g.nth_score_reps(c.reps, n, exclude=c.excl, **c.masks(f))
    want = top_expect(c.scores, n, c.excl, c.allowed(f))
    assert np.array_equal(_bits(cuts), _bits(want[3])) and np.array_equal(counts, np.diff(want[0]))


def run_audience_top(c, f):
    n = _budgets(ROWS)
    ids = np.arange(ITEMS, dtype=np.uint32)
    for order in ("score", "id"):
        got = c.g.audience_top_reps(c.R, c.queries, n, exclude=c.qexcl, order=order)
        _same_above(got, top_expect(c.tscores, n, c.qexcl, None, order, ids), f"audience_top_reps {order}", cuts=True)


def run_capped(c, f):
    cap, pool = 1, 16
    allowed = c.allowed(f)
    ranks = [ranking(c.scores[u], c.excl[u], None if allowed is None else allowed[u]) for u in range(ROWS)]
    device = capped_rows(ranks, c.groups, cap, K, pool)
    assert not device[2].all() and device[2].any()  # the pool leaves some rows short
    _same_rows(c.g.recommend_capped_reps(c.reps, K, cap, pool, exclude=c.excl, exact=False, **c.masks(f)), device, "the device's rows")
    _same_rows(c.g.recommend_capped_reps(c.reps, K, cap, pool, exclude=c.excl, **c.masks(f)), capped_rows(ranks, c.groups, cap, K), "exact")


def run_diverse(c, f):
    pool = 40
    for metric in ("cosine", "dot"):
        got = c.g.recommend_diverse_reps(c.reps, K, pool, 0.5, metric, exclude=c.excl)
        _same_rows(got, DiverseExpectation(c.E, metric).rows(_topk_rows(c.scores, c.excl, pool), K, 0.5), f"recommend_diverse_reps {metric}")


def run_candidates(c, f):
    rs = np.random.RandomState(c.dim)
    cands = [rs.randint(0, ITEMS, u % 37).astype(np.uint32) for u in range(ROWS)]
    cands[2] = np.arange(ITEMS, dtype=np.uint32)
    cptr, cit = csr(cands)
    got = c.g.score_candidates_reps(c.reps, cptr, cit)
    assert len(got) == ROWS
    for u in range(ROWS):
        assert np.array_equal(_bits(got[u]), _bits(c.scores[u][cands[u]])), u
    for u in (0, 31, ROWS - 1):
        assert np.array_equal(_bits(c.g.predict(c.reps[u], cands[2])), _bits(c.scores[u])), u


def run_among(c, f):
    want = AmongExpectation(c.o, ITEMS, c.reps)
    for k in (K, c.S.size + 3):
        _same_rows(c.g.recommend_among_reps(c.reps, k, c.S[::-1], exclude=c.excl), want.rows(c.S, k, c.excl), f"recommend_among_reps k={k}")


def run_rank_targets(c, f):
    rs = np.random.RandomState(c.dim + 1)
    targets = [rs.randint(0, ITEMS, u % 21).astype(np.uint32) for u in range(ROWS)]  # past a scan row's 16 (8 at width 256) thresholds
    targets[4][:4] = (31, 32, 95, 96)
    tptr, tit = csr(targets)
    want = np.concatenate(expect_all(c.scores, c.excl, targets))
    assert np.array_equal(c.g.rank_targets_reps(c.reps, tptr, tit, exclude=c.excl), want)


# ------------------------------------------------------------------------------------------------
# everything with a recurrent cell in it
# ------------------------------------------------------------------------------------------------
def _rep_rows(c, lists):
    return np.array([c.o.user_representation(np.asarray(x, np.uint32)) for x in lists], np.float32).reshape(len(lists), c.dim)


def run_append(c, f):
    """ragged appends (every split of a history, slots listed with nothing, slots never told) and all at once"""
    want = _rep_rows(c, c.hists)
    st = c.g.sessions(2 * ROWS + 5)
    append_ragged(st, c.slots, c.hists, np.random.RandomState(c.dim))
    assert np.array_equal(_bits(st.representations(c.slots)), _bits(want)), "ragged"
    assert st.lengths(c.slots).tolist() == [len(h) for h in c.hists]
    assert not st.lengths(c.slots - 1).any()
    st.close()
    assert np.array_equal(_bits(c.store.representations(c.slots)), _bits(want)), "at once"
    assert np.array_equal(_bits(c.g.user_representations(*csr(c.hists))), _bits(want)), "user_representations"


def _store_with_memory(c, w, hists):
    st = c.g.sessions(2 * ROWS + 5, remember=w)
    seen = SeenModel(2 * ROWS + 5, w)
    st.append(c.slots, hists)
    seen.append(c.slots, hists)
    return st, seen


def _recommend_with_memory(c, st, seen, reps):
    items = np.arange(ITEMS, dtype=np.uint32)
    scores = np.array([c.o.predict(r, items) for r in reps], np.float32).reshape(ROWS, ITEMS)
    _same_rows(st.recommend(c.slots, K, exclude=c.excl), _topk_rows(scores, seen.excluded(c.slots, c.excl), K), "recommend, memory and lists")
    return scores


def run_replay(c, f):
    """a memory of 5 behind histories of up to 6: the ring wraps; replay leaves what append of the memory makes of a fresh slot"""
    st, seen = _store_with_memory(c, 5, c.hists)
    memories = seen.seen(c.slots)
    assert st.replay() == sum(1 for x in memories if len(x))
    want = _rep_rows(c, memories)
    assert np.array_equal(_bits(st.representations(c.slots)), _bits(want))
    assert st.lengths(c.slots).tolist() == [len(x) for x in memories]
    scores = _recommend_with_memory(c, st, seen, want)
    live = np.array([s for s, x in zip(c.slots, memories) if len(x)], np.uint32)  # slots=None: the slots of length > 0, ascending
    at = np.flatnonzero(np.isin(c.slots, live))
    tbits = _bits(np.ascontiguousarray(scores[at].T[c.queries]))
    rs = np.random.RandomState(c.dim + 2)
    qex = [rs.choice(live, size=j % 4, replace=False) for j in range(ROWS)]
    held = ae.seen_excluded(seen, live, c.queries)
    assert any(len(x) for x in held)
    rows, bits = ae.expected_rows(tbits, live, K, ae.unite(held, qex))
    got = st.audience(c.queries, K, exclude=qex)
    assert np.array_equal(got[0], rows) and np.array_equal(_bits(got[1]), bits)
    st.close()


def run_seen_wide(c, f):
    st, seen = _store_with_memory(c, 100, c.hists)
    _recommend_with_memory(c, st, seen, _rep_rows(c, c.hists))
    st.close()


def _rollouts(c, on, lists):
    for mode, sample in (("greedy", None), ("sample", (TEMP, SEED))):
        r = on.rollout(c.slots, ROLL_STEPS, mode=mode, temperature=TEMP, seed=SEED, exclude=c.hexcl, log_prob=True)
        e = rollout_expect(c.rep, c.scores_of, ITEMS, c.hists, ROLL_STEPS, lists, partition_temperature=TEMP, sample=sample, streams=c.slots)
        _same_rollout_expect(r, e, mode)
        assert e.lengths[1] == 0 and e.lengths.max() == ROLL_STEPS and ROLL_STEPS > e.lengths[2] > 0  # nothing; a full row; a padded one
        assert r.frac_bits == frac_bits(ITEMS)


def run_rollout(c, f):
    _rollouts(c, c.store, c.hexcl)


def run_set_rollout(c, f):
    _rollouts(c, c.item_set.on(c.store), c.joined(c.hexcl))


def _beams(c, on, lists):
    r = on.beam_search(c.slots, BEAM_STEPS, width=BEAM_W, temperature=TEMP, exclude=c.hexcl, partitions=True)
    e = beam_expect(c.rep, c.scores_of, ITEMS, c.hists, BEAM_STEPS, BEAM_W, TEMP, lists)
    _same_beams(r, e, "beam_search")
    assert e.beams[1] == 0 and e.beams.max() == BEAM_W and r.frac_bits == frac_bits(ITEMS)


def run_beam(c, f):
    _beams(c, c.store, c.hexcl)


def run_set_beam(c, f):
    _beams(c, c.item_set.on(c.store), c.joined(c.hexcl))


def run_sequences(c, f):
    """mrr_score, sequence_ranks and sequence_partition (what sequence_log_probs reads) over sequences of 0 .. T + 5 items"""
    seqs = _sequences(ROWS, ITEMS, T, seed=c.dim)
    ptr, it = csr(seqs)
    mg, rg = c.g.mrr_score(ptr, it)
    mo, ro = c.o.mrr_score(ptr, it)
    assert np.array_equal(rg, ro) and mg == mo
    fn = oracle_score_fn(c.o, ITEMS)
    for mask in (True, False):
        p, r = c.g.sequence_ranks(ptr, it, include_history=not mask)
        assert_ranks_equal(rows_of(p, r), expect_sequence_ranks(fn, seqs, T, mask_history=mask), f"sequence_ranks mask={mask}")
    p, part, scores, masked = c.g.sequence_partition(ptr, it, temperature=TEMP)
    want = flat(expect_sequence_partition(fn, seqs, T, TEMP, mask_history=True))
    _same_sequence_partition((part.shift.view(np.uint32), part.mass, scores.view(np.uint32), masked), want, "sequence_partition")
    assert p[-1] == want[0].size and part.frac_bits == frac_bits(ITEMS)


RUN = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("run_")}


def test_every_call_of_the_table_has_a_runner():
    assert {c.call for c in sm.CELLS} == set(RUN)


@pytest.mark.parametrize("cell", sm.CELLS, ids=sm.cell_id)
def test_cell(cases, cell):
    RUN[cell.call](cases(cell), cell.filtered)
