"""GPU: sbr_rank_targets / sbr_rank_targets_reps (exact ranks of many held-out items per user from one catalogue scan,
sbr_catalogue.hip: rank_targets_prepare_kernel, rank_targets_gemm_kernel, rank_targets_finish_kernel).

Expectation everywhere: per-item scores (the oracle's user_representation + predict over every item, or designed scores that
are exact in f32), the history masked to f32::MIN, a numpy `>=` count (rank_expect.py).  Ranks are integers and are compared
with np.array_equal; nothing here has a tolerance.  The number of item ranges is forced with SBR_CATALOGUE_GROUPS as in
test_catalogue_gpu.py, whose shapes and helpers the tests reuse."""
import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams, movielens_protocol, synthetic_interactions
from oracle.oracle import OracleModel
from rank_expect import F32_MIN, assert_ranks_equal, expect_all, oracle_scores, ranks_expectation
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, PredictionError
from sbr_rs_amd.evaluation import holdout_split, mrr_ranks, rank_targets, ranking_metrics
from test_catalogue_gpu import (KINDS, LONG_ITEMS, LONG_T, LONG_USERS, S, _design, _designed_model, _designed_scores, _force,
                                _heavy_tie_params, _histories, _long_case, _pair, _range_len, _reps)

pytestmark = pytest.mark.gpu

TMAX = 16  # thresholds per scan-user at d <= 128 (8 at d = 256): users with more targets are split by the host


def _csr(seqs):
    ptr = np.zeros(len(seqs) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(s) for s in seqs])
    it = np.concatenate([np.asarray(s, np.uint32) for s in seqs] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return ptr, it


def _split(flat, seqs):
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return [flat[ptr[u]: ptr[u + 1]] for u in range(len(seqs))]


def _model(hp, E, bias):
    g = Model(hp)
    g.set_param(Param.ITEM_EMBEDDING, E)
    g.set_param(Param.ITEM_BIAS, bias)
    return g


# ------------------------------------------------------------------------------------------------
# 1. oracle parity: long ranges, heavy ties
# ------------------------------------------------------------------------------------------------
def _long_targets(hists, scores):
    """Per user 0, 1, 5, TMAX, TMAX + 1 or 40 random targets; every user with targets also gets a duplicate, its best and worst
    item (by masked score), three items of its largest tie class, and — with a history — the last history item and the first
    one (outside the last LONG_T items where the history is longer)."""
    rs = np.random.RandomState(17)
    targets = []
    for u, h in enumerate(hists):
        n = (0, 1, 5, TMAX, TMAX + 1, 40)[u % 6]
        if u in (127, 128) or len(h) == 0:  # both sides of the 128-user tile edge; the empty histories
            n = max(n, 3)
        t = rs.randint(0, LONG_ITEMS, n).tolist()
        if n:
            m = scores[u].copy()
            m[np.unique(h).astype(np.int64)] = F32_MIN
            vals, inv, cnt = np.unique(scores[u], return_inverse=True, return_counts=True)
            tie_class = np.flatnonzero(inv == np.argmax(cnt))
            t += [t[0], int(np.argmax(m)), int(np.argmin(scores[u]))] + tie_class[:3].tolist()
            if len(h):
                t += [int(h[-1]), int(h[0])]
        targets.append(np.array(t, np.uint32))
    return targets


@pytest.mark.parametrize("groups", [None, 1, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 16, 64, 100, 128, 256])
def test_rank_targets_matches_oracle(monkeypatch, groups, kind, d):
    """5 007 items, 130 users (the second user tile holds two), heavy ties, every width class; forced to 1 range (157 tiles per
    workgroup), to 3, and the split of the day.  Between 0 and 48 targets per user (more than TMAX: several scan-users that share
    a representation row) with duplicates, targets inside the history and inside it but outside the state window, the best and
    the worst item, items of the largest tie class, a user with an empty history.  History masked and included."""
    _force(monkeypatch, groups)
    hp, E, bias, ptr, it, hists, scores = _long_case(kind, d)
    if groups is not None:
        per = _range_len(LONG_ITEMS, groups)
        assert per >= 3 * 32 and (LONG_ITEMS + per - 1) // per == groups
    targets = _long_targets(hists, scores)
    sizes = [len(t) for t in targets]
    assert min(sizes) == 0 and max(sizes) > 2 * TMAX and len(targets) == LONG_USERS
    assert any(len(h) == 0 and len(t) for h, t in zip(hists, targets)), "a user with an empty history and targets"
    assert any(len(h) > LONG_T and len(t) and h[0] not in h[-LONG_T:] for h, t in zip(hists, targets)), "a target outside the window"
    assert len(targets[127]) and len(targets[128])
    _, cnt = np.unique(scores[0], return_counts=True)
    assert cnt.max() >= 200  # heavy ties
    g = _model(hp, E, bias)
    tp, ti = _csr(targets)
    got = _split(g.rank_targets(ptr, it, tp, ti), targets)
    want = expect_all(scores, hists, targets, mask_history=True)
    assert_ranks_equal(got, want, "masked")
    assert any(LONG_ITEMS in w.tolist() for w in want)
    got = _split(g.rank_targets(ptr, it, tp, ti, include_history=True), targets)
    assert_ranks_equal(got, expect_all(scores, hists, targets, mask_history=False), "history included")


# ------------------------------------------------------------------------------------------------
# 2. holdout = 1 is mrr_score's rank
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [None, 1])
@pytest.mark.parametrize("kind,d", [(ModelKind.LSTM_NORMAL, 64), (ModelKind.EWMA, 128), (ModelKind.LSTM_COUPLED, 256)])
def test_holdout_one_equals_mrr_ranks(monkeypatch, groups, kind, d):
    _force(monkeypatch, groups)
    hp, E, bias, ptr, it, hists, _scores = _long_case(kind, d)
    g = _model(hp, E, bias)
    _mrr, want = g.mrr_score(ptr, it)
    ranked = [h for h in hists if len(h) >= 2]
    assert len(ranked) == want.size > 100
    hp_, hi = _csr([h[:-1] for h in ranked])
    tp, ti = _csr([h[-1:] for h in ranked])
    assert np.array_equal(g.rank_targets(hp_, hi, tp, ti), want)


def test_holdout_one_equals_mrr_ranks_movielens():
    """The MovieLens fixture after the two-epoch fit of test_recommend_cpp.py: ranking_metrics' split at holdout = 1 ranks the
    users mrr_score ranks and gives its ranks; the metrics' MRR is the mean of 1 / rank in float64."""
    import sbr_rs_amd as sbr

    data, train, test, rng = movielens_protocol()
    model = (sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).learning_rate(0.16).l2_penalty(0.0004)
             .loss(sbr.Loss.WARP).num_epochs(2).batch_sequences(8).rng(rng).build())
    model.fit(train)
    _mrr, want = mrr_ranks(model, test)
    users, hists, targets = holdout_split(test, 1)
    got = rank_targets(model, hists, targets)
    assert len(got) == want.size and np.array_equal(np.concatenate(got), want)
    m = ranking_metrics(model, test, ks=(10, 100), holdout=1)
    assert m["num_users_ranked"] == want.size and np.array_equal(m["users"], users)
    assert m["mrr"] == float(np.mean(1.0 / want.astype(np.float64)))
    assert m["recall"][10] == m["hit_rate"][10] == float(np.mean(want <= 10))
    assert np.array_equal(np.concatenate(model.rank_targets(hists, targets)), want)


# ------------------------------------------------------------------------------------------------
# 3. designed exact scores through rank_targets_reps
# ------------------------------------------------------------------------------------------------
DES_ITEMS, DES_USERS = 200_000, 300


@pytest.mark.parametrize("groups", [1, None])
@pytest.mark.parametrize("name", ["equal", "ascending", "descending", "sawtooth", "flips"])
def test_rank_targets_designed_scores(monkeypatch, groups, name):
    """300 users x 200 000 items, d = 16, scores that are exact in f32 whatever the order of operations: all equal (every rank
    = num_items), ascending and descending in the id (rank = distance to one end), a sawtooth of period 33 (ties that straddle
    the 32-item tiles and the range borders), per-user sign flips (the lanes of one wave want opposite ends; one bias-only user).
    Forced to 1 range (6 250 tiles per workgroup) and the split of the day.  Targets at the tile and range borders, both ends and
    random ids, 0 to 20 per user; expectation in float64 numpy."""
    _force(monkeypatch, groups)
    x, y, b = _design(name)
    g = _designed_model(y, b)
    rs = np.random.RandomState(len(name))
    per = _range_len(DES_ITEMS, 72)
    fixed = [0, 31, 32, 33, 63, 64, 159, 160, 161, per - 1, per, per + 1, DES_ITEMS // 2, DES_ITEMS - 33, DES_ITEMS - 1]
    targets = [np.array((fixed + rs.randint(0, DES_ITEMS, 8).tolist())[: (u * 5) % 21], np.uint32) for u in range(DES_USERS)]
    assert min(len(t) for t in targets) == 0 and max(len(t) for t in targets) == 20 > TMAX
    cache, want = {}, []
    for u in range(DES_USERS):
        key = float(x[u])
        if key not in cache:
            cache[key] = _designed_scores(x[u], y, b).astype(np.float64)
        s = cache[key]
        want.append(np.array([np.count_nonzero(s >= s[t]) for t in targets[u]], np.uint32))
    tp, ti = _csr(targets)
    got = _split(g.rank_targets_reps(_reps(x), tp, ti), targets)
    assert_ranks_equal(got, want, name)
    if name == "equal":
        assert all((w == DES_ITEMS).all() for w in want)
    if name == "ascending":
        assert want[20].tolist()[:2] == [DES_ITEMS, DES_ITEMS - 31]


# ------------------------------------------------------------------------------------------------
# 4. agreement with recommend
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.EWMA])
def test_rank_targets_agrees_with_recommend(kind):
    """For a target outside the history whose score no other unmasked item shares: rank <= k puts it at position rank - 1 of
    recommend(k)'s row, rank > k leaves it out.  A target inside the history has rank num_items and is not recommended.  Targets
    whose score is shared are left out of the position check: at most 1 % of them (asserted)."""
    items, T, d, k, holdout = 3001, 12, 32, 100, 5
    rs = np.random.RandomState(11)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    bias = (rs.randn(items) * 0.1).astype(np.float32)
    g, o = _pair(items, T, d, kind, E, bias)
    ptr, it = synthetic_interactions(200, items, 30, seed=3, min_len=6)
    seqs = _histories(ptr, it)
    hists, targets = [s[:-holdout] for s in seqs], [s[-holdout:] for s in seqs]
    scores = oracle_scores(o, items, hists)
    hp_, hi = _csr(hists)
    tp, ti = _csr(targets)
    ranks = _split(g.rank_targets(hp_, hi, tp, ti), targets)
    rec_items, _rec_scores = g.recommend(hp_, hi, k)
    total = shared = checked_in = checked_out = 0
    for u in range(len(seqs)):
        hset = set(hists[u].tolist())
        m = scores[u].copy()
        m[np.unique(hists[u]).astype(np.int64)] = F32_MIN
        row = rec_items[u].tolist()
        for t, r in zip(targets[u].tolist(), ranks[u].tolist()):
            total += 1
            if t in hset:
                assert r == items and t not in row
                continue
            if np.count_nonzero(m == m[t]) > 1:
                shared += 1
                continue
            if r <= k:
                assert row[r - 1] == t, (u, t, r)
                checked_in += 1
            else:
                assert t not in row, (u, t, r)
                checked_out += 1
    assert total == 1000 and shared <= 0.01 * total, (shared, total)
    assert checked_in > 0 and checked_out > 0


# ------------------------------------------------------------------------------------------------
# 5. counter width
# ------------------------------------------------------------------------------------------------
def test_rank_targets_counter_width(monkeypatch):
    """rank_targets_gemm_kernel counts the scores that reach a scan-user's lowest threshold in 16-bit lane counters, two per
    register, as rank_gemm_kernel does (test_mrr_counter_width), so launch_rank_targets may give a range at most 65 535 tiles;
    its LDS buckets are 32 bits wide.  Forced to 1 range, 65 535 * 32 + 33 = 2 097 153 items must still be cut in two (65 535
    tiles + 2), and with every item scoring at or above the lowest threshold every lane of the first range counts to exactly
    65 535: one more and it would carry into its neighbour.  The scores above the second lowest threshold land, all but three, in ONE
    bucket per user, which a workgroup counts to 2 097 120 in one LDS word.  d = 16, EWMA, E = 0, bias 1 everywhere but 0 at
    three items; ranks up to and equal to num_items."""
    _force(monkeypatch, 1)
    items, d, T = 65535 * 32 + 33, 16, 4
    E = np.zeros((items, d), np.float32)
    bias = np.ones(items, np.float32)
    low = [5, 1_000_000, items - 1]
    bias[low] = 0.0
    g = _model(hparams(items, T, d, int(ModelKind.EWMA), LOSS_HINGE, B=8), E, bias)
    hists = [np.array(h, np.uint32) for h in ([9, 70_000, 9], [3], [], [9, 70_000, 9, 5])]
    targets = [np.array(t, np.uint32) for t in ([5, 7, 9], low, low + [0], [5, 1_000_000])]
    tp, ti = _csr(targets)
    hp_, hi = _csr(hists)
    want = [ranks_expectation(bias, np.unique(h), t) for h, t in zip(hists, targets)]
    assert want[0].tolist() == [items - 2, items - 5, items] and want[2].tolist() == [items, items, items, items - 3]
    assert want[3].tolist() == [items, items - 3]
    assert_ranks_equal(_split(g.rank_targets(hp_, hi, tp, ti), targets), want, "masked")
    want = [ranks_expectation(bias, (), t) for t in targets]
    assert want[0].tolist() == [items, items - 3, items - 3]
    assert_ranks_equal(_split(g.rank_targets(hp_, hi, tp, ti, include_history=True), targets), want, "included")


# ------------------------------------------------------------------------------------------------
# 6. the host's chunking
# ------------------------------------------------------------------------------------------------
def test_rank_targets_two_chunks_split_user_at_the_border():
    """A launch holds at most 8 192 scan-users.  10 500 users of whom every 7th has no targets; the others have one target each,
    except the user whose first scan-user is number 8 190: it has 40 targets = three scan-users, two at the end of the first
    launch and one at the start of the second (which re-forwards its history and writes out_ranks from c0 != 0 on).  600 items,
    EWMA, d = 16; every rank against the oracle."""
    users, items, d, T = 10500, 600, 16, 8
    E, bias = _heavy_tie_params(items, d, 61)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(users, items, 2 * T, seed=62, min_len=0)
    hists = _histories(ptr, it)
    rs = np.random.RandomState(63)
    targets, scan_users, big = [], 0, None
    for u in range(users):
        if u % 7 == 0:
            targets.append(np.zeros(0, np.uint32))
            continue
        if scan_users == 8190 and big is None:
            big = u
            targets.append(rs.randint(0, items, 40).astype(np.uint32))
            scan_users += 3
            continue
        targets.append(rs.randint(0, items, 1).astype(np.uint32))
        scan_users += 1
    assert big is not None and scan_users > 8192 + 500 and len(hists[big]) > 0
    scores = oracle_scores(o, items, hists)
    tp, ti = _csr(targets)
    got = _split(g.rank_targets(ptr, it, tp, ti), targets)
    assert_ranks_equal(got, expect_all(scores, hists, targets), "two chunks")
    assert len(np.unique(np.concatenate(got[big + 1:]))) > 20
    # the same through rank_targets_reps, which cuts at the same scan-user
    reps = np.array([o.user_representation(h) for h in hists], np.float32)
    got = _split(g.rank_targets_reps(reps, tp, ti, exclude=hists), targets)
    assert_ranks_equal(got, expect_all(scores, hists, targets), "two chunks, reps")


def test_rank_targets_chunks_by_forward_rows():
    """A launch is also cut at 2^22 forward rows: T = 600 and 7 100 users with histories of 600..619 items are 4.26 M rows, two
    launches of fewer than 8 192 scan-users.  EWMA, d = 16, 300 items, one or two targets per user."""
    users, items, d, T = 7100, 300, 16, 600
    E, bias = _heavy_tie_params(items, d, 51)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(users, items, T + 20, seed=52, min_len=T + 1)
    assert users * T > 2 ** 22 and users < 8192
    seqs = _histories(ptr, it)
    hists = [s[:-1] for s in seqs]
    targets = [np.array([s[-1], (u * 13) % items][: 1 + u % 2], np.uint32) for u, s in enumerate(seqs)]
    scores = oracle_scores(o, items, hists)
    got = rank_targets(g, hists, targets)
    assert_ranks_equal(got, expect_all(scores, hists, targets), "forward rows")
    _mrr, mr = g.mrr_score(ptr, it)
    assert np.array_equal(np.array([r[0] for r in got], np.uint32), mr)


# ------------------------------------------------------------------------------------------------
# 7. errors
# ------------------------------------------------------------------------------------------------
def test_rank_targets_errors():
    items, d = 300, 16
    E, bias = _heavy_tie_params(items, d, 7)
    ptr, it = synthetic_interactions(20, items, 10, seed=1)
    tp, ti = _csr([[u, (3 * u) % items] for u in range(20)])
    for where in ("E", "b"):
        E2, b2 = E.copy(), bias.copy()
        if where == "E":
            E2[123, 3] = np.inf
        else:
            b2[45] = np.inf
        g = _model(hparams(items, 8, d, int(ModelKind.EWMA), LOSS_HINGE, B=8), E2, b2)
        with pytest.raises(PredictionError.InvalidPredictionValue):
            g.rank_targets(ptr, it, tp, ti)
        with pytest.raises(PredictionError.InvalidPredictionValue):
            g.rank_targets_reps(np.ones((20, d), np.float32), tp, ti)
    g = _model(hparams(items, 8, d, int(ModelKind.EWMA), LOSS_HINGE, B=8), E, bias)
    assert g.rank_targets(ptr, it, tp, ti).size == 40

    def invalid(fn):
        with pytest.raises(EngineError) as e:
            fn()
        assert e.value.status == Status.INVALID_ARGUMENT

    bad = it.copy()
    bad[5] = items
    invalid(lambda: g.rank_targets(ptr, bad, tp, ti))
    bad_t = ti.copy()
    bad_t[7] = items
    invalid(lambda: g.rank_targets(ptr, it, tp, bad_t))
    invalid(lambda: g.rank_targets_reps(np.ones((20, d), np.float32), tp, bad_t))
    dec = ptr.copy()
    dec[3] = dec[4] + 1  # decreasing pointers
    invalid(lambda: g.rank_targets(dec, it, tp, ti))
    dec_t = tp.copy()
    dec_t[3] = dec_t[4] + 1
    invalid(lambda: g.rank_targets(ptr, it, dec_t, ti))
    invalid(lambda: g.rank_targets_reps(np.ones((20, d), np.float32), dec_t, ti))
    invalid(lambda: g.rank_targets_reps(np.ones((2, d), np.float32), tp[:3], ti, exclude=[[1], [items]]))
    up, ii, tpp, tii = (a.ctypes.data for a in (ptr, it, tp, ti))
    out = np.zeros(40, np.uint32)
    assert g._L.sbr_rank_targets(g._h, up, ii, 20, tpp, tii, 2, out.ctypes.data) == Status.INVALID_ARGUMENT  # unknown flag
    assert g._L.sbr_rank_targets(g._h, up, ii, 20, tpp, tii, 1, out.ctypes.data) == Status.OK
    # no users, and users without targets
    assert g.rank_targets(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32)).size == 0
    assert g.rank_targets(ptr, it, np.zeros(21, np.uint64), np.zeros(0, np.uint32)).size == 0


# ------------------------------------------------------------------------------------------------
# 8. extreme magnitudes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, None])
@pytest.mark.parametrize("case", ["subnormal_products", "subnormal_biases", "negative_zero"])
def test_rank_targets_extreme_magnitudes(monkeypatch, groups, case):
    """The shapes of test_recommend_extreme_magnitudes: scores in the subnormal range and scores that are -0.0 or +0.0, which
    `>=` holds equal (every rank of the negative_zero case is the number of unmasked items).  700 items, d = 16, 40 users, 20
    targets each, against the oracle."""
    _force(monkeypatch, groups)
    items, d, T = 700, 16, 8
    rs = np.random.RandomState(3)
    if case == "subnormal_products":
        E = (rs.randint(-64, 65, (items, d)) * 2.0 ** -76).astype(np.float32)
        bias = np.zeros(items, np.float32)
    elif case == "subnormal_biases":
        E = (rs.randint(-64, 65, (items, d)) * 2.0 ** -76).astype(np.float32)
        bias = (rs.randint(-50, 51, items) * 2.0 ** -149).astype(np.float32)
    else:
        E = (rs.randint(-3, 4, (items, d)) * 2.0 ** -100).astype(np.float32)
        bias = np.where(rs.rand(items) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    g, o = _pair(items, T, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(40, items, 2 * T, seed=4, min_len=1)
    hists = _histories(ptr, it)
    scores = oracle_scores(o, items, hists)
    tiny = np.float32(2.0 ** -126)
    if case == "negative_zero":
        assert np.all(scores == 0) and 0.02 < np.mean(np.signbit(scores)) < 0.98
    else:
        assert np.mean((scores != 0) & (np.abs(scores) < tiny)) > 0.9
    targets = [rs.randint(0, items, 20).astype(np.uint32) for _ in hists]
    got = rank_targets(g, hists, targets)
    want = expect_all(scores, hists, targets)
    assert_ranks_equal(got, want, case)
    if case == "negative_zero":
        for h, t, w in zip(hists, targets, want):
            assert all(r == (items if x in h else items - len(np.unique(h))) for x, r in zip(t.tolist(), w.tolist()))
    assert_ranks_equal(rank_targets(g, hists, targets, mask_history=False), expect_all(scores, hists, targets, mask_history=False), case)


@pytest.mark.parametrize("groups", [1, None])
def test_rank_targets_threshold_equal_to_f32_min(monkeypatch, groups):
    """Items whose real score IS f32::MIN (bias = MIN, embedding 0) as targets with masking on: their threshold equals the masked
    value, so every masked item counts against them as well as every other item (rank = num_items), while for any higher
    threshold a masked item counts for nothing.  Designed exact scores through rank_targets_reps, 2 000 items."""
    _force(monkeypatch, groups)
    items, users = 2000, 140
    rs = np.random.RandomState(8)
    y = rs.randint(-8, 9, items).astype(np.float64)
    b = rs.randint(-4, 5, items) * 0.25
    at_min = rs.choice(items, 30, replace=False)
    y[at_min] = 0.0
    b = b.astype(np.float32)
    b[at_min] = F32_MIN
    x = (1 + np.arange(users) % 4) * S
    g = _designed_model(y, b)
    masks = [rs.randint(0, items, rs.randint(0, 60)).astype(np.uint32) for _ in range(users)]
    targets = [np.concatenate([at_min[(u % 5):(u % 5) + 3], rs.randint(0, items, 6), masks[u][:1]]).astype(np.uint32) for u in range(users)]
    want = []
    for u in range(users):
        s = (b.astype(np.float64) + x[u] * y).astype(np.float32)
        assert np.array_equal(s.astype(np.float64), b.astype(np.float64) + x[u] * y) and np.all(s[at_min] == F32_MIN)
        want.append(ranks_expectation(s, np.unique(masks[u]), targets[u]))
        assert (want[-1][:3] == items).all()
    tp, ti = _csr(targets)
    got = _split(g.rank_targets_reps(_reps(x), tp, ti, exclude=masks), targets)
    assert_ranks_equal(got, want, "MIN thresholds")
