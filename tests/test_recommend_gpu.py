"""GPU: sbr_recommend / sbr_recommend_reps (exact top-k of the whole catalogue, sbr_catalogue.hip) against the oracle:
orc_user_representation + orc_predict over every item, then recommend_expect.topk_expectation.  Items and score bits must be
equal."""
import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams, synthetic_interactions
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM, oracle_recommend, topk_expectation
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, PredictionError

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    gi, gs = got
    wi, ws = want
    assert gi.shape == wi.shape, (gi.shape, wi.shape)
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{len(bad)} items differ; first at {bad[0]}: {gi[tuple(bad[0])]} vs {wi[tuple(bad[0])]}"
    assert np.array_equal(_bits(gs), _bits(ws))


def _pair(items, T, d, kind, E=None, bias=None):
    hp = hparams(items, T, d, int(kind), LOSS_HINGE, B=8)
    g, o = Model(hp), OracleModel(hp)
    for m in (g, o):
        if E is not None:
            m.set_param(Param.ITEM_EMBEDDING, E)
        if bias is not None:
            m.set_param(Param.ITEM_BIAS, bias)
    return g, o


def _tied_params(items, d, seed):
    rs = np.random.RandomState(seed)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    E[rs.randint(0, items, 20)] = E[0]  # exact score ties
    bias = np.round(rs.randn(items) * 0.5, 1).astype(np.float32)
    return E, bias


@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED, ModelKind.EWMA])
@pytest.mark.parametrize("d,items", [(1, 300), (16, 1500), (32, 5000), (100, 2000), (128, 700), (256, 3000)])
def test_recommend_matches_oracle(kind, d, items):
    T = 12
    E, bias = _tied_params(items, d, d + items)
    g, o = _pair(items, T, d, kind, E, bias)
    ptr, it = synthetic_interactions(40, items, 3 * T, seed=d, min_len=1, zipf=True)
    for k in (1, 10, 100, min(1024, items)):
        got = g.recommend(ptr, it, k)
        _same(got, oracle_recommend(o, items, ptr, it, k))


def test_recommend_all_ties():
    items, d, k = 3000, 32, 100
    E = np.tile(np.linspace(-1, 1, d, dtype=np.float32), (items, 1))
    bias = np.full(items, 0.25, np.float32)
    g, o = _pair(items, 8, d, ModelKind.LSTM_NORMAL, E, bias)
    ptr, it = synthetic_interactions(300, items, 20, seed=3, min_len=0)
    gi, gs = g.recommend(ptr, it, k)
    want = oracle_recommend(o, items, ptr, it, k)
    _same((gi, gs), want)
    for u in range(len(ptr) - 1):
        h = set(int(x) for x in it[ptr[u]: ptr[u + 1]])
        assert gi[u].tolist() == [i for i in range(items) if i not in h][:k]


@pytest.mark.parametrize("direction", [1, -1])
def test_recommend_adversarial_order(direction):
    """Bias strictly monotone in the item id: every score beats the running threshold (increasing) or almost none does
    (decreasing); 200 000 items, k = 1024: staging merges and several item ranges per user."""
    items, d, k = 200_000, 32, 1024
    rs = np.random.RandomState(5)
    E = (rs.randn(items, d) * 1e-6).astype(np.float32)
    bias = (np.arange(items, dtype=np.float64) * 1e-3 * direction).astype(np.float32)
    g, o = _pair(items, 8, d, ModelKind.EWMA, E, bias)
    ptr, it = synthetic_interactions(160, items, 12, seed=9, min_len=0)
    it = it.copy()
    it[::3] = (items - 1 - it[::3] % 2000) if direction > 0 else it[::3] % 2000  # histories inside the top of the order
    got = g.recommend(ptr, it, k)
    _same(got, oracle_recommend(o, items, ptr, it, k))


def test_recommend_exclusion_and_padding():
    items, d, T = 400, 16, 6
    E, bias = _tied_params(items, d, 1)
    g, o = _pair(items, T, d, ModelKind.LSTM_NORMAL, E, bias)
    rs = np.random.RandomState(2)
    hists = [
        rs.randint(0, items, 25),                      # longer than T: state from the last T, mask from all 25
        np.array([7, 7, 7, 3, 3, 9, 7], np.uint32),    # duplicates
        np.zeros(0, np.uint32),                        # empty history: item 0's state, nothing excluded
        np.arange(0, items - 3, dtype=np.uint32),      # 3 eligible items left
    ]
    ptr = np.zeros(len(hists) + 1, np.uint64)
    ptr[1:] = np.cumsum([h.size for h in hists])
    it = np.concatenate(hists).astype(np.uint32)
    k = 10
    got = g.recommend(ptr, it, k)
    _same(got, oracle_recommend(o, items, ptr, it, k))
    assert got[0][3].tolist()[3:] == [NO_ITEM] * 7 and np.all(np.isneginf(got[1][3][3:]))
    assert not set(got[0][0].tolist()) & set(hists[0].tolist())
    inc = g.recommend(ptr, it, k, include_history=True)
    _same(inc, oracle_recommend(o, items, ptr, it, k, include_history=True))
    assert set(inc[0][3].tolist()) & set(hists[3].tolist())
    # the lstm / ewma wrapper: a list of sequences, the history excluded by default
    import sbr_rs_amd as sbr

    w = sbr.lstm.ImplicitLSTMModel(g)
    _same(w.recommend(hists, k), got)
    _same(w.recommend(hists, k, exclude_history=False), inc)


def test_recommend_reps_equals_recommend():
    items, d, T = 2500, 100, 10
    E, bias = _tied_params(items, d, 4)
    g, o = _pair(items, T, d, ModelKind.LSTM_COUPLED, E, bias)
    ptr, it = synthetic_interactions(150, items, 30, seed=12, min_len=0)
    k = 50
    reps = np.array([g.user_representation(it[ptr[u]: ptr[u + 1]]) for u in range(len(ptr) - 1)], np.float32)
    hists = [np.unique(it[ptr[u]: ptr[u + 1]]) for u in range(len(ptr) - 1)]
    _same(g.recommend_reps(reps, k, exclude=[it[ptr[u]: ptr[u + 1]] for u in range(len(ptr) - 1)]), g.recommend(ptr, it, k))
    _same(g.recommend_reps(reps, k), g.recommend(ptr, it, k, include_history=True))
    # arbitrary per-user exclusion lists
    rs = np.random.RandomState(0)
    excl = [rs.randint(0, items, rs.randint(0, 40)) for _ in range(len(reps))]
    gi, gs = g.recommend_reps(reps, k, exclude=excl)
    all_items = np.arange(items, dtype=np.uint32)
    for u in range(len(reps)):
        wi, ws = topk_expectation(o.predict(reps[u], all_items), excl[u], k)
        assert np.array_equal(gi[u], wi) and np.array_equal(_bits(gs[u]), _bits(ws))
    assert len(hists) == len(reps)


def test_recommend_errors():
    items, d = 300, 16
    E, bias = _tied_params(items, d, 7)
    ptr, it = synthetic_interactions(20, items, 10, seed=1)
    for where in ("E", "b"):
        E2, b2 = E.copy(), bias.copy()
        if where == "E":
            E2[123, 3] = np.inf
        else:
            b2[45] = np.inf
        g, _ = _pair(items, 8, d, ModelKind.EWMA, E2, b2)
        with pytest.raises(PredictionError.InvalidPredictionValue):
            g.recommend(ptr, it, 10)
        with pytest.raises(PredictionError.InvalidPredictionValue):
            g.recommend_reps(np.ones((3, d), np.float32), 10)
    g, _ = _pair(items, 8, d, ModelKind.EWMA, E, bias)
    for k in (0, 1025):
        with pytest.raises(EngineError) as e:
            g.recommend(ptr, it, k)
        assert e.value.status == Status.INVALID_ARGUMENT
    bad = it.copy()
    bad[5] = items
    with pytest.raises(EngineError) as e:
        g.recommend(ptr, bad, 10)
    assert e.value.status == Status.INVALID_ARGUMENT
    dec = ptr.copy()
    dec[3] = dec[4] + 1  # decreasing pointers
    with pytest.raises(EngineError) as e:
        g.recommend(dec, it, 10)
    assert e.value.status == Status.INVALID_ARGUMENT
    with pytest.raises(EngineError) as e:
        g.recommend_reps(np.ones((2, d), np.float32), 10, exclude=[[1], [items]])
    assert e.value.status == Status.INVALID_ARGUMENT


def test_recommend_headline_shape():
    """BASELINE configs[2]'s table (1e6 items, d = 128), 8 192 users, k = 100, seeded parameters: 32 sampled users against the
    oracle; two calls bitwise identical over all users; the whole first user tile (users 0..127) and the last 128 users against
    the top k of the engine's own predict over all items (predict is held to the oracle in test_parity_gpu.py and by the 32
    users here)."""
    items, d, T, k, U = 1_000_000, 128, 64, 100, 8192
    hp = hparams(items, T, d, int(ModelKind.LSTM_NORMAL), LOSS_HINGE, B=32)
    g = Model(hp)
    ptr, it = synthetic_interactions(U, items, 64, seed=21, min_len=0, zipf=True)
    a = g.recommend(ptr, it, k)
    b = g.recommend(ptr, it, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    o = OracleModel(hp)
    users = np.unique(np.concatenate([[0, 1, 127, 128, 4095, 4096, U - 1], np.random.RandomState(3).choice(U, 25, replace=False)]))
    want = oracle_recommend(o, items, ptr, it, k, users=users)
    _same((a[0][users], a[1][users]), want)
    ptr64 = np.asarray(ptr, dtype=np.int64)
    all_items = np.arange(items, dtype=np.uint32)
    tiles = np.concatenate([np.arange(128), np.arange(U - 128, U)])
    rows = []
    for u in tiles:
        h = it[ptr64[u]: ptr64[u + 1]]
        rows.append(topk_expectation(g.predict(g.user_representation(h), all_items), np.unique(h), k))
    _same((a[0][tiles], a[1][tiles]), (np.array([r[0] for r in rows]), np.array([r[1] for r in rows])))


def test_recommend_partitioned_replica():
    from sbr_rs_amd.engine import group_create

    items, d, T, k = 1237, 32, 10, 64
    hp = hparams(items, T, d, int(ModelKind.LSTM_NORMAL), LOSS_HINGE, B=8, ndev=2)
    part = group_create(hp, 2, partition_item_table=True)
    rep = group_create(hp, 2)
    assert part[1].is_partitioned() and not rep[0].is_partitioned()
    ptr, it = synthetic_interactions(70, items, 20, seed=8, min_len=0)
    want = rep[0].recommend(ptr, it, k)
    _same(part[1].recommend(ptr, it, k), want)
    _same(part[0].recommend(ptr, it, k), want)
    _same(want, oracle_recommend(OracleModel(hp), items, ptr, it, k))
