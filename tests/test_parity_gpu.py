"""GPU parity: the HIP engine (through the C-ABI) against the CPU oracle on identical seeded
inputs.  Bar: bit-exact for indices (negatives, tries, ranks) AND for every float the training
path produces (hidden states, gradients, parameters after whole fits) — the engine reproduces the
oracle's association orders, so no tolerance is needed.  The reported loss is accumulated
order-free in f64 and is compared with rtol 1e-6."""
import numpy as np
import pytest

from helpers import (LOSS_BPR, LOSS_HINGE, LOSS_WARP, OPT_ADAM, PAR_ASYNC, PAR_SYNC, hparams, movielens_protocol,
                     synthetic_interactions)
from oracle.oracle import OracleError, OracleModel
from sbr_rs_amd._abi import Debug, ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, FittingError, PredictionError

pytestmark = pytest.mark.gpu

ALL_PARAMS = {
    ModelKind.EWMA: [Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_BIAS, Param.ITEM_BIAS_ACC,
                     Param.EWMA_ALPHA, Param.EWMA_ALPHA_ACC],
    ModelKind.LSTM_NORMAL: [Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_BIAS, Param.ITEM_BIAS_ACC,
                            Param.LSTM_W, Param.LSTM_W_ACC, Param.LSTM_B, Param.LSTM_B_ACC],
}
ALL_PARAMS[ModelKind.LSTM_COUPLED] = ALL_PARAMS[ModelKind.LSTM_NORMAL]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    if a.dtype == np.float32:
        bad = np.flatnonzero(bits(a).ravel() != bits(b).ravel())
        if bad.size:
            i = bad[0]
            raise AssertionError(f"{what}: {bad.size}/{a.size} differ; first at {i}: gpu={a.ravel()[i]!r} oracle={b.ravel()[i]!r}")
    else:
        assert np.array_equal(a, b), what


def assert_params_equal(gpu, orc, kind, what=""):
    for p in ALL_PARAMS[kind]:
        assert_same_bits(gpu.get_param(p), orc.get_param(p), f"{what} param {p.name}")


def make_pair(hp):
    return Model(hp), OracleModel(hp)


@pytest.mark.parametrize("kind", [ModelKind.EWMA, ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED])
@pytest.mark.parametrize("d", [16, 32, 128, 24, 100])
def test_init_matches(kind, d):
    hp = hparams(97, 12, d, int(kind), LOSS_HINGE, B=4)
    g, o = make_pair(hp)
    assert_params_equal(g, o, kind, "init")


CASES = [
    # kind, loss, d, items, users, T, B
    (ModelKind.EWMA, LOSS_HINGE, 32, 200, 60, 20, 8),
    (ModelKind.EWMA, LOSS_WARP, 128, 500, 40, 16, 5),
    (ModelKind.EWMA, LOSS_BPR, 16, 50, 30, 9, 64),
    (ModelKind.EWMA, LOSS_WARP, 256, 300, 25, 10, 7),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 32, 200, 60, 20, 8),
    (ModelKind.LSTM_NORMAL, LOSS_HINGE, 128, 400, 70, 12, 33),
    (ModelKind.LSTM_NORMAL, LOSS_BPR, 16, 60, 30, 9, 4),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 64, 150, 45, 14, 17),
    (ModelKind.LSTM_COUPLED, LOSS_WARP, 32, 120, 40, 11, 6),
    (ModelKind.LSTM_COUPLED, LOSS_BPR, 16, 80, 30, 8, 3),
    (ModelKind.LSTM_COUPLED, LOSS_HINGE, 64, 90, 30, 10, 16),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 256, 100, 20, 6, 5),
    # embedding_dim that is not one of the kernels' widths: stored in the next width up, extra columns zero
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 48, 150, 45, 14, 9),
    (ModelKind.LSTM_COUPLED, LOSS_HINGE, 100, 90, 30, 10, 16),
    (ModelKind.EWMA, LOSS_WARP, 24, 200, 60, 20, 8),
    (ModelKind.EWMA, LOSS_BPR, 200, 120, 25, 10, 7),
]


@pytest.mark.parametrize("kind,loss,d,items,users,T,B", CASES)
def test_one_minibatch_intermediates(kind, loss, d, items, users, T, B):
    ptr, it = synthetic_interactions(users, items, T + 5, seed=11, zipf=True)
    hp = hparams(items, T, d, int(kind), loss, B=B, lr=0.05)
    g, o = make_pair(hp)
    # make scores non-trivial so the WARP search actually iterates
    rs = np.random.RandomState(5)
    E = (rs.randn(items, d) * 0.4).astype(np.float32)
    bias = (rs.randn(items) * 0.5).astype(np.float32)
    for m in (g, o):
        m.set_param(Param.ITEM_EMBEDDING, E)
        m.set_param(Param.ITEM_BIAS, bias)
    pg, po = g.fit_begin(ptr, it), o.fit_begin(ptr, it)
    nmb = po.epoch_prepare()
    assert pg.epoch_prepare() == nmb
    for mb in range(min(2, nmb)):
        R = po.minibatch_rows(mb)
        assert pg.minibatch_rows(mb) == R
        pg.step_local(mb)
        po.step_local(mb)
        for which in (Debug.IN_IDX, Debug.OUT_IDX, Debug.HIDDEN, Debug.NEGATIVES, Debug.TRIES, Debug.COEF, Debug.LOSS,
                      Debug.DHIDDEN, Debug.DINPUT, Debug.DENSE_GRAD):
            assert_same_bits(pg.debug_fetch(which, R), po.debug_fetch(which, R), f"mb{mb} {which.name}")
        pg.step_apply(mb)
        po.step_apply(_export(po))
        assert_params_equal(g, o, kind, f"after mb{mb}")


@pytest.mark.parametrize("kind,loss", [(ModelKind.LSTM_NORMAL, LOSS_WARP), (ModelKind.LSTM_COUPLED, LOSS_HINGE)])
@pytest.mark.parametrize("min_tiles", ["1", "1000000"])
def test_d256_bptt_both_forms(monkeypatch, kind, loss, min_tiles):
    """d = 256 BPTT: the sequence-resident kernel (large minibatches) and the per-step launches (small ones) give
    the oracle's bits; SBR_BWD256_MIN_TILES forces one or the other."""
    monkeypatch.setenv("SBR_BWD256_MIN_TILES", min_tiles)
    items, T, B = 120, 9, 70  # three 32-sequence tiles, the last one ragged
    ptr, it = synthetic_interactions(90, items, T + 3, seed=17, zipf=True)
    hp = hparams(items, T, 256, int(kind), loss, B=B, lr=0.05)
    g, o = make_pair(hp)
    pg, po = g.fit_begin(ptr, it), o.fit_begin(ptr, it)
    assert pg.epoch_prepare() == po.epoch_prepare()
    R = po.minibatch_rows(0)
    pg.step_local(0)
    po.step_local(0)
    for which in (Debug.HIDDEN, Debug.COEF, Debug.DINPUT, Debug.DENSE_GRAD):
        assert_same_bits(pg.debug_fetch(which, R), po.debug_fetch(which, R), f"{which.name}")
    pg.step_apply(0)
    po.step_apply(_export(po))
    assert_params_equal(g, o, kind, "after the step")


@pytest.mark.parametrize("stream", ["0", "1"])
@pytest.mark.parametrize("rows_per_group", ["1", "2", None])
def test_warp_retry_loop_all_trip_counts(monkeypatch, rows_per_group, stream):
    """sample_warp_negative (sequence_model.rs:47-68): every trip count 1..5 occurs, including
    rows where no candidate violates and the 5th draw is used anyway.  Both forms of the score kernel: one row per lane
    group in flight (bandwidth-bound launches) and two, their retry rounds in lockstep (latency-bound launches); each with its
    rows gathered streaming (nt) and cached (SBR_STREAM: the step's cache policy by size, forced either way)."""
    monkeypatch.setenv("SBR_STREAM", stream)
    if rows_per_group:
        monkeypatch.setenv("SBR_SCORE_U", rows_per_group)
    items, d, T = 400, 64, 24
    ptr, it = synthetic_interactions(80, items, T, seed=31)
    for kind in (ModelKind.EWMA, ModelKind.LSTM_NORMAL):
        hp = hparams(items, T, d, int(kind), LOSS_WARP, B=64)
        g, o = make_pair(hp)
        rs = np.random.RandomState(6)
        E = (rs.randn(items, d) * (0.45 if kind == ModelKind.EWMA else 1.2)).astype(np.float32)
        bias = (rs.randn(items) * 1.0).astype(np.float32)
        for m in (g, o):
            m.set_param(Param.ITEM_EMBEDDING, E)
            m.set_param(Param.ITEM_BIAS, bias)
        pg, po = g.fit_begin(ptr, it), o.fit_begin(ptr, it)
        pg.epoch_prepare(), po.epoch_prepare()
        R = po.minibatch_rows(0)
        pg.step_local(0), po.step_local(0)
        tries = po.debug_fetch(Debug.TRIES, R)
        coef = po.debug_fetch(Debug.COEF, R)
        assert set(np.unique(tries)) == {1, 2, 3, 4, 5}, np.bincount(tries)
        assert np.any((tries == 5) & (coef == 0.0)), "no row exhausted the 5 tries without a violation"
        for which in (Debug.NEGATIVES, Debug.TRIES, Debug.COEF, Debug.LOSS, Debug.DHIDDEN):
            assert_same_bits(pg.debug_fetch(which, R), po.debug_fetch(which, R), f"{kind.name} {which.name}")


def assert_lagged_equal(g, o, what):
    """The number the reference's fit returns (stale loss-node values, sequence_model.rs:157 before :160):
    a sequential f32 chain on both sides, compared bit for bit."""
    assert_same_bits(np.array([g.last_fit_lagged_loss()], dtype=np.float32), np.array([o.last_fit_lagged_loss()], dtype=np.float32),
                     f"{what}: lagged loss figure")


def _export(po):
    """The oracle's apply consumes the exported block of device 0."""
    import ctypes as C

    from oracle.oracle import lib

    out = np.zeros(po.exchange_bytes(), dtype=np.uint8)
    assert lib().orc_fit_export_local(po._h, 0, out.ctypes.data_as(C.c_void_p)) == 0
    return out


@pytest.mark.parametrize("kind,loss,d,items,users,T,B", CASES)
def test_whole_fit_bit_exact(kind, loss, d, items, users, T, B):
    ptr, it = synthetic_interactions(users, items, T + 5, seed=23, zipf=(d % 32 == 0))
    hp = hparams(items, T, d, int(kind), loss, B=B, epochs=3)
    g, o = make_pair(hp)
    lg, lo = g.fit(ptr, it), o.fit(ptr, it)
    assert_params_equal(g, o, kind, "after fit")
    assert lg == pytest.approx(lo, rel=1e-6)
    # the number the reference's fit returns (stale loss-node values, sequence_model.rs:157): f32 chain, compared bit for bit
    assert_lagged_equal(g, o, "whole fit")
    assert g.last_fit_lagged_loss() > 0.0
    # second fit call continues training (optimiser state and epoch counter persist)
    lg, lo = g.fit(ptr, it), o.fit(ptr, it)
    assert_params_equal(g, o, kind, "after second fit")
    assert g.global_epoch() == o.global_epoch() == 6
    # prediction side
    tptr, tit = synthetic_interactions(25, items, 3 * T, seed=99, min_len=1)
    mg, rg = g.mrr_score(tptr, tit)
    mo, ro = o.mrr_score(tptr, tit)
    assert np.array_equal(rg, ro)
    assert mg == mo
    hist = tit[: T + 3]
    ug, uo = g.user_representation(hist), o.user_representation(hist)
    assert_same_bits(ug, uo, "user_representation (longer than T)")
    assert_same_bits(g.user_representation(hist[:2]), o.user_representation(hist[:2]), "user_representation short")
    assert_same_bits(g.user_representation([]), o.user_representation([]), "user_representation empty")
    all_items = np.arange(items, dtype=np.uint32)
    assert_same_bits(g.predict(ug, all_items), o.predict(uo, all_items), "predict")


@pytest.mark.parametrize("kind,loss,d,world,exchange", [
    (ModelKind.EWMA, LOSS_WARP, 32, 2, "owner"),
    (ModelKind.LSTM_NORMAL, LOSS_HINGE, 64, 3, "owner"),
    (ModelKind.LSTM_COUPLED, LOSS_WARP, 16, 4, "owner"),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 2, "gradient"),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 8, "owner"),   # the node size of BASELINE configs[3]: eight chunks, eight owner inputs
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 8, "gradient"),
    (ModelKind.EWMA, LOSS_HINGE, 256, 8, "owner"),
    (ModelKind.EWMA, LOSS_HINGE, 64, 3, "gradient"),
    (ModelKind.EWMA, LOSS_WARP, 32, 9, "owner"),       # more than eight devices: the kernels' 16-device instantiations
    (ModelKind.LSTM_NORMAL, LOSS_HINGE, 32, 9, "gradient"),
])
def test_multi_device_halves_on_one_gpu(kind, loss, d, world, exchange):
    """The multi-GPU protocol through the C-ABI halves with `world` simulated ranks on ONE GPU (tests/simulated_ranks.py: the
    collectives are tensor copies, everything else is the production path), in both forms of the Synchronous step: the
    owner-applied update (scatter / owner_update / in-place all-gather of the parameter slices; the optimiser-state slices when
    the fit ends) and the gradient all-gather (scatter / owner_reduce / apply_table).  All replicas must end bit-identical to each
    other and to the single-process oracle with num_devices = world — parameters AND optimiser state."""
    from simulated_ranks import SimulatedRanks

    items, T, B = 203, 12, 6   # 203 % world != 0 for every world here: ragged last slice
    ptr, it = synthetic_interactions(90 if world < 8 else 240, items, T + 4, seed=17, zipf=True)
    models, plans = [], []
    for q in range(world):
        m = Model(hparams(items, T, d, int(kind), loss, epochs=2, B=B, ndev=world, rank=q))
        models.append(m)
        plans.append(m.fit_begin(ptr, it))
    ranks = SimulatedRanks(models, plans)
    for _ in range(2):
        nmb = {p.epoch_prepare() for p in plans}
        assert len(nmb) == 1
        for mb in range(nmb.pop()):
            ranks.step(mb, exchange)
    if exchange == "owner":  # a row's optimiser state lives on its owner until the slices are gathered: reading it earlier fails loudly
        assert all(m.optimizer_state_is_partial() for m in models)
        with pytest.raises(EngineError):
            models[0].get_param(Param.ITEM_EMBEDDING_ACC)
    ranks.finish()
    o = OracleModel(hparams(items, T, d, int(kind), loss, epochs=2, B=B, ndev=world, rank=0))
    lo = o.fit(ptr, it)
    for q in range(world):
        assert_params_equal(models[q], o, kind, f"rank {q} of {world}")
        lg, ex = plans[q].end()
        assert lg == pytest.approx(lo, rel=1e-6)


@pytest.mark.parametrize("kind,loss,d,world,opt,par", [
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 32, 2, 0, PAR_SYNC),
    (ModelKind.EWMA, LOSS_HINGE, 64, 3, 0, PAR_SYNC),
    (ModelKind.LSTM_COUPLED, LOSS_BPR, 16, 4, OPT_ADAM, PAR_SYNC),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 64, 2, 0, PAR_ASYNC),   # staleness-one pipeline on an exchange stream
    (ModelKind.EWMA, LOSS_WARP, 32, 3, 0, PAR_ASYNC),
    (ModelKind.LSTM_COUPLED, LOSS_HINGE, 128, 4, OPT_ADAM, PAR_ASYNC),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 8, 0, PAR_SYNC),   # world 8 = one xGMI node
    (ModelKind.EWMA, LOSS_HINGE, 64, 8, 0, PAR_ASYNC),
])
def test_group_fit_single_process(kind, loss, d, world, opt, par):
    """sbr_group_fit: `world` replicas driven from ONE process, the exchange as event-ordered peer
    copies between the replicas' streams (here all on one GPU).  ≙ fit with num_threads(world);
    must equal the oracle with num_devices = world bit for bit, on every replica, and a second
    fit call must keep training from the same state on both sides."""
    from sbr_rs_amd.engine import group_fit

    items, T, B = 211, 12, 5
    ptr, it = synthetic_interactions(100 if world < 8 else 260, items, T + 5, seed=23, zipf=True)
    mk = lambda q: hparams(items, T, d, int(kind), loss, epochs=3, B=B, ndev=world, rank=q, opt=opt,
                           lr=0.02 if opt == OPT_ADAM else 0.16, par=par)
    models = [Model(mk(q)) for q in range(world)]
    o = OracleModel(mk(0))
    for call in range(2):
        lg = group_fit(models, ptr, it)
        lo = o.fit(ptr, it)
        assert lg == pytest.approx(lo, rel=1e-6)
        for q in range(world):
            assert_params_equal(models[q], o, kind, f"group_fit call {call} rank {q} of {world}")
            assert_lagged_equal(models[q], o, f"group_fit call {call} rank {q} of {world}")  # the workers' terms added in worker order


@pytest.mark.parametrize("kind,loss,d,world,opt", [
    (ModelKind.EWMA, LOSS_HINGE, 256, 2, 0),          # BASELINE configs[4] in miniature: EWMA + hinge, d = 256
    (ModelKind.EWMA, LOSS_WARP, 32, 3, 0),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 64, 4, 0),
    (ModelKind.LSTM_COUPLED, LOSS_BPR, 16, 2, OPT_ADAM),
    (ModelKind.EWMA, LOSS_HINGE, 128, 1, 0),          # a group of one: the table is just mapped memory
    (ModelKind.EWMA, LOSS_HINGE, 256, 8, 0),          # configs[4]'s world: eight owners
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 8, 0),
    (ModelKind.EWMA, LOSS_WARP, 64, 9, 0),            # more than eight owners: the list merge's 16-device instantiation
])
def test_partitioned_item_table_group_fit(kind, loss, d, world, opt):
    """sbr_group_create(SBR_GROUP_PARTITION_ITEM_TABLE): the item table exists once (row range r on
    replica r's device, one virtual range mapped into every replica), every replica reads it with the
    unchanged kernels, each row is updated by its owner from the devices' gradient lists merged in
    device order.  Must equal the oracle's replicated num_devices = world run bit for bit — table,
    optimiser state and dense parameters — and prediction / MRR must work from any replica."""
    from sbr_rs_amd.engine import group_create, group_fit

    items, T, B = 1237, 12, 5   # 1237 rows over `world` owners: uneven last slice, several 4 KiB pages
    ptr, it = synthetic_interactions(110 if world < 8 else 280, items, T + 5, seed=29, zipf=True)
    tptr, tit = synthetic_interactions(30, items, T, seed=31)
    hp = hparams(items, T, d, int(kind), loss, epochs=3, B=B, ndev=world, opt=opt, lr=0.02 if opt == OPT_ADAM else 0.16)
    models = group_create(hp, world, partition_item_table=True)
    assert all(m.is_partitioned() for m in models)
    o = OracleModel(hp)
    for call in range(2):
        lg = group_fit(models, ptr, it)
        lo = o.fit(ptr, it)
        assert lg == pytest.approx(lo, rel=1e-6)
        for q in range(world):
            assert_params_equal(models[q], o, kind, f"partitioned call {call} replica {q} of {world}")
    mo, ro = o.mrr_score(tptr, tit)
    for q in (0, world - 1):
        mg, rg = models[q].mrr_score(tptr, tit)
        assert np.array_equal(rg, ro) and mg == mo


@pytest.mark.parametrize("threads", [True, False])
@pytest.mark.parametrize("kind,loss,d,world,par,partition", [
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 32, 3, PAR_SYNC, False),
    (ModelKind.EWMA, LOSS_HINGE, 64, 3, PAR_ASYNC, False),     # the staleness-one pipeline, phase by phase
    (ModelKind.LSTM_COUPLED, LOSS_WARP, 16, 5, PAR_SYNC, True),  # owner-computes over a partitioned table
])
def test_group_plan_steps_with_and_without_host_threads(kind, loss, d, world, par, partition, threads):
    """sbr_group_fit taken apart (sbr_group_fit_begin / _epoch_prepare / _step / _fit_end), with one host thread per device
    queueing that device's launches (≙ one rayon worker per partition, sequence_model.rs:100-102) and with one thread for all:
    both must equal the oracle with num_devices = world bit for bit on every replica — the phases' host barriers order every
    event record before the waits on it."""
    from sbr_rs_amd.engine import GroupPlan, group_create

    items, T, B, epochs = 211, 12, 5, 3
    ptr, it = synthetic_interactions(130, items, T + 5, seed=37, zipf=True)
    hp = hparams(items, T, d, int(kind), loss, epochs=epochs, B=B, ndev=world, par=par)
    models = group_create(hp, world, partition_item_table=partition)
    o = OracleModel(hp)
    gp = GroupPlan(models, ptr, it, host_threads=threads)
    for e in range(epochs):
        for mb in range(gp.epoch_prepare(prefetch_next=e + 1 < epochs)):
            gp.step(mb)
    ms, steps, nthreads = gp.stats()
    assert steps > 0 and ms > 0 and nthreads == (world if threads else 1)
    lg = gp.end()
    lo = o.fit(ptr, it)
    assert lg == pytest.approx(lo, rel=1e-6)
    for q in range(world):
        assert_params_equal(models[q], o, kind, f"group plan (host threads {threads}) replica {q} of {world}")
        assert_lagged_equal(models[q], o, f"group plan replica {q}")


def test_group_create_replicated_matches_individual_models():
    from sbr_rs_amd.engine import group_create, group_fit

    ptr, it = synthetic_interactions(60, 150, 14, seed=3, zipf=True)
    hp = hparams(150, 12, 32, int(ModelKind.LSTM_NORMAL), LOSS_WARP, epochs=2, B=4, ndev=2)
    a = group_create(hp, 2)
    assert not a[0].is_partitioned()
    b = [Model(hparams(150, 12, 32, int(ModelKind.LSTM_NORMAL), LOSS_WARP, epochs=2, B=4, ndev=2, rank=q)) for q in range(2)]
    group_fit(a, ptr, it)
    group_fit(b, ptr, it)
    for q in range(2):
        for p in (Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.LSTM_W, Param.ITEM_BIAS):
            assert_same_bits(a[q].get_param(p), b[q].get_param(p), f"replica {q} {p.name}")


ADAM_BLOCKS = {
    ModelKind.EWMA: [Param.ITEM_EMBEDDING_M, Param.ITEM_BIAS_M, Param.EWMA_ALPHA_M],
    ModelKind.LSTM_NORMAL: [Param.ITEM_EMBEDDING_M, Param.ITEM_BIAS_M, Param.LSTM_W_M, Param.LSTM_B_M],
    ModelKind.LSTM_COUPLED: [Param.ITEM_EMBEDDING_M, Param.ITEM_BIAS_M, Param.LSTM_W_M, Param.LSTM_B_M],
}


@pytest.mark.parametrize("kind,loss,d,B", [
    (ModelKind.LSTM_COUPLED, LOSS_BPR, 16, 4),     # Hyperparameters::new defaults (lstm.rs:56-71)
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 64, 9),
    (ModelKind.EWMA, LOSS_HINGE, 128, 16),
])
def test_adam_whole_fit_bit_exact(kind, loss, d, B):
    items, T = 150, 12
    ptr, it = synthetic_interactions(50, items, T + 4, seed=41, zipf=True)
    hp = hparams(items, T, d, int(kind), loss, lr=0.01, l2=1e-5, epochs=3, B=B, opt=OPT_ADAM)
    g, o = make_pair(hp)
    lg, lo = g.fit(ptr, it), o.fit(ptr, it)
    g.fit(ptr, it), o.fit(ptr, it)  # bias-correction counter persists across fits
    assert_params_equal(g, o, kind, "adam")
    for p in ADAM_BLOCKS[kind]:
        assert_same_bits(g.get_param(p), o.get_param(p), f"adam moment {p.name}")
    assert g.counters() == (o.global_epoch(), o.optimizer_steps())
    assert lg == pytest.approx(lo, rel=1e-6)
    mg, rg = g.mrr_score(ptr, it)
    mo, ro = o.mrr_score(ptr, it)
    assert np.array_equal(rg, ro) and mg == mo


@pytest.mark.parametrize("exchange", ["owner", "gradient"])
def test_adam_multi_device_halves(exchange, kind=ModelKind.LSTM_COUPLED):
    from simulated_ranks import SimulatedRanks

    world, items, T, B, d = 2, 101, 10, 5, 32
    ptr, it = synthetic_interactions(60, items, T + 3, seed=19, zipf=True)
    mk = lambda q: hparams(items, T, d, int(kind), LOSS_BPR, lr=0.02, epochs=1, B=B, ndev=world, rank=q, opt=OPT_ADAM)
    models = [Model(mk(q)) for q in range(world)]
    plans = [m.fit_begin(ptr, it) for m in models]
    ranks = SimulatedRanks(models, plans)
    nmb = plans[0].epoch_prepare()
    assert plans[1].epoch_prepare() == nmb
    for mb in range(nmb):
        ranks.step(mb, exchange)
    ranks.finish()  # owner form: both Adam moments of the item table live on the rows' owners until here
    o = OracleModel(mk(0))
    o.fit(ptr, it)
    for q in range(world):
        assert_params_equal(models[q], o, kind, f"adam rank {q}")
        for p in ADAM_BLOCKS[kind]:
            assert_same_bits(models[q].get_param(p), o.get_param(p), f"adam rank {q} {p.name}")


def test_default_hyperparameters_through_the_python_api():
    """The reference's README flow with Hyperparameters::new defaults (Coupled LSTM, BPR, Adam)."""
    import sbr_rs_amd as sbr

    ptr, it = synthetic_interactions(80, 120, 20, seed=3, zipf=True)
    users = np.repeat(np.arange(80), np.diff(ptr.astype(np.int64)))
    data = sbr.data.Interactions.from_arrays(users, it, np.arange(len(it)), 80, 120)
    rng = sbr.XorShiftRng.from_seed(bytes([42] * 16))
    train, test = sbr.data.user_based_split(data, rng, 0.2)
    model = sbr.lstm.Hyperparameters.new(data.num_items(), 16).rng(rng).num_epochs(3).batch_sequences(8).build()
    l0 = model.fit(train.to_compressed())
    l1 = model.fit(train.to_compressed())
    assert np.isfinite(l0) and l1 < l0
    mrr = sbr.evaluation.mrr_score(model, test.to_compressed())
    assert 0.0 < mrr <= 1.0
    user = model.user_representation([1, 2, 3])
    assert model.predict(user, np.arange(120)).shape == (120,)
    with pytest.raises(sbr.FittingError.NoInteractions):
        sbr.ewma.Hyperparameters.new(120, 16).build().fit(sbr.data.Interactions(10, 120).to_compressed())


def test_num_threads_two_through_the_python_api():
    """`.num_threads(2)` in ONE process (≙ lstm.rs:475-497's configuration): two replicas, group fit;
    equals the oracle with num_devices = 2."""
    import sbr_rs_amd as sbr

    ptr, it = synthetic_interactions(70, 150, 18, seed=4, zipf=True)
    seed = bytes([7] * 16)
    comp = sbr.data.CompressedInteractions(70, 150, ptr, it, np.zeros(len(it), dtype=np.uint64))
    model = (sbr.lstm.Hyperparameters.new(150, 16).from_seed(seed).embedding_dim(32).loss(sbr.Loss.Hinge)
             .optimizer(sbr.Optimizer.Adagrad).lstm_variant(sbr.LSTMVariant.Normal).learning_rate(0.16).l2_penalty(0.0004)
             .num_epochs(2).num_threads(2).batch_sequences(6).build())
    lg = model.fit(comp)
    o = OracleModel(hparams(150, 16, 32, int(ModelKind.LSTM_NORMAL), LOSS_HINGE, epochs=2, B=6, seed=seed, ndev=2))
    lo = o.fit(ptr, it)
    assert lg == pytest.approx(lo, rel=1e-6)
    assert_params_equal(model.params, o, ModelKind.LSTM_NORMAL, "num_threads(2)")


def test_partition_item_table_through_the_python_api():
    import sbr_rs_amd as sbr

    ptr, it = synthetic_interactions(70, 900, 18, seed=4, zipf=True)
    comp = sbr.data.CompressedInteractions(70, 900, ptr, it, np.zeros(len(it), dtype=np.uint64))
    mk = lambda: (sbr.ewma.Hyperparameters.new(900, 16).from_seed(bytes([9] * 16)).embedding_dim(256).loss(sbr.Loss.Hinge)
                  .optimizer(sbr.Optimizer.Adagrad).learning_rate(0.16).num_epochs(2).num_threads(3).batch_sequences(6))
    rep, part = mk().build(), mk().partition_item_table().build()
    assert part.params.is_partitioned() and not rep.params.is_partitioned()
    assert rep.fit(comp) == part.fit(comp)
    assert_params_equal(part.params, rep.params, ModelKind.EWMA, "partitioned vs replicated")
    assert sbr.evaluation.mrr_score(part, comp) == sbr.evaluation.mrr_score(rep, comp)


def test_save_load_resumes_training_bit_exactly(tmp_path):
    """≙ the serde derives (lstm.rs:204,386): parameters + optimiser state + counters round-trip, and
    training continues exactly as if it had never been interrupted (given the same next-fit seed)."""
    import sbr_rs_amd as sbr

    ptr, it = synthetic_interactions(40, 90, 14, seed=6, zipf=True)
    for opt in (0, OPT_ADAM):
        hp = hparams(90, 12, 32, int(ModelKind.LSTM_COUPLED), LOSS_WARP, epochs=2, B=5, opt=opt, lr=0.05)
        a = Model(hp)
        a.fit(ptr, it)
        path = str(tmp_path / f"m{opt}.npz")
        sbr.persistence.save_model(a, path)
        b = sbr.persistence.load_engine(path)
        assert b.counters() == a.counters()
        for p in Param:
            assert_same_bits(a.get_param(p), b.get_param(p), f"reload {p.name}")
        u = np.array([3, 1, 4, 1, 5], dtype=np.uint32)
        assert_same_bits(a.user_representation(u), b.user_representation(u), "reload user_representation")
        # the model RNG travels with the model (as the reference's serialised Hyperparameters.rng does): the
        # restored model's next fit is the one the original runs — same shuffles, same partition seeds
        assert b.get_rng() == a.get_rng() != bytes(hp.seed)
        assert sbr.persistence.load_engine(str(tmp_path / f"m{opt}")).counters() == a.counters()  # suffix optional
        a.fit(ptr, it), b.fit(ptr, it)
        for p in Param:
            assert_same_bits(a.get_param(p), b.get_param(p), f"resumed {p.name}")
        assert b.get_rng() == a.get_rng()


def test_save_load_multi_replica_model_continues(tmp_path):
    """A model built with num_threads(2) (two replicas in one process, sbr_group_fit) is saved, restored as two
    replicas and continues training exactly like the original."""
    import sbr_rs_amd as sbr

    ptr, it = synthetic_interactions(60, 120, 14, seed=16, zipf=True)
    comp = sbr.data.CompressedInteractions(60, 120, ptr, it, np.zeros(len(it), dtype=np.uint64))

    def build():
        return (sbr.ewma.Hyperparameters.new(120, 12).from_seed(bytes([7] * 16)).embedding_dim(32).learning_rate(0.16)
                .l2_penalty(0.0004).loss(sbr.Loss.Hinge).optimizer(sbr.Optimizer.Adagrad).num_epochs(2).num_threads(2)
                .batch_sequences(6).build())

    a = build()
    a.fit(comp)
    sbr.persistence.save_model(a, str(tmp_path / "two"))
    b = sbr.persistence.load_model(str(tmp_path / "two"))
    assert len(b._replicas()) == 2 and b.params.get_rng() == a.params.get_rng()
    la, lb = a.fit(comp), b.fit(comp)
    assert la == lb
    for ra, rb in zip(a._replicas(), b._replicas()):
        for p in (Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_BIAS, Param.EWMA_ALPHA):
            assert_same_bits(ra.get_param(p), rb.get_param(p), f"resumed replica {p.name}")


def test_save_load_partitioned_model_stays_partitioned(tmp_path):
    """A model whose item table is partitioned over its replicas comes back with ONE copy of the table (not n full
    tables) and continues training exactly like the original."""
    import sbr_rs_amd as sbr

    ptr, it = synthetic_interactions(60, 1300, 14, seed=18, zipf=True)
    comp = sbr.data.CompressedInteractions(60, 1300, ptr, it, np.zeros(len(it), dtype=np.uint64))

    def build():
        return (sbr.ewma.Hyperparameters.new(1300, 12).from_seed(bytes([9] * 16)).embedding_dim(64).learning_rate(0.16)
                .l2_penalty(0.0004).loss(sbr.Loss.Hinge).optimizer(sbr.Optimizer.Adagrad).num_epochs(2).num_threads(2)
                .partition_item_table(True).batch_sequences(6).build())

    a = build()
    a.fit(comp)
    sbr.persistence.save_model(a, str(tmp_path / "part"))
    b = sbr.persistence.load_model(str(tmp_path / "part"))
    assert len(b._replicas()) == 2 and all(r.is_partitioned() for r in b._replicas())
    for p in (Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_BIAS, Param.ITEM_BIAS_ACC, Param.EWMA_ALPHA):
        assert_same_bits(a.params.get_param(p), b.params.get_param(p), f"reloaded {p.name}")
    assert a.fit(comp) == b.fit(comp)
    for ra, rb in zip(a._replicas(), b._replicas()):
        for p in (Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_BIAS, Param.EWMA_ALPHA, Param.EWMA_ALPHA_ACC):
            assert_same_bits(ra.get_param(p), rb.get_param(p), f"resumed partitioned replica {p.name}")


def test_asynchronous_over_a_partitioned_table_is_the_synchronous_step():
    """Parallelism::Asynchronous has no staleness-one pipeline over a partitioned table (owners update in place after a
    rendezvous): it runs — never refuses — and equals the Synchronous oracle bit for bit."""
    from sbr_rs_amd.engine import group_create, group_fit

    items, T, world = 1237, 12, 3
    ptr, it = synthetic_interactions(110, items, T + 5, seed=33, zipf=True)
    mk = lambda par: hparams(items, T, 32, int(ModelKind.EWMA), LOSS_WARP, epochs=2, B=5, ndev=world, par=par)
    models = group_create(mk(PAR_ASYNC), world, partition_item_table=True)
    o = OracleModel(mk(PAR_SYNC))
    assert group_fit(models, ptr, it) == pytest.approx(o.fit(ptr, it), rel=1e-6)
    for q in range(world):
        assert_params_equal(models[q], o, ModelKind.EWMA, f"partitioned + Asynchronous, rank {q}")


def test_batch_of_one_is_per_sequence_sgd():
    ptr, it = synthetic_interactions(20, 80, 12, seed=4)
    hp = hparams(80, 10, 32, int(ModelKind.LSTM_NORMAL), LOSS_WARP, B=1, epochs=1)
    g, o = make_pair(hp)
    g.fit(ptr, it), o.fit(ptr, it)
    assert_params_equal(g, o, ModelKind.LSTM_NORMAL, "B=1")


def test_popular_item_collisions():
    """Few items, many rows: long duplicate segments in the sparse update."""
    ptr, it = synthetic_interactions(64, 7, 40, seed=8)
    for kind in (ModelKind.EWMA, ModelKind.LSTM_NORMAL):
        hp = hparams(7, 32, 32, int(kind), LOSS_WARP, B=64, epochs=2)
        g, o = make_pair(hp)
        g.fit(ptr, it), o.fit(ptr, it)
        assert_params_equal(g, o, kind, "collisions")


def test_ragged_and_minimum_lengths():
    # users of length 1, 2 (dropped), 3 (minimum kept), exactly T, T+1 (chunks 1+T -> the 1 is dropped), 2T+3
    T = 8
    lens = [1, 2, 3, T, T + 1, 2 * T + 3, 3, 3, T + 3, 5]
    ptr = np.zeros(len(lens) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(lens)
    it = np.random.RandomState(2).randint(0, 40, size=int(ptr[-1])).astype(np.uint32)
    for kind in (ModelKind.EWMA, ModelKind.LSTM_COUPLED):
        hp = hparams(40, T, 32, int(kind), LOSS_HINGE, B=4, epochs=2)
        g, o = make_pair(hp)
        g.fit(ptr, it), o.fit(ptr, it)
        assert_params_equal(g, o, kind, "ragged")


def test_empty_interactions_error():
    """≙ lstm.rs:522-530: fit on empty data returns FittingError::NoInteractions."""
    hp = hparams(100, 100, 16, int(ModelKind.LSTM_COUPLED), LOSS_BPR, B=4)
    g = Model(hp)
    ptr = np.zeros(101, dtype=np.uint64)
    with pytest.raises(FittingError.NoInteractions):
        g.fit(ptr, np.zeros(0, dtype=np.uint32))
    # only sequences of length <= 2
    ptr2 = np.arange(0, 202, 2, dtype=np.uint64)
    with pytest.raises(FittingError):
        g.fit(ptr2, np.zeros(200, dtype=np.uint32))


def test_non_finite_prediction_error():
    """≙ sequence_model.rs:225-229: a non-finite score fails predict / mrr_score."""
    hp = hparams(30, 8, 16, int(ModelKind.EWMA), LOSS_HINGE, B=4)
    g = Model(hp)
    b = np.zeros(30, np.float32)
    b[7] = np.inf
    g.set_param(Param.ITEM_BIAS, b)
    u = g.user_representation([1, 2, 3])
    with pytest.raises(PredictionError.InvalidPredictionValue):
        g.predict(u, np.arange(30, dtype=np.uint32))
    ptr, it = synthetic_interactions(5, 30, 8, seed=1)
    with pytest.raises(PredictionError):
        g.mrr_score(ptr, it)
    assert np.all(np.isfinite(g.predict(u, np.array([0, 1, 2], dtype=np.uint32))))


@pytest.mark.parametrize("kind,loss,d,opt", [
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 48, 0),
    (ModelKind.LSTM_COUPLED, LOSS_BPR, 20, 1),
    (ModelKind.EWMA, LOSS_HINGE, 100, 0),
    (ModelKind.EWMA, LOSS_WARP, 7, 1),
])
def test_any_embedding_dim_fit_predict_mrr(kind, loss, d, opt):
    """The reference's builder takes any embedding_dim (lstm.rs:86-89).  Other widths than 16..256 in powers of two
    are stored zero-padded; parameters, representations and predictions keep the caller's width, the fit equals the
    oracle's bit for bit, and the padding is still zero afterwards (the fixed point the definition rests on)."""
    items, T = 130, 12
    ptr, it = synthetic_interactions(50, items, T + 4, seed=23, zipf=True)
    hp = hparams(items, T, d, int(kind), loss, B=8, epochs=3, opt=opt)
    g, o = make_pair(hp)
    assert g.param_count(Param.ITEM_EMBEDDING) == items * d
    lg, lo = g.fit(ptr, it), o.fit(ptr, it)
    assert lg == pytest.approx(lo, rel=1e-6)
    assert_params_equal(g, o, kind, "after fit")
    assert o.padding_is_zero()
    hist = np.array([3, 5, 8, 13], dtype=np.uint32)
    ug, uo = g.user_representation(hist), o.user_representation(hist)
    assert ug.shape == (d,)
    assert_same_bits(ug, uo, "user representation")
    ids = np.arange(items, dtype=np.uint32)
    assert_same_bits(g.predict(ug, ids), o.predict(uo, ids), "predict")
    mg, rg = g.mrr_score(ptr, it)
    mo, ro = o.mrr_score(ptr, it)
    assert np.array_equal(rg, ro) and mg == mo
    # set_param round trip in the caller's shapes
    E = g.get_param(Param.ITEM_EMBEDDING)
    g.set_param(Param.ITEM_EMBEDDING, E)
    assert_same_bits(g.get_param(Param.ITEM_EMBEDDING), E, "E round trip")


def test_invalid_arguments():
    for bad_dim in (0, 257):
        with pytest.raises(EngineError):
            Model(hparams(10, 8, bad_dim, int(ModelKind.EWMA), LOSS_HINGE))  # embedding_dim 1..256
    g = Model(hparams(10, 8, 16, int(ModelKind.EWMA), LOSS_HINGE))
    with pytest.raises(EngineError):
        g.predict(np.zeros(16, np.float32), np.array([10], dtype=np.uint32))  # item id out of range


@pytest.mark.parametrize("kind,d,items,users", [
    (ModelKind.EWMA, 128, 5003, 700),     # several 128-user tiles, ragged item range
    (ModelKind.LSTM_NORMAL, 32, 1683, 180),
    (ModelKind.LSTM_COUPLED, 256, 999, 37),
    (ModelKind.EWMA, 16, 70, 300),        # fewer items than one workgroup's range
])
def test_mrr_gemm_ranks_bit_exact(kind, d, items, users):
    """mrr_score through the MFMA scoring kernel: ranks (integers) and MRR equal the oracle's."""
    T = 24
    hp = hparams(items, T, d, int(kind), LOSS_HINGE, B=16)
    g, o = make_pair(hp)
    rs = np.random.RandomState(d)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    E[rs.randint(0, items, 20)] = E[0]  # exact score ties
    bias = np.round(rs.randn(items) * 0.5, 1).astype(np.float32)
    for m in (g, o):
        m.set_param(Param.ITEM_EMBEDDING, E)
        m.set_param(Param.ITEM_BIAS, bias)
    ptr, it = synthetic_interactions(users, items, 3 * T, seed=77, min_len=1, zipf=True)
    mg, rg = g.mrr_score(ptr, it)
    mo, ro = o.mrr_score(ptr, it)
    assert rg.shape == ro.shape and rg.size > users // 2
    assert np.array_equal(rg, ro)
    assert mg == mo


def test_test_item_in_history_ranks_last():
    """evaluation.rs:30-41: a test item that also occurs in the history is masked => rank = #items."""
    hp = hparams(20, 8, 16, int(ModelKind.EWMA), LOSS_HINGE, B=4)
    g, o = make_pair(hp)
    ptr = np.array([0, 4, 9], dtype=np.uint64)
    it = np.array([3, 5, 7, 5, 1, 2, 2, 4, 6], dtype=np.uint32)
    mg, rg = g.mrr_score(ptr, it)
    mo, ro = o.mrr_score(ptr, it)
    assert rg[0] == 20 and np.array_equal(rg, ro) and mg == mo


@pytest.mark.parametrize("kind,loss,B,bound", [
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 16, 0.089),   # BASELINE.json configs[1]; reference bound lstm.rs:514-519 (CI branch)
    (ModelKind.EWMA, LOSS_HINGE, 16, 0.091),         # reference bound ewma.rs:478-483 (CI branch)
    (ModelKind.LSTM_NORMAL, LOSS_HINGE, 1, 0.091),   # the reference's per-sequence SGD, lstm.rs:466-471 (CI branch)
])
def test_movielens_fit_bit_exact_and_mrr(kind, loss, B, bound):
    """MovieLens-100K under the reference's protocol (lstm.rs:427-448, 498-520): 10 epochs,
    dim 32, lr 0.16, l2 4e-4, Adagrad.  The GPU fit must equal the oracle's bit for bit, ranks and
    MRR included, and clear the reference's own MRR lower bound (the MKL_CBWR=AVX branch its CI runs)."""
    data, train, test, rng = movielens_protocol()
    hp = hparams(data.num_items(), 128, 32, int(kind), loss, epochs=10, B=B, seed=rng.state_seed())
    g, o = make_pair(hp)
    lg = g.fit(train.user_pointers, train.item_ids)
    lo = o.fit(train.user_pointers, train.item_ids)
    assert_params_equal(g, o, kind, "movielens")
    assert lg == pytest.approx(lo, rel=1e-6)
    mg, rg = g.mrr_score(test.user_pointers, test.item_ids)
    mo, ro = o.mrr_score(test.user_pointers, test.item_ids)
    assert np.array_equal(rg, ro) and mg == mo
    assert mg > bound


@pytest.mark.parametrize("kind,loss,d,mode,items,opt", [
    (ModelKind.EWMA, LOSS_HINGE, 32, "single", 9, 0),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, "single", 9, 0),
    (ModelKind.LSTM_COUPLED, LOSS_BPR, 16, "replicated", 9, 0),
    (ModelKind.EWMA, LOSS_WARP, 64, "partitioned", 9, 0),
    # mixed segment lengths, and Adam, on the chunked path
    (ModelKind.EWMA, LOSS_HINGE, 256, "single", 120, OPT_ADAM),
    (ModelKind.LSTM_COUPLED, LOSS_WARP, 64, "replicated", 120, OPT_ADAM),
    (ModelKind.LSTM_NORMAL, LOSS_BPR, 32, "partitioned", 120, OPT_ADAM),
])
def test_hot_rows_take_the_chunked_reduction(kind, loss, d, mode, items, opt):
    """A tiny catalogue under a big minibatch: every row collects far more than SBR_SEG_CHUNK (256)
    entries per step, some thousands — the long-segment path (parallel chunk partials, in-order
    combination) of all three consumers of the sparse reduction, bit for bit against the oracle's
    sequential statement of the same chunked order.

    9 items: every segment is longer than 256 entries (0 / 0 / 9 segments in the length classes <= 32 / 33..256 / > 256).
    120 Zipf items with the same users, T and B (a numpy census of the keys): on one device 9 198 keys per step and
    14 / 102 / 4 segments in the three classes; on three devices about 6 000 keys per device and step and 69 / 48 / 3
    segments.  So all three classes occur — the 33..256 class is routed to the chunk kernels as a single chunk — and a
    step stays above the 4 096 keys up to which the reduction is a single launch.  These cases run Adam, which
    otherwise never meets the chunk partials' combination or the owners' long rows."""
    from sbr_rs_amd.engine import group_create, group_fit

    T, users = 14, 700
    ptr, it = synthetic_interactions(users, items, T + 3, seed=41, zipf=True)
    world = 1 if mode == "single" else 3
    hp = hparams(items, T, d, int(kind), loss, epochs=2, B=400, ndev=world, opt=opt, lr=0.02 if opt == OPT_ADAM else 0.16)
    o = OracleModel(hp)
    lo = o.fit(ptr, it)
    if mode == "single":
        g = Model(hp)
        lg = g.fit(ptr, it)
        models = [g]
    else:
        models = group_create(hp, world, partition_item_table=mode == "partitioned")
        lg = group_fit(models, ptr, it)
    assert lg == pytest.approx(lo, rel=1e-6)
    for q, m in enumerate(models):
        assert_params_equal(m, o, kind, f"hot rows {mode} replica {q}")


def test_dense_gradient_wide_address_path(monkeypatch):
    """The dense-gradient GEMM reads H through a buffer resource while H is below 2 GiB and through 64-bit per-lane
    addresses beyond; SBR_DW_WIDE_ADDRESSES forces the second path at a size the oracle can follow."""
    monkeypatch.setenv("SBR_DW_WIDE_ADDRESSES", "1")
    users, items, T, B = 1500, 901, 9, 1400
    ptr, it = synthetic_interactions(users, items, T, seed=71, min_len=3)
    for kind, loss in ((ModelKind.LSTM_NORMAL, LOSS_HINGE), (ModelKind.LSTM_COUPLED, LOSS_WARP)):
        hp = hparams(items, T, 128, int(kind), loss, epochs=1, B=B)
        g, o = make_pair(hp)
        assert g.fit(ptr, it) == pytest.approx(o.fit(ptr, it), rel=1e-6)
        assert_params_equal(g, o, kind, "wide addresses")


@pytest.mark.parametrize("kind,loss,d,rt", [
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, "1"),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, "2"),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, "4"),
    (ModelKind.LSTM_COUPLED, LOSS_HINGE, 64, "1"),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 32, "1"),
    (ModelKind.LSTM_COUPLED, LOSS_BPR, 16, "1"),
    (ModelKind.LSTM_COUPLED, LOSS_HINGE, 64, "2"),
    (ModelKind.LSTM_COUPLED, LOSS_HINGE, 64, "4"),
    (ModelKind.EWMA, LOSS_WARP, 256, None),
])
@pytest.mark.parametrize("stream", ["0", "1"])
def test_many_tiles_per_minibatch(monkeypatch, kind, loss, d, rt, stream):
    """A minibatch of 9 000 sequences = 282 tiles of 32 sequences: more than the 256 slots over which the
    sequence-resident kernels fold their length-sorted tile list (second fold group reversed), 40+ chunks of
    1 024 packed rows in the dense-gradient GEMM, and a sparse update with ~10^5 keys — the regime the
    benchmark runs in, at a size the oracle still finishes in seconds.  Whole-fit parity, bit for bit, in both
    forms of the sequence-resident kernels (SBR_SEQ_RT: 16- / 32- / 64-sequence tiles)."""
    monkeypatch.setenv("SBR_STREAM", stream)  # the forward pass's stores and the score kernels' gathers streaming / cached: same bits
    if rt is not None:
        monkeypatch.setenv("SBR_SEQ_RT", rt)
    users, items, T, B = 9500, 4001, 7, 9000
    ptr, it = synthetic_interactions(users, items, T, seed=53, min_len=3)
    hp = hparams(items, T, d, int(kind), loss, epochs=1, B=B)
    g, o = make_pair(hp)
    lg, lo = g.fit(ptr, it), o.fit(ptr, it)
    assert lg == pytest.approx(lo, rel=1e-6)
    assert_params_equal(g, o, kind, "many tiles")
    assert_lagged_equal(g, o, "many tiles")  # 9 000 sequences per step: the chain kernel on the sorter stream


@pytest.mark.parametrize("kind,loss,d,B,T", [
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 32, 1, 40),    # the reference's own schedule: one subsequence per optimiser step
    (ModelKind.LSTM_COUPLED, LOSS_HINGE, 32, 1, 17),
    (ModelKind.LSTM_NORMAL, LOSS_BPR, 16, 1, 23),
    (ModelKind.LSTM_COUPLED, LOSS_WARP, 16, 3, 9),
    (ModelKind.LSTM_NORMAL, LOSS_HINGE, 32, 7, 12),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 32, 64, 30),
])
@pytest.mark.parametrize("wave", ["1", "0"])
def test_wave_per_sequence_form(monkeypatch, kind, loss, d, B, T, wave):
    """Small minibatches at d <= 32 run the recurrent pass with one wave per sequence on the vector ALU (sbr_wave.hip);
    SBR_WAVE = 0 forces the MFMA tile kernels instead.  Whole-fit parity with the oracle, bit for bit, in both forms
    (so the two forms agree with each other too), over ragged lengths including length-2 subsequences."""
    monkeypatch.setenv("SBR_WAVE", wave)
    users, items = 60, 301
    ptr, it = synthetic_interactions(users, items, T, seed=91 + d + B, min_len=2)
    hp = hparams(items, T, d, int(kind), loss, epochs=2, B=B)
    g, o = make_pair(hp)
    lg, lo = g.fit(ptr, it), o.fit(ptr, it)
    assert lg == pytest.approx(lo, rel=1e-6)
    assert_params_equal(g, o, kind, f"wave={wave}")


@pytest.mark.parametrize("kind,loss,d,B", [
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 32, 300),
    (ModelKind.LSTM_COUPLED, LOSS_HINGE, 32, 64),
    (ModelKind.LSTM_NORMAL, LOSS_BPR, 16, 150),
    (ModelKind.LSTM_COUPLED, LOSS_WARP, 16, 301),
])
@pytest.mark.parametrize("form", ["1", "0"])
def test_dense_gradient_block_form(monkeypatch, kind, loss, d, B, form):
    """Small steps at d <= 32 form the dense gradient with one wave per 32 x 32 output block (sbr_wave.hip:
    lstm_dw_block_kernel); SBR_DW_BLOCK = 0 forces the 128 x 128 tile kernel.  Several 1 024-row chunks per step, a ragged
    last chunk with an odd row count, first-step rows (h_{-1} = 0) everywhere: whole-fit parity, bit for bit, in both forms."""
    monkeypatch.setenv("SBR_DW_BLOCK", form)
    users, items, T = 700, 401, 14
    ptr, it = synthetic_interactions(users, items, T, seed=33 + d, min_len=2)
    hp = hparams(items, T, d, int(kind), loss, epochs=1, B=B)
    g, o = make_pair(hp)
    assert g.fit(ptr, it) == pytest.approx(o.fit(ptr, it), rel=1e-6)
    assert_params_equal(g, o, kind, f"dense gradient block form={form}")


def test_small_step_with_a_hot_row():
    """Up to 4 096 keys the sparse reduction is ONE launch: a row with more than SBR_SEG_CHUNK = 256 entries is reduced in
    place, chunk partial by chunk partial, instead of going through the three kernels of the chunked path.  A catalogue of
    three items and 140-step sequences gives every step rows with hundreds of entries."""
    users, items, T = 6, 3, 140
    ptr, it = synthetic_interactions(users, items, T, seed=17, min_len=120)
    for kind, loss, d, B in ((ModelKind.LSTM_NORMAL, LOSS_WARP, 32, 1), (ModelKind.EWMA, LOSS_HINGE, 64, 2), (ModelKind.LSTM_COUPLED, LOSS_BPR, 128, 3)):
        hp = hparams(items, T, d, int(kind), loss, epochs=2, B=B)
        g, o = make_pair(hp)
        assert g.fit(ptr, it) == pytest.approx(o.fit(ptr, it), rel=1e-6)
        assert_params_equal(g, o, kind, "hot row in a small step")


@pytest.mark.parametrize("kind,d", [(ModelKind.LSTM_NORMAL, 32), (ModelKind.LSTM_COUPLED, 16)])
def test_wave_form_walks_long_sequences_in_segments(monkeypatch, kind, d):
    """The wave form stages 128 time steps of a sequence in LDS at a time and carries the recurrence's state in registers
    from segment to segment: 300-step sequences (three segments each way, the last one ragged) against the oracle."""
    monkeypatch.setenv("SBR_WAVE", "1")
    users, items, T = 12, 101, 300
    ptr, it = synthetic_interactions(users, items, T, seed=5, min_len=250)
    hp = hparams(items, T, d, int(kind), LOSS_WARP, epochs=1, B=2)
    g, o = make_pair(hp)
    assert g.fit(ptr, it) == pytest.approx(o.fit(ptr, it), rel=1e-6)
    assert_params_equal(g, o, kind, "long sequences")


@pytest.mark.parametrize("wave", ["1", "0"])
@pytest.mark.parametrize("kind", [ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED])
def test_non_finite_inputs_propagate_through_the_recurrent_pass(monkeypatch, kind, wave):
    """A NaN (or an infinity) in an embedding row reaches the hidden state as the oracle says it does — in the tile form and in
    the wave form, whose packed tanh clamps with v_med3_f32 + an unordered comparison instead of two comparison + select pairs."""
    monkeypatch.setenv("SBR_WAVE", wave)
    items, d = 40, 32
    hp = hparams(items, 12, d, int(kind), LOSS_HINGE, B=1)
    g, o = make_pair(hp)
    E = g.get_param(Param.ITEM_EMBEDDING).copy().reshape(items, d)
    E[3, 5] = np.nan
    E[7, 0] = np.inf
    E[9, 1] = -np.inf
    for m in (g, o):
        m.set_param(Param.ITEM_EMBEDDING, E)
    for seq in ([1, 3, 5], [2, 4, 6, 8], [7, 1], [9, 2, 2], [1, 2, 3, 4, 5, 6]):
        hg, ho = g.user_representation(np.array(seq, np.uint32)), o.user_representation(np.array(seq, np.uint32))
        assert np.array_equal(np.isnan(hg), np.isnan(ho)), seq
        fin = ~np.isnan(ho)
        assert np.array_equal(hg[fin].view(np.uint32), ho[fin].view(np.uint32)), seq


def test_full_size_properties():
    """BASELINE.json configs[2] at full size (100 000 users x 1 000 000 items, len <= 64, d = 128, LSTM +
    WARP, 50 000 sequences per step) is far beyond what the oracle can run, so the checks are
    size-independent properties: the fit is deterministic (two runs, identical bits of the 488 MiB table),
    interactions are conserved (examples == sum(len - 1) over the subsequences), the WARP search scores
    between 1 and 5 negatives per interaction, the same fit over a table held in mapped (virtual-memory)
    pages gives the same bits, and rows that nothing can have touched keep their initial value."""
    import zlib

    from bench import synthetic_csr
    from sbr_rs_amd.engine import group_create, group_fit

    users, items, T, d, B = 100_000, 1_000_000, 64, 128, 50_000
    ptr, it = synthetic_csr(users, items, T)
    hp = hparams(items, T, d, int(ModelKind.LSTM_NORMAL), LOSS_WARP, epochs=1, B=B)

    def run():
        m = Model(hp)
        e0 = m.get_param(Param.ITEM_EMBEDDING)
        plan = m.fit_begin(ptr, it)
        nmb = plan.epoch_prepare()
        for mb in range(nmb):
            plan.step(mb)
        ex, neg = plan.counters()
        loss, ex_end = plan.end()
        plan.close()
        e1 = m.get_param(Param.ITEM_EMBEDDING)
        m.close()
        return e0, e1, ex, neg, loss, nmb

    e0, e1, ex, neg, loss, nmb = run()
    lens = np.diff(ptr.astype(np.int64))
    assert nmb == 2 and ex == int((lens - 1).sum())            # every user is one subsequence here (len <= T)
    assert ex <= neg <= 5 * ex and np.isfinite(loss) and loss > 0
    changed = np.flatnonzero((e0.reshape(items, d) != e1.reshape(items, d)).any(axis=1))
    assert 0.5 * items < len(changed) <= items                  # ~3.2 M + negatives entries over 1 M rows
    _, e1b, ex_b, neg_b, loss_b, _ = run()
    assert (ex_b, neg_b) == (ex, neg) and loss_b == pytest.approx(loss, rel=1e-6)
    assert zlib.crc32(e1b.tobytes()) == zlib.crc32(e1.tobytes()), "two identical fits differ"
    # one replica whose table lives in a mapped virtual range (the partitioned layout with a single owner)
    g = group_create(hp, 1, partition_item_table=True)
    group_fit(g, ptr, it)
    assert zlib.crc32(g[0].get_param(Param.ITEM_EMBEDDING).tobytes()) == zlib.crc32(e1.tobytes())
    g[0].close()


@pytest.mark.parametrize("kind,d,T", [(ModelKind.LSTM_NORMAL, 128, 300), (ModelKind.EWMA, 32, 300), (ModelKind.LSTM_COUPLED, 256, 300),
                                      (ModelKind.LSTM_NORMAL, 128, 256), (ModelKind.LSTM_COUPLED, 64, 200), (ModelKind.LSTM_NORMAL, 32, 257),
                                      (ModelKind.LSTM_NORMAL, 16, 1024), (ModelKind.LSTM_COUPLED, 16, 1030),
                                      (ModelKind.LSTM_NORMAL, 64, 1100), (ModelKind.LSTM_COUPLED, 128, 1040)])  # d > 32 beyond 1 024: the tile path's per-step kernels
def test_long_sequences(kind, d, T):
    """max_sequence_length up to 1030 with users of up to 700 (T <= 300) or 2 500 interactions: several chunks per
    user (short chunk first, data.rs:406-431), minibatches whose tiles differ in length by two orders of magnitude.
    T <= 1024: up to 1 023 dependent time steps inside one launch of the sequence-resident kernels, the longest they
    take; beyond that (and for the d = 256 forward pass) the per-step kernels."""
    ptr, it = synthetic_interactions(40 if T <= 300 else 12, 500, 700 if T <= 300 else 2500, seed=61, min_len=1, zipf=True)
    hp = hparams(500, T, d, int(kind), LOSS_WARP, epochs=1, B=16)
    g, o = make_pair(hp)
    assert g.fit(ptr, it) == pytest.approx(o.fit(ptr, it), rel=1e-6)
    assert_params_equal(g, o, kind, "long sequences")
    hist = it[int(ptr[3]):int(ptr[4])]
    assert_same_bits(g.user_representation(hist), o.user_representation(hist), "user_representation of a long history")


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("SBR_FUZZ_SEEDS", "24"))))
def test_randomised_configurations(seed):
    """Seeded sweep over the configuration space the fixed cases only sample: model kind, loss, optimiser,
    dimension, sequence cap, minibatch, catalogue size (tiny = hot rows, large = sparse), number of
    devices and how they are driven (single model, replicated group, partitioned group), parallelism,
    hyper-parameters.  Whole-fit parity, bit for bit, plus ranks."""
    from sbr_rs_amd.engine import group_create, group_fit

    rs = np.random.RandomState(1000 + seed)
    kind = [ModelKind.EWMA, ModelKind.LSTM_NORMAL, ModelKind.LSTM_COUPLED][rs.randint(3)]
    loss = [LOSS_BPR, LOSS_HINGE, LOSS_WARP][rs.randint(3)]
    opt = OPT_ADAM if rs.rand() < 0.3 else 0
    d = [16, 32, 64, 128, 256][rs.randint(5)]
    T = int(rs.randint(3, 20))
    B = int(rs.choice([1, 3, 8, 37, 200]))
    items = int(rs.choice([5, 40, 300, 5000]))
    users = int(rs.randint(20, 140))
    world = int(rs.choice([1, 1, 2, 3]))
    mode = "single" if world == 1 else ["replicated", "partitioned"][rs.randint(2)]
    par = PAR_ASYNC if (mode == "replicated" and rs.rand() < 0.5) else PAR_SYNC
    lr = float(rs.choice([0.01, 0.05, 0.16])) if opt == 0 else 0.01
    l2 = float(rs.choice([0.0, 1e-4, 4e-4]))
    epochs = int(rs.randint(1, 4))
    ptr, it = synthetic_interactions(users, items, T + int(rs.randint(0, 6)), seed=seed, min_len=int(rs.randint(1, 4)),
                                     zipf=bool(rs.randint(2)))
    tptr, tit = synthetic_interactions(12, items, T + 2, seed=seed + 77, min_len=1)
    if rs.rand() < 0.35:  # an embedding_dim that is stored zero-padded (drawn last: the other draws of a seed stay what they were)
        d = int(rs.choice([5, 24, 48, 100, 200]))
    hp = hparams(items, T, d, int(kind), loss, lr=lr, l2=l2, epochs=epochs, B=B, ndev=world, opt=opt, par=par)
    what = f"seed {seed}: {kind.name} loss {loss} opt {opt} d {d} T {T} B {B} items {items} users {users} {mode} x{world} par {par}"
    o = OracleModel(hp)
    try:
        lo = o.fit(ptr, it)
    except OracleError as e:  # e.g. fewer subsequences than devices, or none longer than two items
        with pytest.raises((EngineError, FittingError)):
            (Model(hp).fit(ptr, it) if mode == "single" else group_fit(group_create(hp, world, mode == "partitioned"), ptr, it))
        return
    if mode == "single":
        models = [Model(hp)]
        lg = models[0].fit(ptr, it)
    else:
        models = group_create(hp, world, partition_item_table=mode == "partitioned")
        lg = group_fit(models, ptr, it)
    assert lg == pytest.approx(lo, rel=1e-6, abs=1e-9), what
    for m in models:
        assert_params_equal(m, o, kind, what)
        assert_lagged_equal(m, o, what)
    mg, rg = models[-1].mrr_score(tptr, tit)
    mo, ro = o.mrr_score(tptr, tit)
    assert np.array_equal(rg, ro) and mg == mo, what


# ---- committed golden vectors: the engine against numbers on disk, no oracle in the loop ------------
class _EngineGroup:
    """Engine-side adapter with the oracle's model surface: one handle, or a single-process group."""

    def __init__(self, hp):
        from sbr_rs_amd.engine import group_create

        self.models = group_create(hp, int(hp.num_devices))

    def fit(self, ptr, it):
        from sbr_rs_amd.engine import group_fit

        return group_fit(self.models, ptr, it)

    def __getattr__(self, name):
        return getattr(self.models[0], name)


@pytest.mark.parametrize("name", ["ewma_hinge_d32", "lstm_warp_d32", "coupled_bpr_adam_d16", "lstm_hinge_two_devices",
                                  "ewma_warp_three_devices_async"])
def test_engine_reproduces_committed_vectors(name):
    import importlib.util
    import os

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_oracle_vectors", os.path.join(golden, "make_oracle_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = np.load(os.path.join(golden, "oracle_vectors.npz"))
    got = mod.run_case(_EngineGroup, name)
    for k in [k.split("/", 1)[1] for k in want.files if k.startswith(name + "/")]:
        a, b = np.asarray(got[k]), want[f"{name}/{k}"]
        if k == "loss":  # f64 sum on the device, order-free: 1e-6 relative
            assert float(a) == pytest.approx(float(b), rel=1e-6)
            continue
        assert a.shape == b.shape, (name, k)
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                              b.view(np.uint32) if b.dtype == np.float32 else b), (name, k)


# ---- the bench's own regime against the oracle, by sampling (tests/sampled_parity.py) ----------------------------------
@pytest.mark.parametrize("name,kind,loss,d,users,items,T,B", [
    # BASELINE configs[2] at full size, the bench's max-batch regime: 1 563 32-sequence tiles (> the 1 024 up to which the tile
    # list is folded), 63-step tiles, the two-pass 20-bit key ordering over 4.9 M keys, ~1 590 dense-gradient chunks
    ("configs2_b50000", ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 100_000, 1_000_000, 64, 50_000),
    # the same workload at the quality-neutral batch the headline is quoted at (16-sequence tiles, folded)
    ("configs2_b8192", ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 100_000, 1_000_000, 64, 8_192),
    # BASELINE configs[3]'s per-GPU shape: 125 000 users, sequences up to 128
    ("configs3_per_gpu", ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 125_000, 1_000_000, 128, 16_384),
    # BASELINE configs[4]'s shape on one GPU: EWMA + hinge, d = 256, 1e7 items (three-pass key ordering, 10 GB table)
    ("ewma256_10M_items", ModelKind.EWMA, LOSS_HINGE, 256, 100_000, 10_000_000, 64, 50_000),
])
def test_bench_regime_first_step_sampled_parity(name, kind, loss, d, users, items, T, B):
    """Every other oracle-checked fit is small (<= 9 500 sequences x 7 steps, or 16 long sequences); the regime bench.py
    measures was covered by determinism and conservation only.  Here the FIRST optimiser step of the bench's own workloads, at
    full size, is compared with the oracle bit for bit by sampling: ~64 sequences across the first / middle / last tiles
    (forward, negatives, trip counts, loss, BPTT), ~256 item rows (the row's whole optimiser step from every entry that touches
    it), 48 elements of the dense gradient as chains over all 1.6 M packed rows, and the dense parameters after the step."""
    import bench
    from sampled_parity import check_first_step, count_subsequences

    ptr, it = bench.synthetic_csr(users, items, T)
    hp = hparams(items, T, d, int(kind), loss, B=B, epochs=1)
    g, o = Model(hp), OracleModel(hp)
    pg, po = g.fit_begin(ptr, it), o.fit_begin(ptr, it)
    assert pg.epoch_prepare() == po.epoch_prepare()

    class Full:
        model = g
        rows = pg.minibatch_rows(0)

        def step_local(self):
            pg.step_local(0)

        def fetch(self, which):
            return pg.debug_fetch(which, self.rows)

        def apply(self):
            pg.step_apply(0)

    nb = min(B, count_subsequences(ptr, T))
    out = check_first_step(Full(), o, po, lstm=kind != ModelKind.EWMA, nb=nb)
    assert out["rows"] > 250_000 and out["sampled_sequences"] >= 60 and out["sampled_items"] >= 200, out
    pg.close(); po.close()


@pytest.mark.parametrize("exchange", ["owner", "gradient"])
def test_bench_regime_multi_device_first_step_sampled_parity(exchange):
    """BASELINE configs[3] at full size — 1e6 users over 8 devices, 1e6 items, sequences to 128, d = 128, LSTM + WARP, 8 192
    sequences per device and step — through the multi-GPU protocol's C-ABI halves with eight simulated ranks on ONE GPU and
    tensor copies in place of the collectives (tests/simulated_ranks.py), in both forms of the Synchronous step: owner-applied
    (scatter into 8 per-owner chunks of 125 000 rows, every owner reduces 8 inputs and updates its 125 000 rows in place, the
    parameter slices are all-gathered into the eight tables; the accumulator slices at the end) and the gradient all-gather
    (owner reduce over 8 inputs, table update from 8 reduced chunks on every replica); dense update from 8 blocks.  The first optimiser step is compared with the oracle by sampling
    (tests/sampled_parity.py::check_first_step_multi): every device's half-step on a sample of its sequences, ~160 item rows'
    device-ordered gradient sums and updates on the first and the last replica, and the dense parameters."""
    import bench
    from sampled_parity import check_first_step_multi, count_subsequences
    from simulated_ranks import SimulatedRanks

    world, users, items, T, d, B = 8, 125_000, 1_000_000, 128, 128, 8_192
    ptr, it = bench.synthetic_csr(users * world, items, T)
    kind, loss = ModelKind.LSTM_NORMAL, LOSS_WARP
    models = [Model(hparams(items, T, d, int(kind), loss, epochs=1, B=B, ndev=world, rank=q)) for q in range(world)]
    plans = [m.fit_begin(ptr, it) for m in models]
    o = OracleModel(hparams(items, T, d, int(kind), loss, epochs=1, B=B, ndev=world, rank=0))
    po = o.fit_begin(ptr, it)
    assert {p.epoch_prepare() for p in plans} == {po.epoch_prepare()}
    ranks = SimulatedRanks(models, plans)

    class Full:
        pass

    f = Full()
    f.world = world
    f.model = lambda q: models[q]
    f.rows = lambda q: plans[q].minibatch_rows(0)
    f.step_local_all = lambda: [plans[q].step_local(0) for q in range(world)]
    f.fetch = lambda q, which: plans[q].debug_fetch(which, f.rows(q))

    def apply_all():
        ranks.exchange(0, exchange)
        ranks.finish()

    f.apply_all = apply_all
    nb = min(B, count_subsequences(ptr, T) // world)
    out = check_first_step_multi(f, o, po, lstm=True, nb=nb)
    assert out["items_touched_by_several_devices"] > 50 and min(out["rows_per_device"]) > 400_000, out
    for p in plans:
        p.close()
    po.close()


@pytest.mark.parametrize("name,kind,loss,d,items,T", [
    # BASELINE configs[4] through its OWN split: 1e6 users over 8 devices, 1e7 items x 256 partitioned over 8 owners
    # (1 250 000 rows = 1.28 GB of embeddings per owner), EWMA + hinge
    ("configs4_ewma256_10M_items", ModelKind.EWMA, LOSS_HINGE, 256, 10_000_000, 64),
    # the LSTM + WARP workload of configs[2]/[3] over a partitioned table: 1e6 items x 128 over 8 owners
    ("lstm_warp_d128_1M_items", ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 1_000_000, 64),
])
def test_bench_regime_partitioned_first_step_sampled_parity(name, kind, loss, d, items, T):
    """The item-table-partitioned step (sbr_group_create(..., SBR_GROUP_PARTITION_ITEM_TABLE): rows [r*S, (r+1)*S) on replica
    r's device, one virtual range mapped into all eight replicas; every replica reduces its own entries per row into a list
    (sparse_reduce_list_kernel), the owners' bounds (owner_bounds_kernel) meet at the host rendezvous, every owner merges the
    eight lists over its rows in device order and updates them in place (owner_list_apply_kernel)) AT SIZE: eight replicas in one
    process on one GPU, 8 x 125 000 users, 8 192 sequences per replica and step.  The first optimiser step is compared with the
    oracle's replicated num_devices = 8 step by sampling (tests/sampled_parity.py::check_first_step_multi): every replica's
    half-step on a sample of its sequences (read through the shared mapping), ~250 item rows' device-ordered gradient sums and
    ONE update — among them the nearest touched row on each side of every ownership change (the seven logical slice starts and
    every physical page run's first row), the last touched rows of the uneven last slice and rows that several devices touch —
    read back from replica 0 and replica 7, and (LSTM) the dense parameters.
    ≙ /root/reference/src/models/ewma.rs:266-352, sequence_model.rs:163-169 over shared HogwildParameter rows (ewma.rs:167-198)."""
    import bench
    from sampled_parity import check_first_step_multi, count_subsequences
    from sbr_rs_amd.engine import GroupPlan, group_create

    world, users, B = 8, 125_000, 8_192
    ptr, it = bench.synthetic_csr(users * world, items, T)
    hp = hparams(items, T, d, int(kind), loss, epochs=1, B=B, ndev=world)
    models = group_create(hp, world, partition_item_table=True)
    assert all(m.is_partitioned() for m in models)
    o = OracleModel(hp)
    po = o.fit_begin(ptr, it)
    gp = GroupPlan(models, ptr, it)
    assert gp.epoch_prepare() == po.epoch_prepare()
    # where the owner of a row changes: logical slices of S = ceil(items / world) rows, and the physical parts of the embedding
    # array (runs of pages homed on one device: a page belongs to the owner of its first row)
    S = (items + world - 1) // world
    boundaries = [k * S for k in range(1, world)]
    off, row_bytes = 0, 4 * models[0].storage_dim
    for home, nbytes in models[0].partition_parts():
        off += nbytes
        if off >= items * row_bytes:
            break
        boundaries.append(off // row_bytes)
    boundaries = sorted(set(boundaries))
    assert len(boundaries) >= world - 1

    class Full:
        pass

    f = Full()
    f.world = world
    f.model = lambda q: models[q]
    f.rows = lambda q: gp.member(q).minibatch_rows(0)
    f.step_local_all = lambda: (gp.step_local(0), gp.synchronize())
    f.fetch = lambda q, which: gp.member(q).debug_fetch(which, f.rows(q))
    f.apply_all = lambda: (gp.step(0), gp.synchronize())
    nb = min(B, count_subsequences(ptr, T) // world)
    out = check_first_step_multi(f, o, po, lstm=kind != ModelKind.EWMA, nb=nb, boundaries=boundaries)
    assert out["items_touched_by_several_devices"] > 30 and min(out["rows_per_device"]) > 200_000, out
    assert len(out["boundary_items"]) >= 2 * (world - 1), out
    for k in range(1, world):  # both sides of every logical owner boundary were compared
        assert any(x < k * S for x in out["boundary_items"]) and any(x >= k * S for x in out["boundary_items"])
    loss_g = gp.end()
    assert np.isfinite(loss_g)
    po.close()


@pytest.mark.parametrize("name,kind,loss,d,items,users,T,B,steps,item_distribution", [
    ("configs2_headline", ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 1_000_000, 100_000, 64, 8_192, 3, "uniform"),
    ("configs2_headline_zipf", ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 1_000_000, 100_000, 64, 8_192, 3, "zipf"),
    ("configs3_per_gpu", ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 1_000_000, 125_000, 128, 8_192, 2, "uniform"),
    ("configs2_max_batch", ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 1_000_000, 100_000, 64, 50_000, 1, "uniform"),
    # configs[4]'s model on one GPU (EWMA + hinge, d = 256; the fused scan + score pass) with a 2e6-item table — the 1e7-item
    # one is covered by the sampled test: comparing 2 x 10 GB of table on the host would be the whole test
    ("ewma256_2M_items", ModelKind.EWMA, LOSS_HINGE, 256, 2_000_000, 100_000, 64, 50_000, 2, "uniform"),
])
def test_bench_regime_whole_steps_full_parity(name, kind, loss, d, items, users, T, B, steps, item_distribution):
    """The bench's own workloads at full size, WHOLE optimiser steps, everything compared: BASELINE configs[2] (100 000 users x
    1e6 items, sequences to 64, d = 128, LSTM + WARP) at the batch the headline is quoted on — three consecutive steps, with both
    item distributions bench.py offers (Zipf: hot rows through the chunked reduction, shorter WARP searches) — configs[3]'s
    per-GPU shape (sequences to 128) for two steps, and one step of the 50 000-sequence regime (`value_max_batch`: 1.6 M rows,
    unfolded tile list, two-pass ordering).  Then EVERY parameter and optimiser accumulator — the whole item table
    included — against the oracle, bit for bit.  The sampled tests above compare intermediates of the first step; this one has
    no sampling and no fresh-state shortcut: later steps start from a touched table and non-zero accumulators, with the previous
    step's ordering and loss chain still in flight on the other streams.  5-30 s of oracle time per step."""
    import bench

    ptr, it = bench.synthetic_csr(users, items, T, zipf=item_distribution == "zipf")
    hp = hparams(items, T, d, int(kind), loss, B=B, epochs=1)
    g, o = make_pair(hp)
    pg, po = g.fit_begin(ptr, it), o.fit_begin(ptr, it)
    assert pg.epoch_prepare() == po.epoch_prepare() >= steps
    rows = 0
    for mb in range(steps):
        assert pg.minibatch_rows(mb) == po.minibatch_rows(mb)
        rows += pg.minibatch_rows(mb)
        pg.step(mb)
        po.step(mb)
    assert rows > steps * 250_000
    (lg, eg), (lo, eo) = pg.end(), po.end()
    assert eg == eo == rows
    assert lg == pytest.approx(lo, rel=1e-6)
    assert bits(np.float32(pg.end_lagged())) == bits(np.float32(po.end_lagged()))
    assert_params_equal(g, o, kind, f"{name}: after {steps} whole steps")
    pg.close(); po.close()


@pytest.mark.parametrize("exchange", ["owner", "gradient"])
def test_bench_regime_two_devices_whole_step_full_parity(exchange):
    """The multi-GPU step at configs[3]'s per-GPU size with no sampling: two devices x 125 000 users, sequences to 128, d = 128,
    LSTM + WARP, 8 192 sequences per device — one whole optimiser step through the protocol's C-ABI halves (two simulated ranks on
    one GPU, tensor copies for the collectives: scatter into two 500 000-row owner chunks, then the owner-applied update + in-place
    all-gather of the parameter and accumulator slices, or owner reduce + table update on both replicas; dense update), then
    every parameter and accumulator of BOTH replicas against the oracle with num_devices = 2.  The eight-device
    step of the full configs[3] is compared by sampling above (its whole step is ~80 s of oracle time)."""
    import bench
    from simulated_ranks import SimulatedRanks

    world, users, items, T, d, B = 2, 125_000, 1_000_000, 128, 128, 8_192
    kind, loss = ModelKind.LSTM_NORMAL, LOSS_WARP
    ptr, it = bench.synthetic_csr(users * world, items, T)
    models = [Model(hparams(items, T, d, int(kind), loss, epochs=1, B=B, ndev=world, rank=q)) for q in range(world)]
    plans = [m.fit_begin(ptr, it) for m in models]
    o = OracleModel(hparams(items, T, d, int(kind), loss, epochs=1, B=B, ndev=world, rank=0))
    po = o.fit_begin(ptr, it)
    assert {p.epoch_prepare() for p in plans} == {po.epoch_prepare()}
    ranks = SimulatedRanks(models, plans)
    rows = sum(plans[q].minibatch_rows(0) for q in range(world))
    assert rows > 900_000
    ranks.step(0, exchange)
    ranks.finish()
    po.step(0)
    lo, eo = po.end()
    for q in range(world):
        assert_params_equal(models[q], o, kind, f"two devices, whole step, rank {q}")
        lg, eg = plans[q].end()
        assert eg == eo == rows and lg == pytest.approx(lo, rel=1e-6)
    for p in plans:
        p.close()
    po.close()


@pytest.mark.parametrize("kind,loss,d,opt,T,items", [
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 32, 0, 12, 300),          # ~10-row steps: the 256-thread tail
    (ModelKind.LSTM_NORMAL, LOSS_HINGE, 32, 0, 128, 1683),       # the reference's bench shape; rows beyond 64: the 1 024-thread tail
    (ModelKind.LSTM_COUPLED, LOSS_BPR, 16, OPT_ADAM, 90, 500),
    (ModelKind.LSTM_COUPLED, LOSS_WARP, 32, OPT_ADAM, 200, 40),  # 40 items: rows repeated many times inside a step
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 16, 0, 300, 97),          # beyond 255 rows: the step falls back to the separate launches
    (ModelKind.EWMA, LOSS_WARP, 32, 0, 100, 211),                # EWMA + WARP: scan, then the score launch with the tail
    (ModelKind.EWMA, LOSS_HINGE, 32, 0, 128, 1683),              # the reference's ewma bench: scan + score + backward scan + tail in one launch
    (ModelKind.EWMA, LOSS_BPR, 16, OPT_ADAM, 60, 50),
])
@pytest.mark.parametrize("fused", [2, 1, 0])
def test_one_sequence_steps_fused_launches(kind, loss, d, opt, T, items, fused):
    """One subsequence per optimiser step (the reference's own schedule, sequence_model.rs:111-169) at d <= 32.  fused = 1: four
    launches per step — forward, score + [header, lagged loss figure, key ordering] (sbr::SmallTail), backward, and [dense gradient
    + dense update + sparse update] (launch_small_back); EWMA with a single-negative loss two: [scan + score + backward scan + tail]
    and [dalpha + its update + sparse update].  fused = 2 (the default): EWMA with a single-negative loss and Adagrad up to 128 rows
    per step runs every epoch's steps in ONE launch (ewma_steps_kernel: one workgroup walks the steps, each step's working set in
    LDS); everything else in the matrix takes the fused launches step by step.  fused = 0: the eight separate launches they
    replace.  Whole fits (two epochs, then a second fit call on the same model) against the oracle, bit for bit, every parameter
    and accumulator, the loss figures, and a representation computed from the re-emitted packed weight copies."""
    ptr, it = synthetic_interactions(14, items, T + 30, seed=31, min_len=3, zipf=True)
    hp = hparams(items, T, d, int(kind), loss, B=1, epochs=2, opt=opt, lr=0.02 if opt else 0.16)
    g, o = Model(hp), OracleModel(hp)
    g.set_step_fusion(fused)
    params = [Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_BIAS, Param.ITEM_BIAS_ACC]
    params += [Param.EWMA_ALPHA, Param.EWMA_ALPHA_ACC] if kind == ModelKind.EWMA else [Param.LSTM_W, Param.LSTM_W_ACC, Param.LSTM_B, Param.LSTM_B_ACC]
    for call in range(2):
        lg, lo = g.fit(ptr, it), o.fit(ptr, it)
        assert abs(lg - lo) <= 1e-6 * abs(lo), (lg, lo)
        assert np.float32(g.last_fit_lagged_loss()).tobytes() == np.float32(o.last_fit_lagged_loss()).tobytes()
        for q in params:
            assert g.get_param(q).tobytes() == o.get_param(q).tobytes(), (call, q)
    hist = it[int(ptr[2]):int(ptr[3])]
    assert g.user_representation(hist).tobytes() == o.user_representation(hist).tobytes()   # (the packed weight copies were re-emitted)


@pytest.mark.parametrize("T,items,users", [(128, 1683, 60), (40, 31, 40), (12, 9, 40)])
@pytest.mark.parametrize("loss", [LOSS_HINGE, LOSS_BPR])
def test_lstm_step_runs_in_one_launch_equal_single_steps(loss, T, items, users):
    """The LSTM's one-launch step runs (lstm_steps_kernel: Normal, d = 32, single-negative loss, Adagrad — the reference's Criterion
    shape): sbr_fit_steps over a whole epoch equals the same steps taken one by one through the four launches, every parameter and
    accumulator and the last step's block, bit for bit.  Steps of more than 48 rows inside the epoch (T = 128: sequences of up to
    127 steps among the short ones) take the separate launches and the run resumes behind them; 31 and 9 items: rows repeated many
    times inside a step."""
    ptr, it = synthetic_interactions(users, items, T + 22, seed=7, min_len=3, zipf=True)
    if T == 128:  # mostly short sequences (the Criterion shape) with a few long ones between them
        lens = np.diff(ptr).astype(np.int64)
        keep = np.where(np.arange(lens.size) % 7 == 0, lens, np.minimum(lens, 3 + np.arange(lens.size) % 30))
        new_ptr = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint64)
        it = np.concatenate([it[int(ptr[u]):int(ptr[u]) + int(keep[u])] for u in range(lens.size)]).astype(np.uint32)
        ptr = new_ptr
    hp = hparams(items, T, 32, int(ModelKind.LSTM_NORMAL), loss, B=1, epochs=1)
    a, b = Model(hp), Model(hp)
    b.set_step_fusion(1)
    pa, pb = a.fit_begin(ptr, it), b.fit_begin(ptr, it)
    for epoch in range(2):
        n = pa.epoch_prepare()
        assert pb.epoch_prepare() == n and n > 12
        pa.steps(0, 5); pa.steps(5, n - 5)
        for mb in range(n):
            pb.step(mb)
    clocks = pa.phase_clocks()
    assert 0 < clocks[5] <= 2 * n and pb.phase_clocks()[5] == 0
    if T != 128:
        assert clocks[5] == 2 * n
    rows = pa.minibatch_rows(n - 1)
    for w in (Debug.IN_IDX, Debug.OUT_IDX, Debug.HIDDEN, Debug.NEGATIVES, Debug.COEF, Debug.DINPUT, Debug.DENSE_GRAD, Debug.LOSS, Debug.TRIES, Debug.DZ):
        assert pa.debug_fetch(w, rows).tobytes() == pb.debug_fetch(w, rows).tobytes(), w
    assert pa.sparse_stats() == pb.sparse_stats()
    assert pa.counters() == pb.counters()
    assert pa.end_lagged() == pb.end_lagged()
    assert pa.end() == pb.end()
    for q in (Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_BIAS, Param.ITEM_BIAS_ACC, Param.LSTM_W, Param.LSTM_W_ACC, Param.LSTM_B, Param.LSTM_B_ACC):
        assert a.get_param(q).tobytes() == b.get_param(q).tobytes(), q
    assert a.counters() == b.counters()
    hist = it[int(ptr[2]):int(ptr[3])]
    assert a.user_representation(hist).tobytes() == b.user_representation(hist).tobytes()   # (the packed weight copies were re-emitted)


@pytest.mark.parametrize("loss,d,T,items", [(LOSS_HINGE, 32, 128, 1683), (LOSS_BPR, 16, 129, 60), (LOSS_HINGE, 32, 12, 9)])
def test_step_runs_in_one_launch_equal_single_steps(loss, d, T, items):
    """sbr_fit_steps over arbitrary runs (a prefix, an empty run, the middle, the rest) equals the same steps taken one by one,
    and the block of the last step stays readable (debug fetch, sparse stats) — the reference's ewma bench shape (T = 128, d = 32,
    hinge, Adagrad), the largest step the one-launch form takes (128 rows, d = 16, BPR), and nine items (every row repeated many
    times inside a step: long segments, bias and row shared by inputs, targets and negatives)."""
    ptr, it = synthetic_interactions(40, items, T + 22, seed=5, min_len=3, zipf=True)
    hp = hparams(items, T, d, int(ModelKind.EWMA), loss, B=1, epochs=1)
    a, b = Model(hp), Model(hp)
    b.set_step_fusion(1)
    pa, pb = a.fit_begin(ptr, it), b.fit_begin(ptr, it)
    n = pa.epoch_prepare()
    assert pb.epoch_prepare() == n and n > 12
    pa.steps(0, 5); pa.steps(5, 0); pa.steps(5, n - 7); pa.steps(n - 2, 2)
    assert pa.phase_clocks()[5] == n   # every step went through the one-launch form
    for mb in range(n):
        pb.step(mb)
    assert pb.phase_clocks()[5] == 0
    rows = pa.minibatch_rows(n - 1)
    for w in (Debug.IN_IDX, Debug.OUT_IDX, Debug.HIDDEN, Debug.NEGATIVES, Debug.COEF, Debug.DINPUT, Debug.DENSE_GRAD, Debug.LOSS, Debug.TRIES):
        assert pa.debug_fetch(w, rows).tobytes() == pb.debug_fetch(w, rows).tobytes(), w
    assert pa.sparse_stats() == pb.sparse_stats()
    assert pa.counters() == pb.counters()
    assert pa.end_lagged() == pb.end_lagged()
    assert pa.end() == pb.end()
    for q in (Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_BIAS, Param.ITEM_BIAS_ACC, Param.EWMA_ALPHA, Param.EWMA_ALPHA_ACC):
        assert a.get_param(q).tobytes() == b.get_param(q).tobytes(), q
    assert a.counters() == b.counters()


@pytest.mark.parametrize("kind,loss,d,T,items", [
    (ModelKind.EWMA, LOSS_HINGE, 16, 6, 57),           # the oracle's own stream test shape: one draw per step
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 32, 40, 23),    # 23 items: long retry runs, windows refilled inside a step
    (ModelKind.LSTM_COUPLED, LOSS_BPR, 16, 128, 400),
    (ModelKind.EWMA, LOSS_WARP, 32, 200, 1683),        # up to 199 rows per step: several 64-draw windows per sequence
    (ModelKind.LSTM_COUPLED, LOSS_HINGE, 64, 50, 150),  # round 6: every kernel width (the MFMA recurrent kernels around the stream scorer)
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 30, 211),
    (ModelKind.EWMA, LOSS_WARP, 128, 221, 1683),       # 220 rows: the most one workgroup's LDS holds at d = 128
    (ModelKind.EWMA, LOSS_HINGE, 256, 24, 97),
    (ModelKind.LSTM_NORMAL, LOSS_BPR, 100, 12, 64),    # embedding_dim 100: the 128-wide model with zero columns
])
def test_reference_order_negatives_follow_the_workers_stream(kind, loss, d, T, items):
    """sbr_model_set_reference_order: the engine draws a step's negatives from the worker's own sequential xorshift128 stream with
    rand 0.5's Uniform — one draw per try, WARP stopping at the first violating candidate, the same generator reshuffling the
    partition every epoch (sequence_model.rs:58-65, :97, :109, :137) — instead of the contract's counter-keyed draws.  Every step's
    negatives and trip counts, and after two fits every parameter, accumulator and loss figure, against the oracle's
    reference-order mode (orc_model_set_reference_order), bit for bit."""
    ptr, it = synthetic_interactions(17, items, T + 25, seed=41, min_len=3, zipf=True)
    hp = hparams(items, T, d, int(kind), loss, B=1, epochs=2)
    g, o = Model(hp), OracleModel(hp)
    g.set_reference_order(True)
    o.set_reference_order(True)
    pg, po = g.fit_begin(ptr, it), o.fit_begin(ptr, it)
    for _ in range(2):
        n = pg.epoch_prepare()
        assert po.epoch_prepare() == n
        for mb in range(n):
            pg.step(mb); po.step(mb)
            rows = pg.minibatch_rows(mb)
            for w in (Debug.IN_IDX, Debug.NEGATIVES, Debug.TRIES):
                assert np.array_equal(pg.debug_fetch(w, rows), po.debug_fetch(w, rows)), (mb, w)
    assert pg.end_lagged() == po.end_lagged()
    pg.end(); po.end()
    assert_params_equal(g, o, kind, "reference order, stepped")
    for call in range(2):  # whole fits continue from the same state on both sides (the model RNG seeds a fresh worker stream)
        lg, lo = g.fit(ptr, it), o.fit(ptr, it)
        assert lg == pytest.approx(lo, rel=1e-6)
        assert_params_equal(g, o, kind, f"reference order, fit call {call}")
        assert_lagged_equal(g, o, f"reference order, fit call {call}")
    with pytest.raises(EngineError):  # the mode is defined for the reference's schedule only
        Model(hparams(items, T, d, int(kind), loss, B=2)).set_reference_order(True)
    with pytest.raises(EngineError):  # ... and for steps whose h rows and candidate window fit one workgroup's LDS
        Model(hparams(items, 128, 256, int(kind), loss, B=1)).set_reference_order(True)


@pytest.mark.parametrize("name,kind,loss", [("lstm hinge 1 thread", ModelKind.LSTM_NORMAL, LOSS_HINGE), ("lstm warp", ModelKind.LSTM_NORMAL, LOSS_WARP),
                                            ("ewma hinge", ModelKind.EWMA, LOSS_HINGE), ("ewma warp", ModelKind.EWMA, LOSS_WARP)])
def test_movielens_protocol_in_reference_order(name, kind, loss):
    """The reference's MovieLens-100K protocol cases with ONE worker (lstm.rs:450-520, ewma.rs:463-507: seed [42; 16], split 0.2,
    d = 32, T = 128, ten epochs, one subsequence per optimiser step) with the ENGINE running the crate's own index stream
    (sbr_model_set_reference_order): parameters and test ranks equal the oracle's reference-order run bit for bit, and the MRR
    clears the floor tests/test_oracle.py asserts for that mode.  (The two-worker case: test_movielens_two_threads_in_reference_order.)"""
    from test_oracle import REFERENCE_ORDER_FLOORS

    data, train, test, rng = movielens_protocol()
    hp = hparams(data.num_items(), 128, 32, int(kind), loss, epochs=10, B=1, seed=rng.state_seed())
    g, o = Model(hp), OracleModel(hp)
    g.set_reference_order(True)
    o.set_reference_order(True)
    lg, lo = g.fit(train.user_pointers, train.item_ids), o.fit(train.user_pointers, train.item_ids)
    assert lg == pytest.approx(lo, rel=1e-6)
    assert_params_equal(g, o, kind, name)
    mg, rg = g.mrr_score(test.user_pointers, test.item_ids)
    mo, ro = o.mrr_score(test.user_pointers, test.item_ids)
    assert np.array_equal(rg, ro) and mg == mo
    assert mg > REFERENCE_ORDER_FLOORS[name], (name, mg)


@pytest.mark.parametrize("kind,loss,d,world,T,items,users", [
    (ModelKind.LSTM_NORMAL, LOSS_HINGE, 32, 2, 128, 1683, 40),   # the shape of the reference's mrr_test_two_threads
    (ModelKind.EWMA, LOSS_WARP, 16, 3, 20, 97, 60),
    (ModelKind.LSTM_NORMAL, LOSS_WARP, 128, 2, 24, 131, 40),     # round 6: beyond d = 32
])
def test_reference_order_several_workers_apply_one_after_the_other(kind, loss, d, world, T, items, users):
    """Reference order with num_threads(n) (Parallelism::Synchronous): every worker draws from its OWN sequential stream, the
    workers rendezvous, and each worker's gradient goes in as its own optimiser step, one after the other in worker order
    (sequence_model.rs:163-166; n Adagrad applications per step) — sbr_group_fit over replicas in reference order
    (sbr_fit_step_apply_blocks_in_order) against the oracle's reference-order run with num_devices = n, every replica, bit for bit."""
    from sbr_rs_amd.engine import group_create, group_fit

    ptr, it = synthetic_interactions(users, items, T + 20, seed=43, min_len=3, zipf=True)
    hp = hparams(items, T, d, int(kind), loss, B=1, epochs=2, ndev=world)
    models = group_create(hp, world)
    for m in models:
        m.set_reference_order(True)
    o = OracleModel(hp)
    o.set_reference_order(True)
    for call in range(2):
        lg, lo = group_fit(models, ptr, it), o.fit(ptr, it)
        assert lg == pytest.approx(lo, rel=1e-6)
        for q in range(world):
            assert_params_equal(models[q], o, kind, f"reference order, {world} workers, call {call}, replica {q}")
            assert_lagged_equal(models[q], o, f"reference order, {world} workers, replica {q}")


def test_movielens_two_threads_in_reference_order():
    """`mrr_test_two_threads` (lstm.rs:473-496: LSTM + hinge, two worker threads, Synchronous) with the engine in reference order:
    two replicas, two sequential streams, two optimiser applications per step — parameters and ranks equal the oracle's
    reference-order run, MRR above the floor recorded for that mode."""
    from sbr_rs_amd.engine import group_create, group_fit
    from test_oracle import REFERENCE_ORDER_FLOORS

    data, train, test, rng = movielens_protocol()
    hp = hparams(data.num_items(), 128, 32, int(ModelKind.LSTM_NORMAL), LOSS_HINGE, epochs=10, B=1, seed=rng.state_seed(), ndev=2)
    models = group_create(hp, 2)
    for m in models:
        m.set_reference_order(True)
    o = OracleModel(hp)
    o.set_reference_order(True)
    lg, lo = group_fit(models, train.user_pointers, train.item_ids), o.fit(train.user_pointers, train.item_ids)
    assert lg == pytest.approx(lo, rel=1e-6)
    for q in range(2):
        assert_params_equal(models[q], o, ModelKind.LSTM_NORMAL, f"two threads, replica {q}")
    mg, rg = models[1].mrr_score(test.user_pointers, test.item_ids)
    mo, ro = o.mrr_score(test.user_pointers, test.item_ids)
    assert np.array_equal(rg, ro) and mg == mo
    assert mg > REFERENCE_ORDER_FLOORS["lstm hinge 2 threads"], mg


@pytest.mark.parametrize("seed", range(16))
def test_step_runs_randomised(seed):
    """Randomised one-sequence-per-step fits through sbr_model_fit (the one-launch step runs where the shape allows, the fused
    launches elsewhere and for the steps a run skips) against the oracle: model (EWMA / LSTM Normal at d = 32, EWMA at d = 16),
    loss (hinge / BPR), max_sequence_length 4..140, catalogues from 5 items (every row repeated inside a step) to 3 000, sequence
    lengths around and across the 48-row cut of the LSTM runs, two epochs and a second fit call — every parameter, accumulator and
    loss figure bit for bit."""
    rs = np.random.RandomState(1000 + seed)
    kind = [ModelKind.EWMA, ModelKind.LSTM_NORMAL, ModelKind.LSTM_NORMAL][seed % 3]
    d = 32 if kind != ModelKind.EWMA or seed % 2 else 16
    loss = LOSS_HINGE if rs.rand() < 0.5 else LOSS_BPR
    T = int(rs.choice([4, 9, 33, 49, 50, 64, 129, 140]))
    items = int(rs.choice([5, 17, 200, 3000]))
    users = int(rs.randint(8, 40))
    lens = rs.randint(3, T + 30, size=users)
    lens[rs.rand(users) < 0.5] = rs.randint(3, 14)          # mostly short sequences, a few long ones between them
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    it = (rs.zipf(1.3, size=int(ptr[-1])) % items).astype(np.uint32)
    hp = hparams(items, T, d, int(kind), loss, B=1, epochs=2, lr=float(rs.choice([0.05, 0.16])), l2=float(rs.choice([0.0, 4e-4])))
    g, o = Model(hp), OracleModel(hp)
    for call in range(2):
        lg, lo = g.fit(ptr, it), o.fit(ptr, it)
        assert lg == pytest.approx(lo, rel=1e-6), (call, lg, lo)
        assert_params_equal(g, o, kind, f"seed {seed} call {call}: {kind.name} d {d} T {T} items {items}")
        assert_lagged_equal(g, o, f"seed {seed} call {call}")
