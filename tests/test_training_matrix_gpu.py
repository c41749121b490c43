"""GPU: every cell of tests/training_matrix.py against the CPU oracle, bit for bit — every parameter and optimiser accumulator, the
lagged loss figure, and the mean loss (order-free in f64) to 1e-6 relative, as tests/test_parity_gpu.py compares them.  A cell is
one configuration of a fit (kind x loss x stored width x optimiser x devices and form of the step x the hooks that force a kernel
form, read per call) on a named shape of training_matrix.SHAPES: 203 Zipf items, max_sequence_length 12, ragged lengths from 2,
two full steps and a ragged third, so that a step starts from touched accumulators.

One device: the first step goes through step_local / debug_fetch, so a failing cell says which stage differs (HIDDEN, NEGATIVES,
TRIES, COEF, DHIDDEN, DINPUT, DENSE_GRAD), then step_apply; the later steps are whole sbr_fit_steps.  Several devices: the
exchange halves through tests/simulated_ranks.py (owner-applied update and gradient all-gather) and group_fit over
group_create(partition_item_table=True).  One subsequence per step: whole fits under set_step_fusion, and the reference-order
mode.  The key ordering's pair sort has no training call: its cells run the serving matrix's replay cell (sessions' audience over
remembered items) under the tile-size hook.

The oracle does not read the hooks: cells that differ only in them share one oracle run."""
import functools

import numpy as np
import pytest

import training_matrix as tm
from helpers import hparams, synthetic_interactions
from oracle.oracle import OracleModel
from sbr_rs_amd._abi import Debug, ModelKind
from sbr_rs_amd.engine import Model, group_create, group_fit
from test_parity_gpu import ALL_PARAMS, _export, assert_params_equal, assert_same_bits

pytestmark = pytest.mark.gpu

KIND = {tm.NORMAL: ModelKind.LSTM_NORMAL, tm.COUPLED: ModelKind.LSTM_COUPLED, tm.EWMA: ModelKind.EWMA}
STAGES = (Debug.IN_IDX, Debug.OUT_IDX, Debug.HIDDEN, Debug.NEGATIVES, Debug.TRIES, Debug.COEF, Debug.LOSS, Debug.DHIDDEN, Debug.DINPUT,
          Debug.DENSE_GRAD)


def _cut(ptr, it, keep):
    """the CSR of the first len(keep) users, user u's sequence cut to its first keep[u] items"""
    keep = np.asarray(keep, np.int64)
    keep = np.minimum(keep, np.diff(ptr).astype(np.int64)[:keep.size])
    new_ptr = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint64)
    return new_ptr, np.concatenate([it[int(ptr[u]):int(ptr[u]) + int(keep[u])] for u in range(keep.size)]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _data(shape, world):
    """two full steps of B sequences on every device and a ragged third of five; a sequence of two items has no row to train on and is
    left out by both sides, so the users are counted by their sequences of three and more"""
    sh = tm.SHAPES[shape]
    if sh.lens == "perstep":  # three sequences of 1 029 steps beside three short ones
        ptr, it = synthetic_interactions(6, tm.ITEMS, sh.T, seed=61, min_len=sh.T, zipf=True)
        ptr, it = _cut(ptr, it, [sh.T, 3, sh.T, 5, sh.T, 9])
    elif sh.lens == "one_long":
        ptr, it = synthetic_interactions(5, tm.ITEMS, sh.T, seed=62, min_len=70, zipf=True)
        ptr, it = _cut(ptr, it, [sh.T, 2, sh.T, 3, sh.T])
    else:
        want = 6 if sh.B == 1 else 2 * sh.B * world + 5
        ptr, it = synthetic_interactions(2 * want + 20, tm.ITEMS, sh.T, seed=63 + sh.B, min_len=sh.T if sh.lens == "long" else 2, zipf=True)
        keep = np.diff(ptr).astype(np.int64)
        if sh.B == 1:
            keep[1], keep[2] = 2, 3
        if sh.lens == "long":
            keep = np.where(np.arange(keep.size) % 7 == 3, 3, np.where(np.arange(keep.size) % 50 == 8, 2, keep))
        users = int(np.flatnonzero(np.cumsum(keep >= 3) == want)[0]) + 1
        ptr, it = _cut(ptr, it, keep[:users])
        assert (np.diff(ptr) >= 3).sum() == want
    assert np.diff(ptr).min() == 2 or sh.lens == "perstep", "length-2 sequences take part"
    ptr.setflags(write=False), it.setflags(write=False)
    return ptr, it


def _hp(c, rank=0):
    sh = tm.SHAPES[c.shape]
    return hparams(tm.ITEMS, sh.T, c.dim, int(KIND[c.kind]), c.loss, epochs=1, B=sh.B, ndev=c.world, rank=rank, opt=c.opt,
                   lr=0.02 if c.opt == tm.ADAM else 0.16)


def _params(m, kind):
    return {p: m.get_param(p) for p in ALL_PARAMS[kind]}


class _Held:
    """an oracle run's outcome, read like a model"""

    def __init__(self, params):
        self._p = params

    def get_param(self, p):
        return self._p[p]


def _same_outcome(models, kind, want, losses, lagged, what):
    for q, m in enumerate(models):
        assert_params_equal(m, _Held(want["params"]), kind, f"{what} replica {q}")
    for lg in losses:
        print(f"{what}: mean loss {lg!r} oracle {want['loss']!r}")
        assert lg == pytest.approx(want["loss"], rel=1e-6)
    assert_same_bits(np.array([lagged], np.float32), np.array([want["lagged"]], np.float32), f"{what}: lagged loss figure")


# ---- the oracle's side, once per configuration: the hooks choose between kernels that compute the same bits ------------------------
def _key(c):
    return (c.kind, c.loss, c.dim, c.opt, c.world, c.mode if c.mode in (tm.SINGLE, tm.REFERENCE) else "fit", c.shape)


@functools.lru_cache(maxsize=4)
def _oracle(key):
    kind, loss, dim, opt, world, how, shape = key
    c = tm.Cell("", kind, loss, dim, opt, world, how, (), shape, ())
    ptr, it = _data(shape, world)
    o = OracleModel(_hp(c))
    out = {}
    if how == tm.SINGLE:
        po = o.fit_begin(ptr, it)
        out["steps"] = nmb = po.epoch_prepare()
        out["rows"] = [po.minibatch_rows(mb) for mb in range(nmb)]
        po.step_local(0)
        out["sequences"] = int(po.last_offsets()[1])  # rows of the first time step: every sequence of the step
        out["stages"] = {w: po.debug_fetch(w, out["rows"][0]) for w in STAGES}
        po.step_apply(_export(po))
        out["after_first"] = _params(o, KIND[kind])
        for mb in range(1, nmb):
            po.step(mb)
        out["lagged"] = po.end_lagged()
        out["loss"] = po.end()[0]
        po.close()
    else:
        if how == tm.REFERENCE:
            o.set_reference_order(True)
        out["loss"] = o.fit(ptr, it)
        out["lagged"] = o.last_fit_lagged_loss()
    out["params"] = _params(o, KIND[kind])
    o.close()
    return out


def _census(c):
    """the keys of every device's first two steps, counted with numpy: (keys of the step, segments of <= 32 / 33..256 / > 256 entries)"""
    ptr, it = _data(c.shape, c.world)
    o = OracleModel(_hp(c))
    po = o.fit_begin(ptr, it)
    assert po.epoch_prepare() >= 3
    out = []
    for mb in (0, 1):
        for q in range(c.world):
            R = po.minibatch_rows(mb, q)
            po.compute_local(mb, q)
            keys = np.concatenate([po.debug_fetch(w, R, q) for w in (Debug.IN_IDX, Debug.OUT_IDX, Debug.NEGATIVES)])
            n = np.bincount(keys, minlength=tm.ITEMS)
            out.append((keys.size, int(((n > 0) & (n <= 32)).sum()), int(((n > 32) & (n <= 256)).sum()), int((n > 256).sum())))
        if mb == 0:
            po.step(0)
    po.close(), o.close()
    return out


def _shape_holds(c, rows):
    """the shape puts the cell's first two steps (on every device) where its claims say: the test does not trust the shape"""
    sh = tm.SHAPES[c.shape]
    if sh.many_keys is None:
        assert max(rows) >= sh.T - 1 > tm.MAX_T, "a step with a sequence past the sequence-resident kernels' limit"
        return
    for R in rows[:2 * c.world]:
        if sh.many_keys:
            assert 3 * R > tm.SEG_INLINE_MAX_KEYS and R >= tm.OVERLAP_MIN_ROWS, R
        else:
            assert 0 < 3 * R <= tm.SEG_INLINE_MAX_KEYS, R
        if tm.NG[c.kind]:
            assert (R > tm.DW_CHUNK_ROWS) == bool(sh.chunks), R
    if sh.many_keys and c.kind == tm.EWMA:
        for keys, short, middle, long in _census(c):
            print(f"{c.label}: {keys} keys, segments of <= 32 / 33..256 / > 256 entries: {short} / {middle} / {long}")
            assert keys > tm.SEG_INLINE_MAX_KEYS and short and middle and long, "all three segment classes occur"


# ---- the engine's side -------------------------------------------------------------------------------------------------------------
def run_single(c):
    want = _oracle(_key(c))
    ptr, it = _data(c.shape, 1)
    g = Model(_hp(c))
    pg = g.fit_begin(ptr, it)
    nmb = pg.epoch_prepare()
    rows = [pg.minibatch_rows(mb) for mb in range(nmb)]
    assert nmb == want["steps"] >= 2 and rows == want["rows"] and want["sequences"] == tm.SHAPES[c.shape].B
    _shape_holds(c, rows)
    pg.step_local(0)
    for w in STAGES:
        assert_same_bits(pg.debug_fetch(w, rows[0]), want["stages"][w], f"{c.label} first step {w.name}")
    pg.step_apply(0)
    assert_params_equal(g, _Held(want["after_first"]), KIND[c.kind], f"{c.label} after the first step")
    for mb in range(1, nmb):
        pg.step(mb)
    lagged = pg.end_lagged()
    _same_outcome([g], KIND[c.kind], want, [pg.end()[0]], lagged, c.label)


def run_fit(c):
    """one subsequence per step: a whole fit under the cell's step-fusion level"""
    want = _oracle(_key(c))
    ptr, it = _data(c.shape, 1)
    assert len(ptr) - 1 >= 2
    sh, rows = tm.SHAPES[c.shape], np.diff(ptr).astype(np.int64) - 1
    if c.shape == "one_long":
        assert ((rows > tm.SMALL_TAIL_TAIL256_ROWS) & (rows <= tm.SMALL_TAIL_MAX_ROWS)).sum() >= 2
    else:
        assert rows.max() <= min(tm.SMALL_TAIL_TAIL256_ROWS, tm.LSTM_STEPS_MAX_ROWS) and sh.B == 1
    g = Model(_hp(c))
    g.set_step_fusion(int(dict(c.env)["step_fusion"]))
    lg = g.fit(ptr, it)
    _same_outcome([g], KIND[c.kind], want, [lg], g.last_fit_lagged_loss(), c.label)


def run_reference(c):
    want = _oracle(_key(c))
    ptr, it = _data(c.shape, 1)
    g = Model(_hp(c))
    g.set_reference_order(True)
    lg = g.fit(ptr, it)
    _same_outcome([g], KIND[c.kind], want, [lg], g.last_fit_lagged_loss(), c.label)


def _exchange(c, exchange):
    from simulated_ranks import SimulatedRanks

    want = _oracle(_key(c))
    ptr, it = _data(c.shape, c.world)
    models = [Model(_hp(c, q)) for q in range(c.world)]
    plans = [m.fit_begin(ptr, it) for m in models]
    ranks = SimulatedRanks(models, plans)
    nmb = {p.epoch_prepare() for p in plans}
    assert len(nmb) == 1
    nmb = nmb.pop()
    assert nmb >= 2
    _shape_holds(c, [plans[q].minibatch_rows(mb) for mb in range(nmb) for q in range(c.world)])
    for mb in range(nmb):
        ranks.step(mb, exchange)
    ranks.finish()
    lagged = np.float32(0.0)
    for p in plans:  # the ranks' terms added in rank order, f32
        lagged = np.float32(lagged + np.float32(p.end_lagged()))
    _same_outcome(models, KIND[c.kind], want, [p.end()[0] for p in plans], lagged, c.label)


def run_owner(c):
    _exchange(c, "owner")


def run_gradient(c):
    _exchange(c, "gradient")


def run_partitioned(c):
    want = _oracle(_key(c))
    ptr, it = _data(c.shape, c.world)
    po = OracleModel(_hp(c)).fit_begin(ptr, it)
    nmb = po.epoch_prepare()
    assert nmb >= 2
    _shape_holds(c, [po.minibatch_rows(mb, q) for mb in range(nmb) for q in range(c.world)])
    po.close()
    models = group_create(_hp(c), c.world, partition_item_table=True)
    assert all(m.is_partitioned() for m in models)
    lg = group_fit(models, ptr, it)
    _same_outcome(models, KIND[c.kind], want, [lg], models[0].last_fit_lagged_loss(), c.label)


def run_sessions(c, monkeypatch):
    """the serving matrix's replay cell: sessions' audience orders (query, slot) pairs drawn from the remembered items with the pair sort"""
    import serving_matrix as sm
    import test_serving_matrix_gpu as serving

    monkeypatch.setenv("SBR_CATALOGUE_GROUPS", str(sm.GROUPS))
    case = serving.Case(KIND[c.kind], c.dim)
    try:
        serving.run_replay(case, False)
    finally:
        case.close()


RUN = {tm.SINGLE: run_single, tm.FUSED: run_fit, tm.REFERENCE: run_reference, tm.OWNER: run_owner, tm.GRADIENT: run_gradient,
       tm.PARTITIONED: run_partitioned}


def test_every_mode_of_the_table_has_a_runner():
    assert {c.mode for c in tm.CELLS} == set(RUN) | {tm.SESSIONS}


@pytest.mark.parametrize("cell", tm.CELLS, ids=tm.cell_id)
def test_cell(monkeypatch, cell):
    for name, value in cell.env:
        if name.startswith("SBR_"):  # every hook is read per call (step_fusion is the model's setting)
            monkeypatch.setenv(name, value)
    if cell.mode == tm.SESSIONS:
        run_sessions(cell, monkeypatch)
    else:
        RUN[cell.mode](cell)
