"""Shape, cases and oracle expectations of tests/test_stream_joins_gpu.py (no GPU needed to import or to run this module).

The shape is the smallest at which the WHOLE stream schedule of a training step engages (sbr_fit_step_local /
sbr_fit_step_apply): 160 sequences per step, all of length 12 -> 1 760 rows per step (the side streams engage above 1 365) and
5 280 sparse-update keys (the single-launch ordering and the hot-row pre-list end at 4 096); 300 items drawn Zipf(1), so that a
table row collects more than SBR_SEG_CHUNK = 256 entries in a step (check_shape asserts all of this from the oracle's indices);
three epochs of two steps, so that steps follow steps across an epoch switch and both epoch buffers are used again.

The MIXED data set adds a third, short step to every epoch (40 sequences -> 440 rows, 1 320 keys): everything on the main stream,
single-launch ordering.  What a step leaves for the next one (which events the main stream still has to join) then crosses a change
of form in both directions, the second one across an epoch switch (check_mixed_shape).
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass, field

import numpy as np

from helpers import LOSS_BPR, LOSS_HINGE, LOSS_WARP, OPT_ADAGRAD, OPT_ADAM, PAR_ASYNC, PAR_SYNC, hparams, synthetic_interactions
from recommend_expect import oracle_recommend
from sbr_rs_amd._abi import Debug, ModelKind, Param

ITEMS, T, B, STEPS_PER_EPOCH, EPOCHS = 300, 12, 160, 2, 3
ROWS_PER_STEP = B * (T - 1)
OVERLAP_ABOVE_ROWS = 1365      # step_schedule: small_rows
SINGLE_LAUNCH_SORT_KEYS = 4096
SEG_CHUNK = 256                # SBR_SEG_CHUNK
TOP_K = 10
EVAL_USERS = 6


@dataclass(frozen=True)
class Data:
    name: str
    users: int     # histories per device
    rows: tuple    # rows of the steps of every epoch

    @property
    def steps(self):
        return EPOCHS * len(self.rows)

    @property
    def overlapped_steps(self):   # the steps that queue anything on the side and sorter streams
        return EPOCHS * sum(r > OVERLAP_ABOVE_ROWS for r in self.rows)


UNIFORM = Data("uniform", B * STEPS_PER_EPOCH, (ROWS_PER_STEP,) * STEPS_PER_EPOCH)
MIXED = Data("mixed", 360, (ROWS_PER_STEP, ROWS_PER_STEP, 40 * (T - 1)))   # steps of 160, 160 and 40 sequences
MIXED_CASES = ["normal-warp-32", "coupled-hinge-16", "ewma-bpr-32"]


@dataclass(frozen=True)
class Case:
    name: str
    kind: ModelKind
    loss: int
    d: int
    opt: int = OPT_ADAGRAD
    lr: float = 0.16

    @property
    def ewma_fused(self):   # scan, scores and backward scan in one launch: no RECURRENT_FWD / _BWD launches
        return self.kind == ModelKind.EWMA and self.loss != LOSS_WARP

    def hp(self, world=1, rank=0, par=PAR_SYNC, epochs=EPOCHS, batch=B, items=ITEMS):
        return hparams(items, T, self.d, int(self.kind), self.loss, lr=self.lr, epochs=epochs, B=batch, ndev=world, rank=rank,
                       opt=self.opt, par=par)


# every branch of step_schedule (sbr_engine.hip)
CASES = [
    Case("normal-warp-32", ModelKind.LSTM_NORMAL, LOSS_WARP, 32),        # side_header, the ordering behind the score kernel
    Case("coupled-hinge-16", ModelKind.LSTM_COUPLED, LOSS_HINGE, 16),    # early ordering, from the start of the step
    Case("ewma-bpr-32", ModelKind.EWMA, LOSS_BPR, 32),                   # ewma_fused
    Case("ewma-warp-16", ModelKind.EWMA, LOSS_WARP, 16),
    Case("normal-warp-256", ModelKind.LSTM_NORMAL, LOSS_WARP, 256),      # per-time-step launches
    Case("normal-hinge-32-adam", ModelKind.LSTM_NORMAL, LOSS_HINGE, 32, opt=OPT_ADAM, lr=0.01),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def params_of(case):
    base = [Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_BIAS, Param.ITEM_BIAS_ACC]
    dense = ([Param.EWMA_ALPHA, Param.EWMA_ALPHA_ACC] if case.kind == ModelKind.EWMA
             else [Param.LSTM_W, Param.LSTM_W_ACC, Param.LSTM_B, Param.LSTM_B_ACC])
    moments = []
    if case.opt == OPT_ADAM:
        moments = [Param.ITEM_EMBEDDING_M, Param.ITEM_BIAS_M] + ([Param.EWMA_ALPHA_M] if case.kind == ModelKind.EWMA
                                                                 else [Param.LSTM_W_M, Param.LSTM_B_M])
    return base + dense + moments


def train_data(world=1, data=UNIFORM):
    return _train_data(world, data)   # (one cache entry however the defaults are spelled)


@functools.lru_cache(maxsize=None)
def _train_data(world, data):
    """world x 320 (MIXED: 360) histories of exactly T items, Zipf(1) over 300 items: one sequence of T - 1 rows each."""
    return synthetic_interactions(world * data.users, ITEMS, T, seed=41, min_len=T, zipf=True)


@functools.lru_cache(maxsize=None)
def eval_data():
    return synthetic_interactions(EVAL_USERS, ITEMS, T + 3, seed=43, min_len=2)


def _export(po):
    from oracle.oracle import lib

    out = np.zeros(po.exchange_bytes(), dtype=np.uint8)
    assert lib().orc_fit_export_local(po._h, 0, out.ctypes.data_as(C.c_void_p)) == 0
    return out


@dataclass
class Expect:
    params: dict
    loss: float
    lagged: float
    mrr: float
    ranks: np.ndarray
    predict: np.ndarray
    rec_items: np.ndarray
    rec_scores: np.ndarray
    hidden: list = field(default_factory=list)   # per step, in order (one device only)
    dense: list = field(default_factory=list)
    rows: list = field(default_factory=list)     # the oracle's row count of every step
    hottest_row_entries: int = 0                 # of the first step, from its indices


def _evaluation(o):
    tptr, tit = eval_data()
    mrr, ranks = o.mrr_score(tptr, tit)
    hist = tit[int(tptr[0]): int(tptr[1])]
    pred = o.predict(o.user_representation(hist), np.arange(ITEMS, dtype=np.uint32))
    ri, rs = oracle_recommend(o, ITEMS, tptr, tit, TOP_K)
    return mrr, ranks, pred, ri, rs


def oracle_single(name, data=UNIFORM) -> Expect:
    return _oracle_single(name, data)


@functools.lru_cache(maxsize=None)
def _oracle_single(name, data) -> Expect:
    """The oracle's run of the case, step by step (the hidden states and the dense gradient of every step are kept: the engine's
    debug fetch between the two halves of a step is compared with them).  Computed once per case, data set and process."""
    from oracle.oracle import OracleModel

    case = CASE_BY_NAME[name]
    ptr, it = train_data(1, data)
    o = OracleModel(case.hp())
    po = o.fit_begin(ptr, it)
    hidden, dense, rows, hottest = [], [], [], 0
    for e in range(EPOCHS):
        nmb = po.epoch_prepare()
        assert nmb == len(data.rows)
        for mb in range(nmb):
            R = po.minibatch_rows(mb)
            assert R == data.rows[mb]
            rows.append(R)
            po.step_local(mb)
            hidden.append(po.debug_fetch(Debug.HIDDEN, R))
            dense.append(po.debug_fetch(Debug.DENSE_GRAD, R))
            if e == 0 and mb == 0:
                keys = np.concatenate([po.debug_fetch(w, R) for w in (Debug.IN_IDX, Debug.OUT_IDX, Debug.NEGATIVES)])
                hottest = int(np.bincount(keys.astype(np.int64), minlength=ITEMS).max())
            po.step_apply(_export(po))
    lagged = po.end_lagged()
    loss = po.end()[0]
    po.close()
    ex = Expect({p: o.get_param(p) for p in params_of(case)}, loss, lagged, *_evaluation(o), hidden=hidden, dense=dense, rows=rows,
                hottest_row_entries=hottest)
    o.close()
    return ex


def oracle_world(name, world, par, data=UNIFORM) -> Expect:
    return _oracle_world(name, world, par, data)


@functools.lru_cache(maxsize=None)
def _oracle_world(name, world, par, data) -> Expect:
    """The oracle's whole fit with num_devices = world (every device takes B sequences of a step)."""
    from oracle.oracle import OracleModel

    case = CASE_BY_NAME[name]
    ptr, it = train_data(world, data)
    o = OracleModel(case.hp(world=world, par=par))
    loss = o.fit(ptr, it)
    ex = Expect({p: o.get_param(p) for p in params_of(case)}, loss, o.last_fit_lagged_loss(), *_evaluation(o))
    o.close()
    return ex


def check_shape(name):
    """The whole schedule engages at this shape: stated on the indices, not assumed."""
    ex = oracle_single(name)
    assert ROWS_PER_STEP > OVERLAP_ABOVE_ROWS, "the side streams do not engage"
    assert 3 * ROWS_PER_STEP > SINGLE_LAUNCH_SORT_KEYS, "the ordering is the single-launch form; no hot-row pre-list"
    assert ex.hottest_row_entries > SEG_CHUNK, f"no table row with more than {SEG_CHUNK} entries ({ex.hottest_row_entries})"
    assert len(ex.hidden) == EPOCHS * STEPS_PER_EPOCH


def check_mixed_shape(name):
    """Every epoch of the MIXED data is two steps of the whole overlapped schedule and one that stays on the main stream with the
    single-launch ordering, by the oracle's row counts: both changes of form occur, the second across an epoch switch."""
    rows = oracle_single(name, MIXED).rows
    assert rows == [1760, 1760, 440] * EPOCHS
    large, small = rows[0], rows[2]
    assert large > OVERLAP_ABOVE_ROWS and 3 * large > SINGLE_LAUNCH_SORT_KEYS, "the first two steps do not engage the side streams"
    assert small <= OVERLAP_ABOVE_ROWS and 3 * small <= SINGLE_LAUNCH_SORT_KEYS, "the third step is not the everything-on-main form"


# ---- one sequence per step (the one-launch runs of sbr_fit_steps, which timing switches off) ----
ONE_SEQ_CASE = Case("ewma-hinge-32-one-sequence", ModelKind.EWMA, LOSS_HINGE, 32)
ONE_SEQ_ITEMS, ONE_SEQ_USERS, ONE_SEQ_EPOCHS = 60, 24, 2


@functools.lru_cache(maxsize=None)
def one_sequence_data():
    return synthetic_interactions(ONE_SEQ_USERS, ONE_SEQ_ITEMS, T, seed=47, min_len=3, zipf=True)


@functools.lru_cache(maxsize=None)
def oracle_one_sequence():
    from oracle.oracle import OracleModel

    ptr, it = one_sequence_data()
    o = OracleModel(ONE_SEQ_CASE.hp(epochs=ONE_SEQ_EPOCHS, batch=1, items=ONE_SEQ_ITEMS))
    loss = o.fit(ptr, it)
    out = {p: o.get_param(p) for p in params_of(ONE_SEQ_CASE)}, loss, o.last_fit_lagged_loss()
    o.close()
    return out
