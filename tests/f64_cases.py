"""The case tables and the comparisons that tests/test_f64_truth.py (oracle, CPU) and tests/test_f64_truth_gpu.py (engine,
GPU) share: a training step, its intermediates and its optimiser update against tests/f64_model.py — on one device (run_case)
and as the group step of N devices (run_world_case, run_partition_check; second half of the file).

A `driver` hides the only differences between the two implementations' Python bindings (how a model is made, how the two
halves of a step are called, where the optimiser step count is read).  Nothing here imports the oracle or the engine.

Metric (per quantity): e(q) = max|q - q64| / max|q64|; for parameters, accumulators and moments q is the CHANGE of the step.
Yardstick: the same e for torch float32 on the same graph and inputs.  Bound: e <= M * max(e_f32, floor), M = 32 for every
class: the activation approximation is allowed 3e-7 .. 1e-6 absolute (tests/test_oracle.py::test_activation_accuracy) against
about 6e-8 for f32 libm, a factor of 5 to 16, and a different summation order is worth about 2.  floor = 2^-24 (the rounding of
a stored f32) for the step's intermediates and 2^-24 * max|after| / max|change| for a change.
"""
from __future__ import annotations

from collections import Counter
from typing import NamedTuple

import numpy as np
import torch

import f64_model as F
from helpers import LOSS_BPR, LOSS_HINGE, LOSS_WARP, OPT_ADAGRAD, OPT_ADAM, PAR_ASYNC, PAR_SYNC, hparams, synthetic_interactions
from sbr_rs_amd._abi import Debug, ModelKind, Param, storage_dim

M_BOUND = {"forward": 32.0, "rowgrad": 32.0, "dense": 32.0, "param": 32.0}
MIN_MARGIN = 1e-4          # the kink: every hinge / WARP row's float64 margin is at least this far from zero
EPS32 = 2.0 ** -24
NORMAL, COUPLED, EWMA = int(ModelKind.LSTM_NORMAL), int(ModelKind.LSTM_COUPLED), int(ModelKind.EWMA)

SLOTS = {
    "E": (Param.ITEM_EMBEDDING, Param.ITEM_EMBEDDING_ACC, Param.ITEM_EMBEDDING_M),
    "b": (Param.ITEM_BIAS, Param.ITEM_BIAS_ACC, Param.ITEM_BIAS_M),
    "W": (Param.LSTM_W, Param.LSTM_W_ACC, Param.LSTM_W_M),
    "bW": (Param.LSTM_B, Param.LSTM_B_ACC, Param.LSTM_B_M),
    "alpha": (Param.EWMA_ALPHA, Param.EWMA_ALPHA_ACC, Param.EWMA_ALPHA_M),
}


class Case(NamedTuple):
    name: str
    kind: int
    loss: int
    d: int
    items: int
    users: int
    T: int
    layout: str            # "epoch": B = every subsequence, ragged lengths; "equal": all of length L, B as given; "single": B = 1
    B: int = 0
    L: int = 0             # "equal": the users' length
    opt: int = OPT_ADAGRAD
    l2: float = 4e-4
    zipf: bool = True
    seed: int = 1          # data seed, searched on the CPU so that the kink condition holds on all three steps
    hot: bool = False      # assert on the indices: rows that are input, target and negative at once, many times
    inactive: bool = False  # assert: referenced rows whose data gradient is zero
    lr: float = 0.16


CASES = [
    # kinds x losses at d = 16, ragged lengths down to 3 (two rows), whole epoch in one minibatch
    Case("normal-hinge-16", NORMAL, LOSS_HINGE, 16, 60, 12, 9, "epoch", seed=3, inactive=True),
    Case("normal-bpr-16", NORMAL, LOSS_BPR, 16, 60, 12, 9, "epoch", l2=0.0, seed=3),
    Case("normal-warp-16", NORMAL, LOSS_WARP, 16, 60, 12, 9, "epoch", seed=3),
    Case("coupled-hinge-16", COUPLED, LOSS_HINGE, 16, 60, 12, 9, "epoch", l2=0.0, seed=3),
    Case("coupled-bpr-16", COUPLED, LOSS_BPR, 16, 60, 12, 9, "epoch", opt=OPT_ADAM, lr=0.01, seed=3),
    Case("coupled-warp-16", COUPLED, LOSS_WARP, 16, 60, 12, 9, "epoch", seed=3),
    Case("ewma-hinge-16", EWMA, LOSS_HINGE, 16, 60, 12, 9, "epoch", seed=3, inactive=True),
    Case("ewma-bpr-16", EWMA, LOSS_BPR, 16, 60, 12, 9, "epoch", seed=3),
    Case("ewma-warp-16", EWMA, LOSS_WARP, 16, 60, 12, 9, "epoch", opt=OPT_ADAM, lr=0.01, l2=0.0, seed=3),
    # every width, the stored ones and the padded ones
    Case("ewma-hinge-1", EWMA, LOSS_HINGE, 1, 40, 20, 8, "epoch", seed=1),
    Case("normal-bpr-1", NORMAL, LOSS_BPR, 1, 40, 20, 8, "epoch", seed=1),
    Case("coupled-warp-24", COUPLED, LOSS_WARP, 24, 50, 30, 10, "epoch", seed=1, hot=True),
    Case("normal-hinge-32-adam", NORMAL, LOSS_HINGE, 32, 30, 40, 12, "epoch", opt=OPT_ADAM, lr=0.01, seed=1, hot=True),
    Case("ewma-warp-64", EWMA, LOSS_WARP, 64, 150, 60, 14, "epoch", seed=3, hot=True),
    Case("normal-warp-64", NORMAL, LOSS_WARP, 64, 150, 60, 14, "epoch", seed=1, hot=True),
    Case("coupled-hinge-100", COUPLED, LOSS_HINGE, 100, 90, 30, 10, "epoch", seed=1, inactive=True),
    Case("normal-hinge-128", NORMAL, LOSS_HINGE, 128, 300, 60, 12, "epoch", seed=6, inactive=True),
    Case("ewma-bpr-200", EWMA, LOSS_BPR, 200, 120, 25, 10, "epoch", opt=OPT_ADAM, lr=0.01, seed=1),
    Case("normal-bpr-200", NORMAL, LOSS_BPR, 200, 80, 20, 7, "epoch", l2=0.0, seed=1),
    Case("coupled-warp-256", COUPLED, LOSS_WARP, 256, 120, 90, 9, "epoch", seed=1),
    Case("ewma-hinge-256", EWMA, LOSS_HINGE, 256, 100, 40, 10, "epoch", l2=0.0, seed=1),
    # B = 1 (the reference's own schedule), ragged; and equal lengths over several minibatches with B not a multiple of 32
    Case("normal-hinge-32-single", NORMAL, LOSS_HINGE, 32, 40, 14, 30, "single", seed=1),
    Case("ewma-bpr-16-single", EWMA, LOSS_BPR, 16, 30, 14, 40, "single", opt=OPT_ADAM, lr=0.01, seed=1),
    Case("ewma-hinge-32-single", EWMA, LOSS_HINGE, 32, 40, 14, 30, "single", seed=1),
    Case("coupled-bpr-64-equal", COUPLED, LOSS_BPR, 64, 70, 120, 11, "equal", B=37, L=11, seed=1, hot=True),
    # several thousand rows: many workgroup tiles, hot rows with long entry lists
    Case("normal-hinge-128-large", NORMAL, LOSS_HINGE, 128, 3000, 900, 20, "equal", B=300, L=20, seed=2, hot=True, inactive=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def case_data(case: Case):
    """(ptr, items, B): the interactions of a case and the batch_sequences its layout needs."""
    if case.layout == "equal":
        ptr, items = synthetic_interactions(case.users, case.items, case.L, seed=case.seed, min_len=case.L, zipf=case.zipf)
        assert case.L <= case.T
        return ptr, items, case.B
    ptr, items = synthetic_interactions(case.users, case.items, case.T + 5, seed=case.seed, min_len=3, zipf=case.zipf)
    if case.layout == "single":
        return ptr, items, 1
    return ptr, items, len(F.subsequences(ptr, items, case.T))


def _shapes(case: Case):
    d, ng = case.d, {NORMAL: 4, COUPLED: 3, EWMA: 0}[case.kind]
    s = {"E": (case.items, d), "b": (case.items,)}
    if case.kind == EWMA:
        s["alpha"] = (d,)
    else:
        s["W"], s["bW"] = (2 * d, ng * d), (ng * d,)
    return s


def seed_state(case: Case, model, rows_per_step):
    """Every parameter, accumulator and moment to seeded values off the initialisation.  Accumulators are of the order of
    the squared gradient of a few steps (row gradients are O(0.1 .. 1); a dense gradient sums over the packed rows), so that
    the update depends on the gradient's magnitude and not on its sign alone."""
    rs = np.random.RandomState(1000 + case.seed)
    adam = case.opt == OPT_ADAM
    for name, shape in _shapes(case).items():
        # W: 0.3 at d = 16 and 1 / sqrt(fan-in) beyond, so that the gates of a wide cell are not all saturated
        w = rs.randn(*shape) * {"E": 0.5, "b": 0.3, "W": 0.3 * min(1.0, (16.0 / case.d) ** 0.5), "bW": 0.2, "alpha": 0.7}[name]
        scale = 1.0 if name in ("E", "b") else max(1.0, rows_per_step / 8.0)
        acc = (0.02 + 0.2 * rs.rand(*shape)) * scale
        if adam:
            acc = acc * 0.05
        p, pa, pm = SLOTS[name]
        model.set_param(p, w.astype(np.float32))
        model.set_param(pa, acc.astype(np.float32))
        if adam:
            model.set_param(pm, (rs.randn(*shape) * 0.05 * np.sqrt(scale)).astype(np.float32))


def fetch_state(case: Case, model):
    """{name: [w, acc, mom or None]} as float32 arrays in their logical shapes."""
    out = {}
    for name, shape in _shapes(case).items():
        p, pa, pm = SLOTS[name]
        out[name] = [model.get_param(p).reshape(shape), model.get_param(pa).reshape(shape),
                     model.get_param(pm).reshape(shape) if case.opt == OPT_ADAM else None]
    return out


def unpack_dense(case: Case, dense):
    """The debug view of the dense gradient (stored width) as {name: logical array} and the padding elements."""
    d, ds = case.d, storage_dim(case.d)
    if case.kind == EWMA:
        return {"alpha": dense[:d]}, dense[d:]
    ng = 4 if case.kind == NORMAL else 3
    dW = dense[:2 * ds * ng * ds].reshape(2, ds, ng, ds)
    dbW = dense[2 * ds * ng * ds:].reshape(ng, ds)
    pad = np.concatenate([dW[:, d:].ravel(), dW[:, :d, :, d:].ravel(), dbW[:, d:].ravel()])
    return {"W": dW[:, :d, :, :d].reshape(2 * d, ng * d), "bW": dbW[:, :d].reshape(ng * d)}, pad


def err(q, q64):
    q64 = np.asarray(q64, dtype=np.float64)
    top = np.abs(q64).max() if q64.size else 0.0
    dev = np.abs(np.asarray(q, dtype=np.float64) - q64).max() if q64.size else 0.0
    if top == 0.0:
        return 0.0 if dev == 0.0 else np.inf
    return dev / top


class Report:
    """Every compared figure of a run: (step, quantity, class, e, e_f32, floor, bound), and the checks that failed."""

    def __init__(self, case):
        self.case, self.entries, self.failures = case, [], []

    def compare(self, step, quantity, cls, q, q64, q32, q64_plain=None, floor=EPS32):
        """q against q64 (the model under test, possibly mutated); the yardstick is q32 against the unmutated float64."""
        e, e32 = err(q, q64), err(q32, q64 if q64_plain is None else q64_plain)
        bound = M_BOUND[cls] * max(e32, floor)
        self.entries.append((step, quantity, cls, e, e32, floor, bound))
        if not e <= bound:
            self.failures.append(f"{self.case.name} step {step} {quantity}: e = {e:.3e} > {bound:.3e} (f32 {e32:.3e}, floor {floor:.3e})")

    def check(self, ok, what):
        if not ok:
            self.failures.append(f"{self.case.name}: {what}")

    def worst(self, cls, col=3):
        v = [en[col] for en in self.entries if en[2] == cls]
        return max(v) if v else 0.0

    def worst_ratio(self):
        """Largest e / bound over the tolerance checks."""
        return max((en[3] / en[6] for en in self.entries), default=0.0)

    def lines(self):
        return [f"{self.case.name:28s} step {s} {q:14s} {c:8s} e {e:.3e}  f32 {e32:.3e}  floor {fl:.3e}  bound {b:.3e}"
                for s, q, c, e, e32, fl, b in self.entries]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _changed_rows(before, after):
    ch = np.zeros(before[0].shape[0], dtype=bool)
    for x, y in zip(before, after):
        if x is not None:
            diff = _bits(x) != _bits(y)
            ch |= diff.reshape(diff.shape[0], -1).any(axis=1)
    return np.flatnonzero(ch)


def run_case(case: Case, driver, mutation=None, steps=3, whole_step=False, setup=None) -> Report:
    """Three optimiser steps of one plan.  Before each, the float64 side restarts from the implementation's current
    parameters and state: a one-step check repeated, not a free float64 trajectory.  whole_step: the step is taken by the
    plan's own `step` (the forms that fuse both halves); its intermediates are read afterwards and DHIDDEN, which those
    forms do not keep, is left out."""
    rep = Report(case)
    kind, loss, d, ds = case.kind, case.loss, case.d, storage_dim(case.d)
    ptr, items, B = case_data(case)
    hp = hparams(case.items, case.T, d, kind, loss, lr=case.lr, l2=case.l2, epochs=1, B=B, opt=case.opt)
    lr, l2 = float(hp.learning_rate), float(hp.l2_penalty)   # as stored: rounded to f32
    model = driver.make(hp)
    if setup is not None:
        setup(model)
    plan = model.fit_begin(ptr, items)
    nmb = plan.epoch_prepare()
    seed_state(case, model, plan.minibatch_rows(0))
    mb = 0
    for step in range(steps):
        if mb == nmb:
            nmb, mb = plan.epoch_prepare(), 0
        before = fetch_state(case, model)
        if case.l2 > 0:
            assert all(np.all(v[0] != 0) for v in before.values()), "start values must be non-zero under l2 > 0"
        t = driver.opt_steps(model) + 1
        R = plan.minibatch_rows(mb)
        if whole_step:
            driver.step(plan, mb)
            after = fetch_state(case, model)
        else:
            driver.step_local(plan, mb)
        dbg = {w: plan.debug_fetch(w, R) for w in (Debug.IN_IDX, Debug.OUT_IDX, Debug.NEGATIVES, Debug.HIDDEN, Debug.LOSS,
                                                   Debug.COEF, Debug.TRIES, Debug.DINPUT, Debug.DENSE_GRAD)}
        if not whole_step:
            dbg[Debug.DHIDDEN] = plan.debug_fetch(Debug.DHIDDEN, R)
            driver.step_apply(plan, mb)
            after = fetch_state(case, model)
        assert driver.opt_steps(model) == t
        in_idx, out_idx, neg = (dbg[w].astype(np.int64) for w in (Debug.IN_IDX, Debug.OUT_IDX, Debug.NEGATIVES))
        assert neg.min() >= 0 and neg.max() < case.items

        # ---- packed layout, from the input's lengths alone
        if case.layout == "epoch":
            off = F.layout_whole_epoch(ptr, items, case.T, R)
        elif case.layout == "equal":
            off = F.layout_equal_lengths(case.L - 1, R)
        else:
            off = np.arange(R + 1, dtype=np.int64)
        F.check_layout(off, in_idx, out_idx, ptr, items, case.T, whole_epoch=case.layout == "epoch")
        if case.hot:
            cnt = [np.bincount(v, minlength=case.items) for v in (in_idx, out_idx, neg)]
            both = (cnt[0] >= 2) & (cnt[1] >= 2) & (cnt[2] >= 1)
            assert both.any() and (cnt[0] + cnt[1] + cnt[2])[both].max() >= 8, "no hot row that is input, target and negative"

        # ---- the graph: float64 (the reference), float32 (the yardstick), and the mutant if one is planted
        p64 = {k: v[0].astype(np.float64) for k, v in before.items()}
        g64 = F.step_gradients(kind, loss, d, p64, in_idx, out_idx, neg, off)
        g32 = F.step_gradients(kind, loss, d, p64, in_idx, out_idx, neg, off, dtype=torch.float32)
        gm = g64 if mutation is None else F.step_gradients(kind, loss, d, p64, in_idx, out_idx, neg, off, mutation=mutation)
        if loss != LOSS_BPR:
            assert np.abs(g64["margin"]).min() >= MIN_MARGIN, f"{case.name} step {step}: a row sits on the kink ({np.abs(g64['margin']).min():.2e})"
            rep.check(np.array_equal(dbg[Debug.COEF] != 0, g64["margin"] > 0), f"step {step}: COEF is not non-zero exactly on the violating rows")
        if loss == LOSS_WARP:
            tries = dbg[Debug.TRIES]
            rep.check(tries.min() >= 1 and tries.max() <= 5, f"step {step}: TRIES outside 1..5")
            rep.check(bool(np.all(g64["margin"][tries < 5] > 0)), f"step {step}: a negative kept before the fifth try does not violate")
        if case.inactive:
            ref = np.unique(np.concatenate([in_idx, out_idx, neg]))
            assert (np.abs(g64["gE"][ref]).max(axis=1) == 0).any(), "no referenced row with a zero data gradient"
        cmp = lambda q, cls, name, key: rep.compare(step, name, cls, q, gm[key], g32[key], g64[key])
        cmp(dbg[Debug.HIDDEN][:, :d], "forward", "HIDDEN", "H")
        cmp(dbg[Debug.LOSS], "forward", "LOSS", "loss")
        cmp(dbg[Debug.COEF], "rowgrad", "COEF", "coef")
        if not whole_step:
            cmp(dbg[Debug.DHIDDEN][:, :d], "rowgrad", "DHIDDEN", "dH")
        cmp(dbg[Debug.DINPUT][:, :d], "rowgrad", "DINPUT", "dX")
        dense, pad = unpack_dense(case, dbg[Debug.DENSE_GRAD])
        for k, v in dense.items():
            cmp(v, "dense", "DENSE_GRAD." + k, k)
        pads = [dbg[w][:, d:] for w in (Debug.HIDDEN, Debug.DINPUT) + (() if whole_step else (Debug.DHIDDEN,))]
        rep.check(all(not _bits(p).any() for p in pads[:1]) and all(not np.any(p) for p in pads) and not np.any(pad),
                  f"step {step}: padding columns are not zero")

        # ---- the optimiser
        s64 = {k: [None if a is None else a.astype(np.float64) for a in v] for k, v in before.items()}
        sm = {k: [None if a is None else a.astype(np.float64) for a in v] for k, v in before.items()}
        s32 = {k: [None if a is None else a.copy() for a in v] for k, v in before.items()}
        F.optimiser_step(kind, case.opt, lr, l2, t, s64, g64, in_idx, out_idx, neg)
        rows_e, rows_b = F.optimiser_step(kind, case.opt, lr, l2, t, sm, gm, in_idx, out_idx, neg, mutation=mutation)
        F.optimiser_step(kind, case.opt, lr, l2, t, s32, {k: (None if v is None else v.astype(np.float32)) for k, v in g32.items()},
                         in_idx, out_idx, neg, dtype=np.float32)
        for name in before:
            for slot, what in enumerate(("", ".acc", ".m")):
                if before[name][slot] is None:
                    continue
                b0 = before[name][slot].astype(np.float64)
                c64, cm = s64[name][slot] - b0, sm[name][slot] - b0
                floor = EPS32 * np.abs(after[name][slot]).max() / max(np.abs(cm).max(), 1e-300)
                rep.compare(step, name + what, "param", after[name][slot].astype(np.float64) - b0, cm,
                            s32[name][slot].astype(np.float64) - b0, c64, floor=floor)
        # exact: which rows moved.  A referenced row moves whenever its gradient is non-zero: always under l2 > 0 (non-zero
        # start values) and under Adam (the moments decay); with Adagrad and l2 = 0 a zero gradient leaves it as it was.
        for name, rows in (("E", rows_e), ("b", rows_b)):
            changed = _changed_rows(before[name], after[name])
            if case.l2 > 0 or case.opt == OPT_ADAM:
                rep.check(np.array_equal(changed, rows), f"step {step}: changed {name} rows are not the referenced rows "
                          f"({len(changed)} changed, {len(rows)} referenced)")
            else:
                g = g64["gE" if name == "E" else "gb"]
                moving = rows[np.abs(g[rows]).reshape(len(rows), -1).max(axis=1) > 0]
                rep.check(np.array_equal(changed, moving), f"step {step}: changed {name} rows are not the referenced rows with a gradient")
        mb += 1

    # ---- user_representation and predict: history longer than T, shorter, empty
    state = fetch_state(case, model)
    p64 = {k: v[0].astype(np.float64) for k, v in state.items()}
    long_hist = np.concatenate([items[:case.T], items[:7]]).astype(np.uint32)
    for label, hist in (("long", long_hist), ("short", items[:min(3, case.T - 1)]), ("empty", items[:0])):
        r = model.user_representation(hist)
        r64 = F.user_representation(kind, d, p64, hist, case.T)
        r32 = F.user_representation(kind, d, p64, hist, case.T, dtype=torch.float32)
        rep.compare("rep", "rep." + label, "forward", r, r64, r32)
        allit = np.arange(case.items, dtype=np.uint32)
        rep.compare("rep", "predict." + label, "forward", model.predict(r, allit), F.predict(p64, r.astype(np.float64), allit),
                    F.predict(p64, r.astype(np.float64), allit, dtype=torch.float32))
    rep.one_launch_steps = plan.phase_clocks()[5] if hasattr(plan, "phase_clocks") else None
    plan.close()
    return rep


# ================================================================ world N ====================================================
# The group step of DESIGN.md §8 against tests/f64_model.py: N devices, one optimiser update.  M_BOUND, the floors and
# MIN_MARGIN are the ones above.
class WorldCase(NamedTuple):
    name: str
    world: int
    kind: int
    loss: int
    d: int
    items: int             # items % world != 0: the last owner slice is short
    users: int             # every user is one subsequence of L items; users % world != 0: a remainder is dropped
    T: int
    L: int
    B: int                 # sequences per device and step
    opt: int = OPT_ADAGRAD
    l2: float = 4e-4
    lr: float = 0.16
    seed: int = 1          # data seed, searched on the CPU so that the input conditions of run_world_case hold
    pipeline: bool = False  # Parallelism::Asynchronous on a replicated table: the staleness-one pipeline
    steps: int = 3


WORLD_CASES = [
    WorldCase("w2-normal-hinge-16", 2, NORMAL, LOSS_HINGE, 16, 41, 25, 9, 9, 4, seed=1),
    WorldCase("w3-ewma-warp-64", 3, EWMA, LOSS_WARP, 64, 100, 38, 10, 10, 4, seed=1),
    WorldCase("w4-coupled-bpr-24-adam", 4, COUPLED, LOSS_BPR, 24, 90, 39, 8, 8, 3, opt=OPT_ADAM, lr=0.01, seed=1),
    WorldCase("w8-normal-warp-128", 8, NORMAL, LOSS_WARP, 128, 150, 53, 8, 8, 2, seed=1),
    WorldCase("w8-ewma-hinge-256", 8, EWMA, LOSS_HINGE, 256, 203, 75, 9, 9, 3, l2=0.0, seed=1),
    WorldCase("w9-ewma-warp-32", 9, EWMA, LOSS_WARP, 32, 210, 58, 9, 9, 2, seed=1),
    # three minibatches per epoch, four steps: staleness one at step 2, the restart at step 3 (the next epoch's first)
    WorldCase("pipe-w2-normal-warp-64", 2, NORMAL, LOSS_WARP, 64, 61, 17, 9, 9, 3, seed=2, pipeline=True, steps=4),
    WorldCase("pipe-w3-ewma-hinge-32", 3, EWMA, LOSS_HINGE, 32, 70, 32, 10, 10, 4, seed=1, pipeline=True, steps=4),
]
WORLD_CASE_BY_NAME = {c.name: c for c in WORLD_CASES}


def world_case_data(case: WorldCase):
    return synthetic_interactions(case.users, case.items, case.L, seed=case.seed, min_len=case.L, zipf=True)


def world_hparams(case: WorldCase, rank=0):
    return hparams(case.items, case.T, case.d, case.kind, case.loss, lr=case.lr, l2=case.l2, epochs=2, B=case.B, opt=case.opt,
                   ndev=case.world, rank=rank, par=PAR_ASYNC if case.pipeline else PAR_SYNC)


_DEBUG_BLOCKS = (Debug.IN_IDX, Debug.OUT_IDX, Debug.NEGATIVES, Debug.HIDDEN, Debug.LOSS, Debug.COEF, Debug.TRIES, Debug.DINPUT,
                 Debug.DENSE_GRAD, Debug.DHIDDEN)


def _read_devices(case, drv, mb):
    """Every device's debug blocks of the local half that has just run."""
    out = []
    for q in range(case.world):
        R = drv.rows(mb, q)
        blocks = _DEBUG_BLOCKS if drv.keeps_dhidden else _DEBUG_BLOCKS[:-1]
        out.append({w: drv.debug_fetch(q, w, R) for w in blocks})
    return out


def _f64(state):
    return {k: v[0].astype(np.float64) for k, v in state.items()}


class _Conditions:
    """Item 3's conditions on the indices of a group step; each must hold on some step of the case."""

    def __init__(self, case):
        self.case, self.S = case, (case.items + case.world - 1) // case.world
        self.every = self.foreign = self.last_slice = self.straddle = False
        assert case.items % case.world != 0 and (case.world - 1) * self.S < case.items, "no short last owner slice"

    def see(self, dev_rows):
        case, S, n = self.case, self.S, self.case.world
        cnt = np.zeros(case.items, dtype=np.int64)
        sole = np.zeros(case.items, dtype=np.int64)
        for q, rows in enumerate(dev_rows):
            cnt[rows] += 1
            sole[rows] = q
        self.every |= bool((cnt == n).any())
        once = np.flatnonzero(cnt == 1)
        self.foreign |= bool((sole[once] != once // S).any())
        self.last_slice |= bool((np.flatnonzero(cnt) >= (n - 1) * S).any())
        self.straddle |= any(cnt[r * S - 1] > 0 and cnt[r * S] > 0 for r in range(1, n) if r * S < case.items)

    def assert_all(self):
        assert self.every, f"{self.case.name}: no row is referenced by every device in one step"
        assert self.foreign, f"{self.case.name}: no row is referenced by exactly one device that is not its owner"
        assert self.last_slice, f"{self.case.name}: no referenced row in the last, short owner slice"
        assert self.straddle, f"{self.case.name}: no owner change r with rows r*S - 1 and r*S both referenced"


def _compare_world_step(rep, case, step, dbgs, snap, snap_mut, before, after, t, mutation, cond, totals, keeps_dhidden):
    """One group step.  dbgs: the devices' debug blocks; snap: the state the gradient was taken at (snap_mut: where the planted
    pipeline mutant believes it was taken); before / after: the state around the update."""
    kind, loss, d, n = case.kind, case.loss, case.d, case.world
    lr, l2 = float(np.float32(case.lr)), float(np.float32(case.l2))      # as stored: rounded to f32
    p64, pm = _f64(snap), _f64(snap_mut)
    mutated_snap = snap_mut is not snap
    parts, dev_g, dev_idx = [], [], []
    for q, dbg in enumerate(dbgs):
        in_idx, out_idx, neg = (dbg[w].astype(np.int64) for w in (Debug.IN_IDX, Debug.OUT_IDX, Debug.NEGATIVES))
        assert neg.min() >= 0 and neg.max() < case.items
        off = F.layout_equal_lengths(case.L - 1, len(in_idx))
        parts.append((in_idx, out_idx, neg, off))
        dev_idx.append((in_idx, out_idx, neg))
        g64 = F.step_gradients(kind, loss, d, p64, in_idx, out_idx, neg, off)
        g32 = F.step_gradients(kind, loss, d, p64, in_idx, out_idx, neg, off, dtype=torch.float32)
        gm = F.step_gradients(kind, loss, d, pm, in_idx, out_idx, neg, off) if mutated_snap else g64
        dev_g.append(gm)
        if loss != LOSS_BPR:
            assert np.abs(g64["margin"]).min() >= MIN_MARGIN, f"{case.name} step {step} device {q}: a row sits on the kink ({np.abs(g64['margin']).min():.2e})"
            rep.check(np.array_equal(dbg[Debug.COEF] != 0, g64["margin"] > 0), f"step {step} device {q}: COEF is not non-zero exactly on the violating rows")
        if loss == LOSS_WARP:
            tries = dbg[Debug.TRIES]
            rep.check(tries.min() >= 1 and tries.max() <= 5, f"step {step} device {q}: TRIES outside 1..5")
            rep.check(bool(np.all(g64["margin"][tries < 5] > 0)), f"step {step} device {q}: a negative kept before the fifth try does not violate")
        cmp = lambda v, cls, name, key: rep.compare(step, f"dev{q}.{name}", cls, v, gm[key], g32[key], g64[key])
        cmp(dbg[Debug.HIDDEN][:, :d], "forward", "HIDDEN", "H")
        cmp(dbg[Debug.LOSS], "forward", "LOSS", "loss")
        cmp(dbg[Debug.COEF], "rowgrad", "COEF", "coef")
        if keeps_dhidden:
            cmp(dbg[Debug.DHIDDEN][:, :d], "rowgrad", "DHIDDEN", "dH")
        cmp(dbg[Debug.DINPUT][:, :d], "rowgrad", "DINPUT", "dX")
        dense, pad = unpack_dense(case, dbg[Debug.DENSE_GRAD])
        for k, v in dense.items():
            cmp(v, "dense", "DENSE_GRAD." + k, k)
        pads = [dbg[w][:, d:] for w in (Debug.HIDDEN, Debug.DINPUT) + ((Debug.DHIDDEN,) if keeps_dhidden else ())]
        rep.check(not _bits(pads[0]).any() and all(not np.any(p) for p in pads) and not np.any(pad),
                  f"step {step} device {q}: padding columns are not zero")
        totals[q][0] += g64["loss"].sum()
        totals[q][1] += g32["loss"].sum()
        totals[q][2] += len(in_idx)
    cond.see([np.unique(np.concatenate(ix)) for ix in dev_idx])

    # ---- the one update, from the union minibatch
    u_in, u_out, u_neg, u_off = F.concat_packed(parts)
    idx = (u_in, u_out, u_neg)
    g64 = F.step_gradients(kind, loss, d, p64, u_in, u_out, u_neg, u_off)
    g32 = F.step_gradients(kind, loss, d, p64, u_in, u_out, u_neg, u_off, dtype=torch.float32)
    gm = F.step_gradients(kind, loss, d, pm, u_in, u_out, u_neg, u_off) if mutated_snap else g64
    copy64 = lambda: {k: [None if a is None else a.astype(np.float64) for a in v] for k, v in before.items()}
    s64, sm = copy64(), copy64()
    s32 = {k: [None if a is None else a.copy() for a in v] for k, v in before.items()}
    rows_e, rows_b = F.optimiser_step(kind, case.opt, lr, l2, t, s64, g64, *idx)
    F.world_optimiser_step(kind, case.opt, lr, l2, t, sm, gm, idx, dev_g, dev_idx, mutation=mutation)
    F.optimiser_step(kind, case.opt, lr, l2, t, s32, {k: (None if v is None else v.astype(np.float32)) for k, v in g32.items()},
                     *idx, dtype=np.float32)
    for name in before:
        for slot, what in enumerate(("", ".acc", ".m")):
            if before[name][slot] is None:
                continue
            b0 = before[name][slot].astype(np.float64)
            c64, cm = s64[name][slot] - b0, sm[name][slot] - b0
            floor = EPS32 * np.abs(after[name][slot]).max() / max(np.abs(cm).max(), 1e-300)
            rep.compare(step, name + what, "param", after[name][slot].astype(np.float64) - b0, cm,
                        s32[name][slot].astype(np.float64) - b0, c64, floor=floor)
    for name, rows in (("E", rows_e), ("b", rows_b)):            # exact: which rows moved, by run_case's rule
        changed = _changed_rows(before[name], after[name])
        if case.l2 > 0 or case.opt == OPT_ADAM:
            rep.check(np.array_equal(changed, rows), f"step {step}: changed {name} rows are not the union's referenced rows "
                      f"({len(changed)} changed, {len(rows)} referenced)")
        else:
            g = g64["gE" if name == "E" else "gb"]
            moving = rows[np.abs(g[rows]).reshape(len(rows), -1).max(axis=1) > 0]
            rep.check(np.array_equal(changed, moving), f"step {step}: changed {name} rows are not the union's referenced rows with a gradient")


def _after_update(rep, case, drv, step, t):
    """The state after a group step, read from replica 0 once every replica is bit-identical to it and has counted t steps."""
    drv.gather_state()
    states = [fetch_state(case, m) for m in drv.replicas]
    for q, st in enumerate(states[1:], 1):
        same = all(np.array_equal(_bits(a), _bits(b)) for k in st for a, b in zip(st[k], states[0][k]) if a is not None)
        rep.check(same, f"step {step}: replica {q} is not bit-identical to replica 0")
    rep.check(all(drv.opt_steps(m) == t for m in drv.replicas), f"step {step}: the optimiser step count is not {t} on every replica")
    return states[0]


def run_world_case(case: WorldCase, driver, mutation=None) -> Report:
    """case.steps group steps of `driver(case, ptr, items)` (see tests/test_f64_truth.py::OracleWorld for what a driver is).
    Synchronous: every step restarts from seeded state on every replica.  Pipeline: seeded once; the float64 gradient of step
    k is taken at the state read when step_local(k) ran, the float64 update at the state read when update k was applied."""
    rep = Report(case)
    assert mutation is None or mutation in F.WORLD_MUTATIONS
    n = case.world
    ptr, items = world_case_data(case)
    nseq = len(F.subsequences(ptr, items, case.T))
    assert nseq == case.users and nseq % n != 0, "the partitions must drop a remainder"
    drv = driver(case, ptr, items)
    nmb, mb = drv.epoch_prepare(), 0
    assert nmb == (nseq // n + case.B - 1) // case.B
    cond = _Conditions(case)
    totals = [[0.0, 0.0, 0] for _ in range(n)]     # per device: float64 loss sum, float32 loss sum, examples
    reseed = lambda step: [seed_state(case._replace(seed=case.seed + 1000 * step), m, sum(drv.rows(mb, q) for q in range(n)))
                           for m in drv.replicas]
    nonzero = lambda st: case.l2 == 0 or all(np.all(v[0] != 0) for v in st.values())
    local = prev_snap = None                       # pipeline: (state at step_local, blocks) of the minibatch about to be applied
    for step in range(case.steps):
        if mb == nmb:
            nmb, mb, local = drv.epoch_prepare(), 0, None
        if not case.pipeline:
            reseed(step)
            before = fetch_state(case, drv.replicas[0])
            t = drv.opt_steps(drv.replicas[0]) + 1
            drv.step_local(mb)
            dbgs = _read_devices(case, drv, mb)
            drv.exchange(mb)
            snap = snap_mut = before
        else:
            if step == 0:
                reseed(0)
            if local is None:                      # an epoch's first minibatch: nothing is in flight
                start = fetch_state(case, drv.replicas[0])
                drv.step_local(mb)
                local = (start, _read_devices(case, drv, mb))
            snap, dbgs = local
            drv.scatter(mb)
            before = fetch_state(case, drv.replicas[0])
            local = None
            if mb + 1 < nmb and step + 1 < case.steps:   # minibatch mb + 1 is computed before update mb lands
                drv.step_local(mb + 1)
                local = (before, _read_devices(case, drv, mb + 1))
            t = drv.opt_steps(drv.replicas[0]) + 1
            drv.apply(mb)
            snap_mut = {None: snap, "pipeline_fresh_gradient": before,
                        "pipeline_stale_by_two": snap if prev_snap is None else prev_snap}.get(mutation, snap)
            prev_snap = snap
        assert nonzero(before), "start values must be non-zero under l2 > 0"
        after = _after_update(rep, case, drv, step, t)
        _compare_world_step(rep, case, step, dbgs, snap, snap_mut, before, after, t, mutation, cond, totals, drv.keeps_dhidden)
        mb += 1
    cond.assert_all()
    # ---- the loss of the fit: the devices' terms, each its loss sum over (1 + its examples)
    got = drv.end()
    rep.compare("end", "loss", "forward", np.array([got]), np.array([sum(t[0] / (1 + t[2]) for t in totals)]),
                np.array([sum(t[1] / (1 + t[2]) for t in totals)]))
    drv.close()
    return rep


def run_partition_check(case: WorldCase, driver, mutation=None) -> Report:
    """One whole epoch at world N, step by step, exact: from every device's IN_IDX / OUT_IDX of every minibatch its
    subsequences.  Every device holds floor(nseq / N), the devices' multisets are disjoint parts of the input's, and nseq mod N
    subsequences (not zero) are trained by nobody.  mutation = "remainder_kept" expects them trained."""
    rep = Report(case)
    n = case.world
    ptr, items = world_case_data(case)
    have = Counter(F.subsequences(ptr, items, case.T))
    nseq = sum(have.values())
    assert nseq % n != 0
    drv = driver(case, ptr, items)
    held = [Counter() for _ in range(n)]
    for mb in range(drv.epoch_prepare()):
        drv.step_local(mb)
        for q in range(n):
            R = drv.rows(mb, q)
            in_idx, out_idx = (drv.debug_fetch(q, w, R).astype(np.int64) for w in (Debug.IN_IDX, Debug.OUT_IDX))
            off = F.layout_equal_lengths(case.L - 1, R)
            held[q].update(F.check_layout(off, in_idx, out_idx, ptr, items, case.T, whole_epoch=False))
        if case.pipeline:
            drv.scatter(mb)
            drv.apply(mb)
        else:
            drv.exchange(mb)
    union = sum(held, Counter())
    want_each = nseq // n
    want_missing = 0 if mutation == "remainder_kept" else nseq % n
    rep.check(all(sum(h.values()) == want_each for h in held), f"a device does not hold floor(nseq / N) = {want_each} subsequences: "
              f"{[sum(h.values()) for h in held]}")
    # disjoint as multisets and inside the input: the union takes no subsequence more often than the input has it
    rep.check(all(have[s] >= c for s, c in union.items()), "the devices' subsequences overlap or are not the input's")
    missing = nseq - sum(union.values())
    rep.check(missing == want_missing, f"{missing} subsequences are trained by nobody, not {want_missing}")
    rep.compare("epoch", "trained", "forward", np.array([float(sum(union.values()))]), np.array([float(nseq - want_missing)]),
                np.array([float(nseq - nseq % n)]), np.array([float(nseq - nseq % n)]))
    drv.close()
    return rep
