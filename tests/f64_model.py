"""Float64 restatement of the training step of DESIGN.md §2 — the reference the oracle and the engine are both held to.

Written from the crate's graph (lstm.rs:258-337, ewma.rs:266-352, sequence_model.rs:70-232) and DESIGN.md §2 only.  The graph
is torch autograd (float64, or float32 to measure what plain f32 arithmetic loses), the optimiser is numpy.  Nothing here
imports the oracle or the engine; model and loss kinds are the plain integers of the C ABI.

The world-N group step of DESIGN.md §8 is the same step on the concatenation of the N devices' minibatches: `concat_packed`
and `world_optimiser_step` add nothing else.

`mutation=` plants one plausible misreading of the contract (MUTATIONS; WORLD_MUTATIONS for the world-N step);
tests/test_f64_truth.py uses it to show that the comparison can fail.  Nothing else passes it.
"""
from __future__ import annotations

from collections import Counter

import numpy as np
import torch

LSTM_NORMAL, LSTM_COUPLED, EWMA = 0, 1, 2
LOSS_BPR, LOSS_HINGE, LOSS_WARP = 0, 1, 2
OPT_ADAGRAD, OPT_ADAM = 0, 1

MUTATIONS = (
    "bias_touched_by_inputs",      # bias rows referenced by inputs too
    "l2_needs_data_gradient",      # L2 only on rows with a non-zero data gradient
    "mean_over_sequences",         # mean over the B sequences for sum
    "update_per_occurrence",       # one optimiser application per occurrence of a duplicate row
    "no_input_row_path",           # E gradient without the input-row path
    "hinge_without_one",           # relu(neg - pos)
    "ewma_first_step_scaled",      # h_0 = (1 - a) x_0
    "coupled_f_from_i",            # coupled LSTM: first gate block read as i, f = 1 - i
    "adam_decays_untouched_rows",  # moments of untouched rows decayed
    "adam_bias_step_off_by_one",   # 1 - beta^(t + 1)
)

# Misreadings of the world-N step: each is the identity at N = 1, so only tests/f64_cases.py::run_world_case can
# see them.  Kept apart from MUTATIONS: those are planted in the one-device step.
WORLD_MUTATIONS = (
    "mean_over_devices",                   # the devices' gradients averaged for summed
    "update_per_device",                   # N optimiser applications per step, one per device in device order
    "accumulator_of_per_device_squares",   # second moment from sum_q g_q^2 for (sum_q g_q)^2
    "l2_per_device",                       # the L2 term added once per device
    "adam_t_counts_devices",               # the step count advances by N
    "remainder_kept",                      # the nseq mod N subsequences beyond the partitions trained as well
    "pipeline_fresh_gradient",             # Asynchronous: gradient k taken after update k - 1 (staleness 0)
    "pipeline_stale_by_two",               # Asynchronous: gradient k taken where gradient k - 1 was taken (staleness 2)
)


# ---------------------------------------------------------------- packed layout ----------------------------------------------
def chunks_of(seq, T):
    """A user's chunks, short chunk first (data.rs:406-431)."""
    out, i, n = [], 0, len(seq)
    while i < n:
        r = (n - i) % T
        c = r if r else T
        out.append(tuple(int(v) for v in seq[i:i + c]))
        i += c
    return out


def subsequences(ptr, items, T):
    """The training subsequences: every chunk longer than two items (sequence_model.rs:76-83)."""
    out = []
    for u in range(len(ptr) - 1):
        out += [c for c in chunks_of(items[int(ptr[u]):int(ptr[u + 1])], T) if len(c) > 2]
    return out


def offsets_from_steps(steps):
    """off[t] = packed rows before time step t, for sequences of `steps` rows each (row(t, b) = off[t] + b)."""
    steps = np.sort(np.asarray(steps, dtype=np.int64))[::-1]
    off = [0]
    for t in range(int(steps[0])):
        off.append(off[-1] + int((steps > t).sum()))
    return np.asarray(off, dtype=np.int64)


def layout_whole_epoch(ptr, items, T, rows):
    """Set-up (a): the minibatch is the whole epoch, so its length multiset is the input's."""
    off = offsets_from_steps([len(s) - 1 for s in subsequences(ptr, items, T)])
    assert off[-1] == rows, (off[-1], rows)
    return off


def layout_equal_lengths(steps, rows):
    """Set-up (b): every subsequence has `steps` rows, any number of minibatches: row(t, b) = t * nb + b."""
    assert rows % steps == 0, (rows, steps)
    return np.arange(steps + 1, dtype=np.int64) * (rows // steps)


def columns(off):
    """Packed rows of every sequence of a minibatch, in packed (length-descending) order."""
    n = np.diff(off)
    return [np.asarray([off[t] + b for t in range(len(n)) if n[t] > b], dtype=np.int64) for b in range(int(n[0]))]


def check_layout(off, in_idx, out_idx, ptr, items, T, whole_epoch):
    """The recovered columns chain (input of step t + 1 = target of step t), are length-descending, and are subsequences
    of the input — all of them, each once, when the minibatch is the whole epoch.  Returns the sequences."""
    n = np.diff(off)
    assert np.all(n[:-1] >= n[1:]) and n[-1] > 0 and off[-1] == len(in_idx) == len(out_idx)
    seqs = []
    for rows in columns(off):
        assert np.array_equal(in_idx[rows[1:]], out_idx[rows[:-1]]), "column does not chain"
        seqs.append(tuple(int(v) for v in in_idx[rows]) + (int(out_idx[rows[-1]]),))
    have = Counter(subsequences(ptr, items, T))
    got = Counter(seqs)
    if whole_epoch:
        assert got == have, "the minibatch is not the epoch's subsequences"
    else:
        assert all(have[s] >= c for s, c in got.items()), "a column is not a subsequence of the input"
    return seqs


def concat_packed(parts):
    """The N devices' minibatches of one group step as ONE packed minibatch: parts[q] = (in_idx, out_idx, neg, off) as read
    back from device q.  The sequences of all devices, longest first (device order among equals), packed time-major again.
    Returns (in_idx, out_idx, neg, off) of the union."""
    cols = [(q, rows) for q, part in enumerate(parts) for rows in columns(part[3])]
    order = sorted(range(len(cols)), key=lambda c: -len(cols[c][1]))     # stable
    off = offsets_from_steps([len(cols[c][1]) for c in order])
    out = [np.zeros(int(off[-1]), dtype=np.int64) for _ in range(3)]
    for b, c in enumerate(order):
        q, rows = cols[c]
        dst = off[:len(rows)] + b
        for k in range(3):
            out[k][dst] = np.asarray(parts[q][k], dtype=np.int64)[rows]
    assert int(off[-1]) == sum(len(part[0]) for part in parts)
    return out[0], out[1], out[2], off


# ---------------------------------------------------------------- the graph ---------------------------------------------------
def _cell(kind, d, x, h, c, W, bW, mutation):
    z = torch.cat([x, h], dim=1) @ W + bW
    if kind == LSTM_NORMAL:
        i, f = torch.sigmoid(z[:, :d]), torch.sigmoid(z[:, d:2 * d])
        g, o = torch.tanh(z[:, 2 * d:3 * d]), torch.sigmoid(z[:, 3 * d:])
    else:
        g, o = torch.tanh(z[:, d:2 * d]), torch.sigmoid(z[:, 2 * d:])
        if mutation == "coupled_f_from_i":
            i = torch.sigmoid(z[:, :d])
            f = 1 - i
        else:
            f = torch.sigmoid(z[:, :d])
            i = 1 - f
    c = f * c + i * g
    return o * torch.tanh(c), c


def _recurrence(kind, d, X, off, dense, mutation):
    """Hidden state of every packed row, one batched evaluation per time step."""
    n = np.diff(off)
    dt = X.dtype
    h = torch.zeros(int(n[0]), d, dtype=dt)
    c = torch.zeros(int(n[0]), d, dtype=dt)
    out = []
    if kind == EWMA:
        a = torch.sigmoid(dense[0])
    for t in range(len(n)):
        x = X[int(off[t]):int(off[t + 1])]
        h, c = h[:int(n[t])], c[:int(n[t])]
        if kind == EWMA:
            if t == 0:
                h = (1 - a) * x if mutation == "ewma_first_step_scaled" else x
            else:
                h = a * h + (1 - a) * x
        else:
            h, c = _cell(kind, d, x, h, c, dense[0], dense[1], mutation)
        out.append(h)
    return torch.cat(out, dim=0)


def dense_names(kind):
    return ("alpha",) if kind == EWMA else ("W", "bW")


def step_gradients(kind, loss, d, params, in_idx, out_idx, neg, off, dtype=torch.float64, mutation=None):
    """One minibatch against one parameter snapshot: forward, summed loss, backward with seed gradient 1.

    params: E [I, d], b [I], and W [2d, G d] + bW [G d] (column blocks i f g o; coupled f g o) or alpha [d].
    Returns float64 numpy arrays: H, loss, margin (hinge / WARP: (1 + neg) - pos), coef (d loss / d (neg - pos)), dH (score
    path only), dX (recurrence path only), gE, gb, and the dense gradients by name."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    ii, oi, ni = (torch.as_tensor(np.asarray(v, dtype=np.int64)) for v in (in_idx, out_idx, neg))
    E = t(params["E"]).requires_grad_(True)
    b = t(params["b"]).requires_grad_(True)
    dense = [t(params[k]).requires_grad_(True) for k in dense_names(kind)]
    X = (E.detach()[ii].requires_grad_(True) if mutation == "no_input_row_path" else E[ii])
    X.retain_grad()
    H = _recurrence(kind, d, X, off, dense, mutation)
    Hs = H.clone()          # the scores' own view of h: its gradient is the score path alone
    Hs.retain_grad()
    pos = (Hs * E[oi]).sum(dim=1) + b[oi]
    ng = (Hs * E[ni]).sum(dim=1) + b[ni]
    diff = ng - pos
    diff.retain_grad()
    if loss == LOSS_BPR:
        margin = None
        rows = torch.sigmoid(diff)
    else:
        margin = (1 + ng) - pos
        rows = torch.relu(diff if mutation == "hinge_without_one" else 1 + diff)
    total = rows.sum()
    if mutation == "mean_over_sequences":
        total = total / int(off[1] - off[0])
    total.backward()
    f = lambda v: v.detach().numpy().astype(np.float64)
    out = {"H": f(H), "loss": f(rows), "coef": f(diff.grad), "dH": f(Hs.grad),
           "dX": f(X.grad) if X.grad is not None else np.zeros((len(in_idx), d)),
           "gE": f(E.grad), "gb": f(b.grad), "pos": f(pos), "neg": f(ng),
           "margin": None if margin is None else f(margin)}
    for k, v in zip(dense_names(kind), dense):
        out[k] = f(v.grad)
    return out


def user_representation(kind, d, params, history, T, dtype=torch.float64):
    """sequence_model.rs:182-211: the last T items (an empty history is item 0), the state after the last of them."""
    items = [int(v) for v in history][-T:] or [0]
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    dense = [t(params[k]) for k in dense_names(kind)]
    X = t(params["E"])[torch.as_tensor(items)]
    H = _recurrence(kind, d, X, np.arange(len(items) + 1), dense, None)
    return H[-1].numpy().astype(np.float64)


def predict(params, rep, item_ids, dtype=torch.float64):
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    ids = torch.as_tensor(np.asarray(item_ids, dtype=np.int64))
    return (t(params["E"])[ids] @ t(rep) + t(params["b"])[ids]).numpy().astype(np.float64)


# ---------------------------------------------------------------- the optimiser -----------------------------------------------
def _apply(opt, w, acc, mom, g, lr, l2, t, ft, l2_mask=None, mutation=None, cross=None):
    """Element update of DESIGN §2 on arrays of one shape, in place.  acc: Adagrad's sum of squares / Adam's second moment.
    cross (a world mutant's only): subtracted from the square of the gradient."""
    g = g + (l2 * w if l2_mask is None else l2 * w * l2_mask)
    gg = g * g if cross is None else g * g - cross
    if opt == OPT_ADAGRAD:
        acc += gg
        w -= lr / (ft(1e-10) + np.sqrt(acc)) * g
    else:
        b1, b2 = ft(0.9), ft(0.999)
        if mutation == "adam_bias_step_off_by_one":
            t = t + 1
        mom[...] = b1 * mom + (1 - b1) * g
        acc[...] = b2 * acc + (1 - b2) * gg
        c1, c2 = ft(1.0 - 0.9 ** t), ft(1.0 - 0.999 ** t)
        w -= lr / (np.sqrt(acc / c2) + ft(1e-8)) * (mom / c1)


def optimiser_step(kind, opt, lr, l2, t, state, grads, in_idx, out_idx, neg, dtype=np.float64, mutation=None, cross=None):
    """state: {name: (w, acc, mom or None)} for E, b and the dense parameters, updated in place (arrays of `dtype`).
    t: the optimiser step being taken, counted from 1.  Returns (touched embedding rows, touched bias rows).
    cross: {gradient name: array} taken off the squared gradients (world_optimiser_step's accumulator mutant only)."""
    ft = dtype
    lr, l2 = ft(lr), ft(l2)
    for k in dense_names(kind):
        w, acc, mom = state[k]
        _apply(opt, w, acc, mom, grads[k].astype(dtype), lr, l2, t, ft, mutation=mutation, cross=None if cross is None else cross[k])
    rows_e = np.unique(np.concatenate([in_idx, out_idx, neg]).astype(np.int64))
    rows_b = np.unique(np.concatenate([out_idx, neg] + ([in_idx] if mutation == "bias_touched_by_inputs" else [])).astype(np.int64))
    if mutation == "update_per_occurrence":
        _per_occurrence(opt, lr, l2, t, state, grads, in_idx, out_idx, neg, ft)
        return rows_e, rows_b
    for name, rows, g in (("E", rows_e, grads["gE"]), ("b", rows_b, grads["gb"])):
        w, acc, mom = state[name]
        gr = g[rows].astype(dtype)
        mask = None
        if mutation == "l2_needs_data_gradient":
            nz = gr != 0
            mask = (nz.any(axis=1, keepdims=True) if gr.ndim == 2 else nz).astype(dtype)
        wr, ar = w[rows], acc[rows]
        mr = mom[rows] if mom is not None else None
        _apply(opt, wr, ar, mr, gr, lr, l2, t, ft, l2_mask=mask, mutation=mutation,
               cross=None if cross is None else cross["gE" if name == "E" else "gb"][rows])
        w[rows], acc[rows] = wr, ar
        if mom is not None:
            mom[rows] = mr
            if mutation == "adam_decays_untouched_rows":
                rest = np.setdiff1d(np.arange(w.shape[0]), rows)
                mom[rest] *= ft(0.9)
                acc[rest] *= ft(0.999)
    return rows_e, rows_b


def world_optimiser_step(kind, opt, lr, l2, t, state, grads, idx, dev_grads, dev_idx, dtype=np.float64, mutation=None):
    """The ONE optimiser update of a world-N group step: `optimiser_step` on the union minibatch — grads and
    idx = (in_idx, out_idx, neg) of concat_packed's union; the devices' gradients are summed there because the union's loss
    is one sum.  L2 once, one accumulator update from the summed gradient, t advances by 1.  dev_grads / dev_idx (the same
    per device) serve the mutants alone.  Returns (touched embedding rows, touched bias rows) of the union."""
    n = len(dev_idx)
    names = ("gE", "gb") + dense_names(kind)
    rows = optimiser_step(kind, opt, lr, l2, t, {k: [None if a is None else a.copy() for a in v] for k, v in state.items()},
                          grads, *idx, dtype=dtype)           # the union's touched rows, whatever the mutant does
    if mutation == "update_per_device":
        for q in range(n):
            optimiser_step(kind, opt, lr, l2, t, state, dev_grads[q], *dev_idx[q], dtype=dtype)
        return rows
    cross = None
    if mutation == "mean_over_devices":
        grads = dict(grads, **{k: grads[k] / n for k in names})
    elif mutation == "l2_per_device":
        l2 = l2 * n
    elif mutation == "adam_t_counts_devices":
        t = t * n
    elif mutation == "accumulator_of_per_device_squares":
        cross = {k: sum(g[k] for g in dev_grads) ** 2 - sum(g[k] ** 2 for g in dev_grads) for k in names}
    optimiser_step(kind, opt, lr, l2, t, state, grads, *idx, dtype=dtype, cross=cross)
    return rows


def _per_occurrence(opt, lr, l2, t, state, grads, in_idx, out_idx, neg, ft):
    """The mutant that walks the sparse gradient entry by entry (packed row order; input, target, negative)."""
    coef, H, dX = grads["coef"], grads["H"], grads["dX"]
    for r in range(len(in_idx)):
        for row, ge, gb in ((int(in_idx[r]), dX[r], None), (int(out_idx[r]), -coef[r] * H[r], -coef[r]),
                            (int(neg[r]), coef[r] * H[r], coef[r])):
            for name, g in (("E", ge), ("b", gb)):
                if g is None:
                    continue
                w, acc, mom = state[name]
                wr, ar = w[row:row + 1], acc[row:row + 1]
                mr = mom[row:row + 1] if mom is not None else None
                _apply(opt, wr, ar, mr, np.asarray(g, dtype=ft)[None], lr, l2, t, ft)
