"""The expectation of sbr_sequence_partition, from per-item scores only: for every user and kept position the scores of ALL items
for the state of the prefix (a function of the prefix, as in sequence_expect.py), then partition_expect.partition_row with the
prefix's distinct items excluded, the target's own score and whether the target is among them.  It restates no arithmetic: the
windows and positions are sequence_expect's, the shift and the mass partition_expect's."""
from __future__ import annotations

import numpy as np

from partition_expect import partition_row
from sequence_expect import kept_positions, window_of


def expect_sequence_partition(score_fn, seqs, T, temperature, mask_history=True, last=None):
    """score_fn(prefix: u32 array) -> [num_items] f32 scores.  -> one (shift bits u32, mass u64, score bits u32, masked u8) tuple
    of arrays per sequence, positions ascending."""
    out = []
    for seq in seqs:
        w = window_of(seq, T)
        shift, mass, score, masked = [], [], [], []
        for p in kept_positions(w.size, last):
            prefix = w[:p]
            s = np.asarray(score_fn(prefix), dtype=np.float32)
            sh, ms = partition_row(s, np.unique(prefix) if mask_history else (), temperature)
            shift.append(np.float32(sh))
            mass.append(ms)
            score.append(s[int(w[p])])
            masked.append(1 if mask_history and int(w[p]) in prefix.tolist() else 0)
        out.append((np.array(shift, dtype=np.float32).view(np.uint32), np.array(mass, dtype=np.uint64),
                    np.array(score, dtype=np.float32).view(np.uint32), np.array(masked, dtype=np.uint8)))
    return out


def flat(rows):
    """The per-sequence tuples as four flat arrays, in row order."""
    dt = (np.uint32, np.uint64, np.uint32, np.uint8)
    return tuple(np.concatenate([r[j] for r in rows]) if rows else np.zeros(0, dt[j]) for j in range(4))


def unresolved_rows(score_fn, seqs, T, pool, last=None):
    """How many kept positions have their `pool` best items (score desc, id asc) of the whole catalogue all inside their own
    prefix while the catalogue is larger than the pool — the rows the product must resolve by its second scan."""
    n = 0
    for seq in seqs:
        w = window_of(seq, T)
        for p in kept_positions(w.size, last):
            prefix = w[:p]
            s = np.asarray(score_fn(prefix), dtype=np.float32)
            if s.size <= pool:
                continue
            best = np.lexsort((np.arange(s.size), -s.astype(np.float64)))[:pool]
            n += bool(np.isin(best, prefix).all())
    return n
