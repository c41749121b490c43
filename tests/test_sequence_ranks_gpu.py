"""GPU: sbr_sequence_ranks (the exact next-item rank at every position of a sequence from one forward pass: rank_test_score_kernel
and rank_gemm_kernel over one scan row per position, then rank_prefix_kernel's mask correction over the sequence's own packed
input rows).  Ranks are integers and compared with np.array_equal: against the oracle expectation (sequence_expect.py: the
oracle's user_representation + predict for every prefix), against the product's own rank_targets on the explicit prefixes and
mrr_score, across `last`, across the host's chunks and on poisoned scratch.  Models as in test_catalogue_gpu.py: engine model
and oracle with the same set parameters, heavy-tie parameters so that `>=` against `>` shows."""
import functools

import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams
from oracle.oracle import OracleModel
from rank_expect import assert_ranks_equal
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Model
from sbr_rs_amd.errors import EngineError, PredictionError
from sbr_rs_amd.evaluation import rank_targets
from sequence_expect import csr, expect_sequence_ranks, kept_positions, oracle_score_fn, rows_of, window_of

pytestmark = pytest.mark.gpu

HOOK = "SBR_CATALOGUE_GROUPS"


def _heavy_tie_params(items, d, seed):
    """test_catalogue_gpu.py's: E rows drawn from 50 distinct rows and biases from 4 values, so scores tie in large classes."""
    rs = np.random.RandomState(seed)
    rows = (rs.randn(50, d) * 0.3).astype(np.float32)
    p = 1.0 / np.arange(1, 51)
    E = rows[rs.choice(50, size=items, p=p / p.sum())]
    bias = np.array([-0.5, 0.0, 0.25, 0.5], np.float32)[rs.randint(0, 4, items)]
    return np.ascontiguousarray(E), bias


def _engine(hp, E, bias):
    g = Model(hp)
    g.set_param(Param.ITEM_EMBEDDING, E)
    g.set_param(Param.ITEM_BIAS, bias)
    return g


def _sequences(users, items, T, seed, lengths=None):
    """Sequences of the lengths 0, 1, 2, T, T + 1, T + 5 (and 3, T - 1) in turn, or `lengths` = (lo, hi) uniform; each draws
    from its own pool of about half as many items as it is long, so that sequences repeat items — inside a prefix and as
    targets of their own prefixes."""
    rs = np.random.RandomState(seed)
    cycle = [0, 1, 2, T, T + 1, T + 5, 3, T - 1]
    seqs = []
    for u in range(users):
        n = cycle[u % len(cycle)] if lengths is None else rs.randint(lengths[0], lengths[1] + 1)
        pool = rs.choice(items, size=max(2, min(items, max(3, n // 2 + 1 + u % 3))), replace=False)
        seqs.append(pool[rs.randint(0, pool.size, n)].astype(np.uint32))
    return seqs


def _units(seqs, T, last=None):
    return sum(len(kept_positions(window_of(s, T).size, last)) for s in seqs)


def _call(g, seqs, **kw):
    ptr, it = csr(seqs)
    p, r = g.sequence_ranks(ptr, it, **kw)
    assert p.dtype == np.uint64 and r.dtype == np.uint32 and p[0] == 0 and p[-1] == r.size
    return rows_of(p, r)


# ------------------------------------------------------------------------------------------------
# 1. against the oracle expectation
# ------------------------------------------------------------------------------------------------
#        kind                    d    items  T   users
SHAPES = [(ModelKind.EWMA, 16, 1100, 24, 130),
          (ModelKind.LSTM_NORMAL, 32, 300, 24, 48),
          (ModelKind.LSTM_COUPLED, 256, 70, 6, 30),
          (ModelKind.EWMA, 100, 517, 6, 130),
          (ModelKind.LSTM_NORMAL, 128, 200, 6, 40),
          (ModelKind.LSTM_COUPLED, 64, 70, 6, 30)]


@functools.lru_cache(maxsize=None)
def _oracle_case(kind, d, items, T, users):
    """Parameters, sequences and the expectation with and without the mask, computed once for the case's forced group counts."""
    E, bias = _heavy_tie_params(items, d, 300 + d)
    hp = hparams(items, T, d, int(kind), LOSS_HINGE, B=8)
    o = OracleModel(hp)
    o.set_param(Param.ITEM_EMBEDDING, E)
    o.set_param(Param.ITEM_BIAS, bias)
    seqs = _sequences(users, items, T, seed=d + T)
    fn = oracle_score_fn(o, items)
    want = {mask: expect_sequence_ranks(fn, seqs, T, mask_history=mask) for mask in (True, False)}
    return hp, E, bias, seqs, want


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0].name}-d{s[1]}")
def test_sequence_ranks_match_oracle(monkeypatch, groups, shape):
    """Every position of every window against the oracle's scores of its explicit prefix, masked and unmasked, with the scan in
    one item range and in three.  The lengths cover the empty row (n = 0, 1), one position, a full window (T + 1) and a cut one
    (T + 5); the repeats make targets that occur in their prefix (rank num_items) and prefix items masked once."""
    monkeypatch.setenv(HOOK, str(groups))
    hp, E, bias, seqs, want = _oracle_case(*shape)
    kind, d, items, T, users = shape
    g = _engine(hp, E, bias)
    lens = {len(s) for s in seqs}
    assert {0, 1, 2, T, T + 1, T + 5} <= lens
    assert any(int(s[-1]) in s[:-1].tolist() for s in seqs if len(s) >= 2) and any((r == items).any() for r in want[True])
    for mask in (True, False):
        got = _call(g, seqs, include_history=not mask)
        assert [r.size for r in got] == [0 if len(s) < 2 else min(len(s), T + 1) - 1 for s in seqs]
        assert_ranks_equal(got, want[mask], f"mask={mask}")
    assert any(not np.array_equal(a, b) for a, b in zip(want[True], want[False]))


# ------------------------------------------------------------------------------------------------
# 2. against the product's own rank_targets and mrr_score
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(ModelKind.EWMA, 16), (ModelKind.LSTM_NORMAL, 32)])
def test_sequence_ranks_equal_rank_targets_on_prefixes(kind, d):
    items, T, users = 300, 12, 60
    E, bias = _heavy_tie_params(items, d, 11)
    g = _engine(hparams(items, T, d, int(kind), LOSS_HINGE, B=8), E, bias)
    seqs = _sequences(users, items, T, seed=5)
    for mask in (True, False):
        got = _call(g, seqs, include_history=not mask)
        hists, targets, owner = [], [], []
        for u, s in enumerate(seqs):
            w = window_of(s, T)
            for p in range(1, w.size):
                hists.append(w[:p])
                targets.append(w[p: p + 1])
                owner.append(u)
        flat = np.concatenate(rank_targets(g, hists, targets, mask_history=mask))
        assert np.array_equal(np.concatenate(got), flat) and flat.size == _units(seqs, T)
    # the last entry of a row is mrr_score's rank where the whole sequence fits the window
    ptr, it = csr(seqs)
    _mrr, mr = g.mrr_score(ptr, it)
    ranked = [u for u, s in enumerate(seqs) if len(s) >= 2]
    assert len(ranked) == mr.size
    got = _call(g, seqs)
    fits = [(j, u) for j, u in enumerate(ranked) if len(seqs[u]) <= T + 1]
    assert len(fits) > 10 and len(fits) < len(ranked)
    assert all(got[u][-1] == mr[j] for j, u in fits)


# ------------------------------------------------------------------------------------------------
# 3. last
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(ModelKind.EWMA, 16), (ModelKind.LSTM_COUPLED, 32)])
def test_sequence_ranks_last_is_the_tail_of_the_full_call(kind, d):
    items, T, users = 300, 12, 60
    E, bias = _heavy_tie_params(items, d, 12)
    g = _engine(hparams(items, T, d, int(kind), LOSS_HINGE, B=8), E, bias)
    seqs = _sequences(users, items, T, seed=6)
    full = _call(g, seqs)
    assert max(r.size for r in full) == T
    for last in (1, 3, T + 40):
        got = _call(g, seqs, last=last)
        assert_ranks_equal(got, [r[max(0, r.size - last):] for r in full], f"last={last}")
    assert_ranks_equal(_call(g, seqs, last=None), full, "last=None")
    # sizing alone: out_ranks NULL fills out_ptr
    ptr, it = csr(seqs)
    out_ptr = np.full(users + 1, 77, np.uint64)
    assert g._L.sbr_sequence_ranks(g._h, ptr.ctypes.data, it.ctypes.data, users, 0, 3, out_ptr.ctypes.data, None) == Status.OK
    assert np.array_equal(np.diff(out_ptr.astype(np.int64)), [min(3, r.size) for r in full]) and out_ptr[0] == 0


# ------------------------------------------------------------------------------------------------
# 4. chunking
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [ModelKind.EWMA, ModelKind.LSTM_NORMAL])
def test_sequence_ranks_chunks(kind):
    """More than 8 192 scan units: two launches, with a user cut by the first chunk's end and forwarded again in the second.
    The ranks equal the per-user calls' (a user alone is never cut), and a few rows on either side of the cut the oracle's."""
    items, T, d, users = 300, 24, 16, 400
    E, bias = _heavy_tie_params(items, d, 13)
    hp = hparams(items, T, d, int(kind), LOSS_HINGE, B=8)
    g = _engine(hp, E, bias)
    seqs = _sequences(users, items, T, seed=7, lengths=(20, 25))
    per_user = np.array([min(len(s), T + 1) - 1 for s in seqs])
    ends = np.cumsum(per_user)
    assert ends[-1] > 8192
    cut = int(np.searchsorted(ends, 8192, side="right"))  # the user who holds unit 8 192
    assert ends[cut] > 8192 > ends[cut - 1], "the chunk's end cuts a user"
    got = _call(g, seqs)
    assert [r.size for r in got] == per_user.tolist()
    second = np.concatenate(got)[8192:]
    assert second.size == ends[-1] - 8192 and np.unique(second).size > 1
    pieces = [_call(g, seqs[a: a + 100]) for a in range(0, users, 100)]  # 100 users: about 2 300 units, one launch each
    assert_ranks_equal(got, [r for piece in pieces for r in piece], "whole call vs calls of 100 users")
    o = OracleModel(hp)
    o.set_param(Param.ITEM_EMBEDDING, E)
    o.set_param(Param.ITEM_BIAS, bias)
    near = [cut - 1, cut, cut + 1, users - 1]
    want = expect_sequence_ranks(oracle_score_fn(o, items), [seqs[u] for u in near], T)
    assert_ranks_equal([got[u] for u in near], want, "around the cut")


# ------------------------------------------------------------------------------------------------
# 5. poisoned scratch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["0xFF", "0x7F", "0x80"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=["LSTM", "EWMA"])
def test_sequence_ranks_on_poisoned_scratch(monkeypatch, poison, shape):
    """No kernel of the call may assume zeroed scratch: the same ranks with the arena filled with a byte pattern at every carve."""
    hp, E, bias, seqs, want = _oracle_case(*shape)
    monkeypatch.setenv("SBR_TEST_POISON", poison)
    g = _engine(hp, E, bias)
    assert_ranks_equal(_call(g, seqs), want[True], f"poison {poison}")
    assert_ranks_equal(_call(g, seqs, include_history=True, last=2), [r[max(0, r.size - 2):] for r in want[False]], f"poison {poison}")


# ------------------------------------------------------------------------------------------------
# 6. errors
# ------------------------------------------------------------------------------------------------
def test_sequence_ranks_errors():
    items, d, T, users = 300, 16, 8, 20
    E, bias = _heavy_tie_params(items, d, 7)
    seqs = _sequences(users, items, T, seed=9)
    ptr, it = csr(seqs)
    E2 = E.copy()
    E2[123, 3] = np.nan
    bad_model = _engine(hparams(items, T, d, int(ModelKind.EWMA), LOSS_HINGE, B=8), E2, bias)
    with pytest.raises(PredictionError.InvalidPredictionValue):
        bad_model.sequence_ranks(ptr, it)
    g = _engine(hparams(items, T, d, int(ModelKind.EWMA), LOSS_HINGE, B=8), E, bias)
    total = _units(seqs, T)
    assert g.sequence_ranks(ptr, it)[1].size == total > 0

    def refused(p, i, flags=0):
        out_ptr = np.full(users + 1, 77, np.uint64)
        out = np.full(total, 99, np.uint32)
        st = g._L.sbr_sequence_ranks(g._h, p.ctypes.data, i.ctypes.data, users, flags, 0, out_ptr.ctypes.data, out.ctypes.data)
        assert st == Status.INVALID_ARGUMENT
        assert (out_ptr == 77).all() and (out == 99).all(), "outputs untouched"

    bad = it.copy()
    bad[5] = items
    refused(ptr, bad)
    dec = ptr.copy()
    dec[3] = dec[4] + 1
    refused(dec, it)
    refused(ptr, it, flags=2)
    refused(ptr, it, flags=3)
    with pytest.raises(EngineError) as e:
        g.sequence_ranks(ptr, bad)
    assert e.value.status == Status.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        g.sequence_ranks(ptr, it, last=0)
    # no users; users without positions only
    p, r = g.sequence_ranks(np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert p.tolist() == [0] and r.size == 0
    p, r = g.sequence_ranks(np.array([0, 0, 1, 2], np.uint64), np.array([4, 5], np.uint32))
    assert p.tolist() == [0, 0, 0, 0] and r.size == 0
