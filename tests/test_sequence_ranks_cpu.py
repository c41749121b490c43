"""No device: the expectation of sbr_sequence_ranks (sequence_expect.py) against a brute-force restatement on hand-made score
tables, sequence_metrics_from_ranks against hand-computed values, and the argument checks and declarations of the new call that
need no GPU."""
import math
import os
import re

import numpy as np
import pytest

from sbr_rs_amd import _lib
from sbr_rs_amd.engine import Model
from sbr_rs_amd.evaluation import sequence_metrics_from_ranks
from sequence_expect import expect_sequence_ranks, kept_positions, window_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MIN = float(np.finfo(np.float32).min)


def _table_fn(items, seed):
    """Scores that depend on the prefix (its length and last item) and tie heavily: small integers."""
    rs = np.random.RandomState(seed)
    table = rs.randint(-3, 4, size=(7, items, items)).astype(np.float32)

    def fn(prefix):
        return table[len(prefix) % 7, int(prefix[-1])]

    return fn


def _brute(score_fn, seqs, T, mask=True, last=None):
    """The contract of include/sbr_hip.h word for word, with Python loops and sets."""
    out = []
    for seq in seqs:
        seq = [int(x) for x in seq]
        W = min(len(seq), T + 1)
        w = seq[len(seq) - W:]
        row = []
        for p in range(1, W):
            s = [float(x) for x in score_fn(np.array(w[:p], np.uint32))]
            seen = set(w[:p]) if mask else set()
            m = [F32_MIN if i in seen else s[i] for i in range(len(s))]
            row.append(sum(1 for x in m if x >= m[w[p]]))
        if last is not None:
            row = row[max(0, len(row) - last):]
        out.append(np.array(row, dtype=np.uint32))
    return out


def test_expectation_equals_brute_force():
    items, T = 23, 5
    fn = _table_fn(items, 1)
    rs = np.random.RandomState(2)
    seqs = [rs.randint(0, 6 + u % 17, size=n) for u, n in enumerate([0, 1, 2, 3, T, T + 1, T + 2, T + 9, 4, 6, 2, 11] * 3)]
    for mask in (True, False):
        for last in (None, 1, 3, 50):
            got = expect_sequence_ranks(fn, seqs, T, mask_history=mask, last=last)
            want = _brute(fn, seqs, T, mask=mask, last=last)
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g.dtype == np.uint32 and np.array_equal(g, w)


def test_expectation_edge_cases_by_hand():
    items = 6
    scores = np.array([5, 4, 4, 3, 2, 1], np.float32)  # the same for every prefix; items 1 and 2 tie
    fn = lambda prefix: scores  # noqa: E731
    T = 3
    # n = 0, 1: empty rows; n = 2: one position
    assert [r.tolist() for r in expect_sequence_ranks(fn, [[], [3], [0, 3]], T)] == [[], [], [3]]  # 5 masked: 4, 4, 3 >= 3
    # target in its own prefix -> num_items, masked or not only when masked
    assert expect_sequence_ranks(fn, [[3, 0, 3]], T)[0].tolist() == [1, items]
    assert expect_sequence_ranks(fn, [[3, 0, 3]], T, mask_history=False)[0].tolist() == [1, 4]
    # a repeated prefix item is masked once: prefix (0, 0, 0) removes ONE item above the target 4 (score 2): 4, 4, 3, 2
    assert expect_sequence_ranks(fn, [[0, 0, 0, 4]], T)[0].tolist() == [items, items, 4]
    # ties count against the target: target 1 ties with 2
    assert expect_sequence_ranks(fn, [[5, 1]], T)[0].tolist() == [3]
    assert expect_sequence_ranks(fn, [[5, 2]], T)[0].tolist() == [3]
    # the window is the last T + 1 = 4 items: item 0 before it is neither masked nor in any prefix
    seq = [0, 5, 4, 3, 2]
    assert window_of(seq, T).tolist() == [5, 4, 3, 2]
    assert expect_sequence_ranks(fn, [seq], T)[0].tolist() == [5, 4, 3]  # target 4 (score 2): 5, 4, 4, 3, 2 — item 0 counts
    seen = []
    expect_sequence_ranks(lambda p: (seen.append(p.tolist()), scores)[1], [seq], T)
    assert seen == [[5], [5, 4], [5, 4, 3]]
    # last keeps the tail
    assert expect_sequence_ranks(fn, [seq], T, last=2)[0].tolist() == [4, 3]
    assert expect_sequence_ranks(fn, [seq], T, last=9)[0].tolist() == [5, 4, 3]
    assert kept_positions(1) == [] and kept_positions(0) == [] and kept_positions(4, 1) == [3]


def test_sequence_metrics_from_ranks_by_hand():
    rows = [np.array([1, 4], np.uint32), np.zeros(0, np.uint32), np.array([2], np.uint32), np.array([20, 1, 3], np.uint32)]
    m = sequence_metrics_from_ranks(rows, ks=(1, 3))
    assert m["ks"] == (1, 3) and m["num_positions"] == 6 and m["num_users_ranked"] == 3
    assert m["mrr"] == pytest.approx((1 + 1 / 4 + 1 / 2 + 1 / 20 + 1 + 1 / 3) / 6, rel=1e-15)
    assert m["mean_rank"] == pytest.approx(31 / 6, rel=1e-15)
    assert m["hit_rate"] == {1: pytest.approx(2 / 6), 3: pytest.approx(4 / 6)}
    g = lambda r: 1 / math.log2(1 + r)  # noqa: E731
    assert m["ndcg"][1] == pytest.approx(2 * g(1) / 6, rel=1e-15)
    assert m["ndcg"][3] == pytest.approx((2 * g(1) + g(2) + g(3)) / 6, rel=1e-15)
    mac = m["macro"]
    assert mac["mrr"] == pytest.approx(((1 + 1 / 4) / 2 + 1 / 2 + (1 / 20 + 1 + 1 / 3) / 3) / 3, rel=1e-15)
    assert mac["mean_rank"] == pytest.approx((2.5 + 2 + 8) / 3, rel=1e-15)
    assert mac["hit_rate"][1] == pytest.approx((1 / 2 + 0 + 1 / 3) / 3, rel=1e-15)
    assert mac["hit_rate"][3] == pytest.approx((1 / 2 + 1 + 2 / 3) / 3, rel=1e-15)
    assert mac["ndcg"][3] == pytest.approx((g(1) / 2 + g(2) + (g(1) + g(3)) / 3) / 3, rel=1e-15)
    by = m["by_history_length"]
    assert by["count"].tolist() == [0, 3, 2, 1] and by["count"].dtype == np.int64
    assert by["mrr"][1] == pytest.approx((1 + 1 / 2 + 1 / 20) / 3, rel=1e-15) and by["mrr"][2] == pytest.approx((1 / 4 + 1) / 2, rel=1e-15)
    assert by["mean_rank"][3] == 3.0 and by["hit_rate"][3][3] == 1.0 and by["hit_rate"][1][3] == 0.0
    assert by["ndcg"][3][2] == pytest.approx(g(1) / 2, rel=1e-15) and math.isnan(by["mrr"][0])
    # max_sequence_length pads the arrays; a shorter one is refused
    by5 = sequence_metrics_from_ranks(rows, ks=(1,), max_sequence_length=5)["by_history_length"]
    assert by5["count"].tolist() == [0, 3, 2, 1, 0, 0] and math.isnan(by5["mrr"][4]) and math.isnan(by5["ndcg"][1][5])
    with pytest.raises(ValueError):
        sequence_metrics_from_ranks(rows, ks=(1,), max_sequence_length=2)
    # a user with one position: micro = macro = that position
    one = sequence_metrics_from_ranks([np.array([5], np.uint32)], ks=(10,))
    assert one["num_positions"] == 1 and one["mrr"] == one["macro"]["mrr"] == 0.2
    assert one["ndcg"][10] == one["macro"]["ndcg"][10] == pytest.approx(g(5), rel=1e-15) and one["hit_rate"][10] == 1.0
    assert one["by_history_length"]["count"].tolist() == [0, 1]
    # empty input, and only empty rows
    for empty in ([], [np.zeros(0, np.uint32)] * 3):
        e = sequence_metrics_from_ranks(empty, ks=(10, 100))
        assert e["num_positions"] == 0 and e["num_users_ranked"] == 0 and math.isnan(e["mrr"]) and math.isnan(e["macro"]["mean_rank"])
        assert math.isnan(e["hit_rate"][10]) and math.isnan(e["macro"]["ndcg"][100]) and e["by_history_length"]["count"].tolist() == [0]
    with pytest.raises(ValueError):
        sequence_metrics_from_ranks(rows, ks=(0,))
    with pytest.raises(ValueError):
        sequence_metrics_from_ranks([np.array([0], np.uint32)])


def test_sequence_ranks_declared_and_abi_unchanged():
    header = open(os.path.join(ROOT, "include", "sbr_hip.h")).read()
    assert "sbr_sequence_ranks" in _lib.DECLARED_SYMBOLS
    assert re.search(r"sbr_status\s+sbr_sequence_ranks\(sbr_model\*\s*m,\s*const uint64_t\*\s*user_ptr,\s*const uint32_t\*\s*item_ids,\s*"
                     r"uint64_t num_users,\s*uint32_t flags,\s*uint32_t last_positions,\s*uint64_t\*\s*out_ptr,\s*uint32_t\*\s*out_ranks\);", header)
    assert "#define SBR_ABI_VERSION 13u" in header and _lib.ABI_VERSION == 13
    L = _lib.load()  # loads without a device
    assert hasattr(L, "sbr_sequence_ranks") and len(L.sbr_sequence_ranks.argtypes) == 8
    hpp = open(os.path.join(ROOT, "include", "sbr.hpp")).read()
    assert "sequence_ranks(" in hpp and "struct SequenceMetrics" in hpp and "sequence_metrics(" in hpp


def test_sequence_ranks_argument_checks_without_a_device():
    """What the binding refuses before it reaches the library, on an object that has no engine handle."""
    m = Model.__new__(Model)
    ptr, it = np.array([0, 3], np.uint64), np.array([1, 2, 3], np.uint32)
    for last in (0, -1, 2 ** 32):
        with pytest.raises(ValueError):
            m.sequence_ranks(ptr, it, last=last)
    with pytest.raises(ValueError):
        m.sequence_ranks(np.zeros(0, np.uint64), it)
    with pytest.raises(ValueError):
        m.sequence_ranks(np.zeros((2, 2), np.uint64), it)
    # the library's own checks that come before any device work
    L = _lib.load()
    out_ptr = np.full(2, 77, np.uint64)
    assert L.sbr_sequence_ranks(None, ptr.ctypes.data, it.ctypes.data, 1, 0, 0, out_ptr.ctypes.data, None) != 0
    assert (out_ptr == 77).all()
