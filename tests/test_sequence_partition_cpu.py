"""No device: the expectation of sbr_sequence_partition (sequence_partition_expect.py) against a brute-force float64 log-sum-exp,
sequence_log_likelihood_from_log_probs and golden_section_max on hand-made inputs, and the declarations and argument checks of
the new call that need no GPU."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from partition_expect import frac_bits, inv_temperature, log_z_expect
from sbr_rs_amd import _lib, evaluation
from sbr_rs_amd.engine import Model, Partition
from sbr_rs_amd.evaluation import golden_section_max, sequence_log_likelihood_from_log_probs
from sequence_partition_expect import expect_sequence_partition, flat, unresolved_rows
from test_partition_cpu import EXP32_MAX_REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sequence_partition_declared_and_abi_unchanged():
    header = open(os.path.join(ROOT, "include", "sbr_hip.h")).read()
    assert "sbr_sequence_partition" in _lib.DECLARED_SYMBOLS
    assert re.search(r"sbr_status\s+sbr_sequence_partition\(sbr_model\*\s*m,\s*const uint64_t\*\s*user_ptr,\s*const uint32_t\*\s*item_ids,\s*"
                     r"uint64_t num_users,\s*float temperature,\s*uint32_t flags,\s*uint32_t last_positions,\s*uint64_t\*\s*out_ptr,\s*"
                     r"float\*\s*out_shift,\s*uint64_t\*\s*out_mass,\s*float\*\s*out_scores,\s*uint8_t\*\s*out_masked\);", header)
    assert "#define SBR_ABI_VERSION 13u" in header and _lib.ABI_VERSION == 13
    L = _lib.load()  # loads without a device
    assert hasattr(L, "sbr_sequence_partition") and len(L.sbr_sequence_partition.argtypes) == 12
    hpp = open(os.path.join(ROOT, "include", "sbr.hpp")).read()
    for name in ("struct SequencePartition", "sequence_partition(", "sequence_log_probs(", "sequence_log_likelihood("):
        assert name in hpp


def test_signatures_and_defaults():
    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}

    assert defaults(Model.sequence_partition) == {"temperature": 1.0, "include_history": False, "last": None}
    assert defaults(evaluation.sequence_log_probs) == {"temperature": 1.0, "mask_history": True, "last": None}
    assert defaults(evaluation.sequence_log_likelihood) == {"temperature": 1.0, "mask_history": True, "last": None}
    assert defaults(evaluation.calibrate_temperature) == {"bounds": (0.01, 100.0), "evaluations": 24, "mask_history": True, "last": 1}
    assert list(inspect.signature(golden_section_max).parameters)[:4] == ["f", "lo", "hi", "evaluations"]
    from sbr_rs_amd.ewma import ImplicitEWMAModel
    from sbr_rs_amd.lstm import ImplicitLSTMModel

    for cls in (ImplicitLSTMModel, ImplicitEWMAModel):
        assert defaults(cls.sequence_log_probs) == {"temperature": 1.0, "mask_history": True, "last": None}
        assert defaults(cls.calibrate_temperature)["last"] == 1


def _table_fn(items, seed):
    """Scores that depend on the prefix (its length and last item)."""
    table = (np.random.RandomState(seed).randn(7, items, items) * 2).astype(np.float32)
    return lambda prefix: table[len(prefix) % 7, int(prefix[-1])]


@pytest.mark.parametrize("temperature", [0.5, 1.0, 4.0])
def test_expectation_against_a_float64_log_sum_exp(temperature):
    """40 items: log_z of every position against a brute-force float64 log-sum-exp over the eligible items, within the bound
    tests/test_partition_cpu.py holds log_z to (num_items 2^-F truncation plus the recorded exp32 error); the score is the
    table's, the flag a set lookup, a prefix that covers the catalogue has shift -inf and mass 0."""
    items, T = 40, 9
    fn = _table_fn(items, 3)
    rs = np.random.RandomState(4)
    seqs = [rs.randint(0, 3 + u % 38, size=n) for u, n in enumerate([0, 1, 2, 5, T, T + 1, T + 4, 7, 3] * 4)]
    seqs.append(np.arange(items - 1, -1, -1)[-T - 1:] % 4)  # few distinct items
    fb = frac_bits(items)
    bound = items * 2.0 ** -fb + EXP32_MAX_REL
    for mask in (True, False):
        for last in (None, 2):
            rows = expect_sequence_partition(fn, seqs, T, temperature, mask_history=mask, last=last)
            assert len(rows) == len(seqs)
            checked = 0
            for seq, (shift, mass, score, masked) in zip(seqs, rows):
                seq = [int(x) for x in seq]
                W = min(len(seq), T + 1)
                w = seq[len(seq) - W:]
                pos = list(range(1, W))
                pos = pos if last is None else pos[max(0, len(pos) - last):]
                assert shift.size == mass.size == score.size == masked.size == len(pos)
                assert shift.dtype == np.uint32 and mass.dtype == np.uint64 and score.dtype == np.uint32 and masked.dtype == np.uint8
                for j, p in enumerate(pos):
                    s = fn(np.array(w[:p], np.uint32))
                    ok = [i for i in range(items) if not (mask and i in set(w[:p]))]
                    t = (s[ok] * inv_temperature(temperature)).astype(np.float64)  # the f32 product, as test_partition_cpu.py takes it
                    want = t.max() + math.log(np.exp(t - t.max()).sum())
                    got = log_z_expect(shift[j: j + 1].view(np.float32), mass[j: j + 1], fb)[0]
                    assert abs(got - want) <= bound
                    assert score[j] == np.float32(s[w[p]]).view(np.uint32) and masked[j] == (1 if mask and w[p] in w[:p] else 0)
                    checked += 1
            assert checked > 50
    # a prefix that covers the whole catalogue: nothing is eligible
    small = lambda prefix: np.arange(3, dtype=np.float32)  # noqa: E731
    (shift, mass, score, masked), = expect_sequence_partition(small, [[0, 1, 2, 1]], 5, temperature)
    assert np.isneginf(shift.view(np.float32)[2]) and mass.tolist()[2] == 0 and masked.tolist() == [0, 0, 1]
    assert not np.isneginf(shift.view(np.float32)[:2]).any() and score.view(np.float32).tolist() == [1.0, 2.0, 1.0]
    (shift2, mass2, _s, masked2), = expect_sequence_partition(small, [[0, 1, 2, 1]], 5, temperature, mask_history=False)
    assert masked2.tolist() == [0, 0, 0] and (mass2 > 0).all()
    assert [a.size for a in flat([])] == [0, 0, 0, 0]
    # unresolved_rows: the two best items of the catalogue in the prefix, a pool of 2
    assert unresolved_rows(small, [[2, 1, 0]], 5, pool=2) == 1 and unresolved_rows(small, [[2, 1, 0]], 5, pool=1) == 2
    assert unresolved_rows(small, [[0, 1, 0]], 5, pool=1) == 0


def test_log_prob_of_a_partition_row_is_log_w_over_mass():
    """What sequence_log_probs does on the host with one position's four values."""
    fn = _table_fn(12, 8)
    (shift, mass, score, masked), = expect_sequence_partition(fn, [[3, 5, 3, 7]], 6, 2.0)
    part = Partition(2.0, shift.view(np.float32), mass, frac_bits(12))
    lp = part.log_prob(score.view(np.float32)[:, None])[:, 0]
    assert masked.tolist() == [0, 1, 0] and np.all(lp <= 0) and np.all(np.isfinite(lp))
    for p, pre in ((0, [3]), (2, [3, 5, 3])):
        t = (fn(np.array(pre, np.uint32)) * inv_temperature(2.0)).astype(np.float64)
        ok = [i for i in range(12) if i not in pre]
        want = t[[5, 3, 7][p]] - math.log(np.exp(t[ok]).sum())
        # log mass to test_partition_cpu.py's bound; log w to the exp32 error plus its truncation, 2^-F relative to w = e^d 2^F
        d = t[[5, 3, 7][p]] - t[ok].max()
        assert abs(lp[p] - want) <= (12 * 2.0 ** -40 + EXP32_MAX_REL) + (EXP32_MAX_REL + 2.0 ** -40 * math.exp(-d))


def test_sequence_log_likelihood_from_log_probs_by_hand():
    inf = -np.inf
    rows = [np.array([-1.0, inf, -3.0]), np.zeros(0), np.array([inf]), np.array([-2.0, -4.0])]
    m = sequence_log_likelihood_from_log_probs(rows)
    assert m["positions"] == 4 and m["masked_positions"] == 2
    assert m["mean_log_prob"] == pytest.approx(-10.0 / 4, rel=1e-15) and m["perplexity"] == pytest.approx(math.exp(2.5), rel=1e-15)
    assert m["macro"]["users"] == 2  # the user whose one position is masked is left out, as is the one without positions
    assert m["macro"]["mean_log_prob"] == pytest.approx((-2.0 + -3.0) / 2, rel=1e-15)
    assert m["macro"]["perplexity"] == pytest.approx(math.exp(2.5), rel=1e-15)
    by = m["by_history_length"]
    assert by["count"].tolist() == [0, 2, 1, 1] and by["masked"].tolist() == [0, 1, 1, 0] and by["count"].dtype == np.int64
    assert by["mean_log_prob"][1] == -1.5 and by["mean_log_prob"][2] == -4.0 and by["mean_log_prob"][3] == -3.0
    assert by["perplexity"][3] == pytest.approx(math.exp(3.0), rel=1e-15) and math.isnan(by["mean_log_prob"][0])
    by5 = sequence_log_likelihood_from_log_probs(rows, max_sequence_length=5)["by_history_length"]
    assert by5["count"].tolist() == [0, 2, 1, 1, 0, 0] and math.isnan(by5["mean_log_prob"][4])
    with pytest.raises(ValueError):
        sequence_log_likelihood_from_log_probs(rows, max_sequence_length=2)
    for empty in ([], [np.zeros(0)] * 3, [np.array([inf, inf])]):
        e = sequence_log_likelihood_from_log_probs(empty)
        assert e["positions"] == 0 and math.isnan(e["mean_log_prob"]) and math.isnan(e["perplexity"]) and e["macro"]["users"] == 0
        assert math.isnan(e["macro"]["mean_log_prob"])
    assert sequence_log_likelihood_from_log_probs([np.array([inf, inf])])["masked_positions"] == 2
    with pytest.raises(ValueError):
        sequence_log_likelihood_from_log_probs([np.array([0.5])])
    with pytest.raises(ValueError):
        sequence_log_likelihood_from_log_probs([np.array([np.nan])])


def test_golden_section_max_on_concave_functions():
    calls = []

    def f(x):
        calls.append(x)
        return -(x - 2.0) ** 2 + 3.0

    x, fx = golden_section_max(f, 0.0, 10.0, 40)
    # 40 evaluations leave a bracket of 10 * 0.618^38 = 1.1e-7; a parabola is flat to within rounding over sqrt(eps) = 1.5e-8
    assert len(calls) == 40 and abs(x - 2.0) < 1e-6 and fx == f(x) and fx == max(-(c - 2.0) ** 2 + 3.0 for c in calls[:40])
    assert all(0.0 < c < 10.0 for c in calls)
    # the shape of the calibration: a linear term minus a log-sum-exp — one item of score 1 that is the target half of the time
    # among three of score 0: g'(b) = 1/2 - e^b / (e^b + 3) = 0 at b = log 3
    g = lambda b: 0.5 * b - math.log(math.exp(b) + 3.0)  # noqa: E731
    x, gx = golden_section_max(g, 0.01, 100.0, 48)
    assert abs(x - math.log(3.0)) < 1e-5 and gx == g(x) and gx == pytest.approx(0.5 * math.log(3.0) - math.log(6.0), abs=1e-12)
    # a maximum at either end, and -inf over the upper part of the bracket (the search moves to where f is finite)
    assert golden_section_max(lambda x: -x, 1.0, 2.0, 30)[0] == pytest.approx(1.0, abs=1e-5)
    assert golden_section_max(lambda x: x, 1.0, 2.0, 30)[0] == pytest.approx(2.0, abs=1e-5)
    h = lambda x: -np.inf if x > 5.0 else -(x - 4.0) ** 2  # noqa: E731
    assert golden_section_max(h, 0.0, 100.0, 40)[0] == pytest.approx(4.0, abs=1e-4)
    for bad in ((1.0, 1.0, 10), (2.0, 1.0, 10), (0.0, 1.0, 1)):
        with pytest.raises(ValueError):
            golden_section_max(f, *bad)


def test_sequence_partition_argument_checks_without_a_device():
    """What the binding refuses before it reaches the library, on an object that has no engine handle."""
    m = Model.__new__(Model)
    ptr, it = np.array([0, 3], np.uint64), np.array([1, 2, 3], np.uint32)
    for last in (0, -1, 2 ** 32):
        with pytest.raises(ValueError):
            m.sequence_partition(ptr, it, last=last)
    for t in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            m.sequence_partition(ptr, it, temperature=t)
    with pytest.raises(ValueError):
        m.sequence_partition(np.zeros(0, np.uint64), it)
    with pytest.raises(ValueError):
        m.sequence_partition(np.zeros((2, 2), np.uint64), it)
    for bounds in ((0.0, 1.0), (2.0, 1.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            evaluation.calibrate_temperature(m, None, bounds=bounds)
    # the library's own checks that come before any device work
    L = _lib.load()
    out_ptr = np.full(2, 77, np.uint64)
    assert L.sbr_sequence_partition(None, ptr.ctypes.data, it.ctypes.data, 1, 1.0, 0, 0, out_ptr.ctypes.data, None, None, None, None) != 0
    assert (out_ptr == 77).all()
