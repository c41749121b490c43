"""CPU: the host side of the *_above calls.  tests/above_expect.py — the numpy restatement the GPU tests compare against — is held to
a brute-force loop; the Python layer's order sort (engine.above_sort) and the Above accessors run on hand-made CSR; the new methods'
signatures and defaults are the issue's.  No device is touched."""
import inspect

import numpy as np
import pytest

from above_expect import above_expect, counts_expect, transposed
from sbr_rs_amd import engine, lstm
from sbr_rs_amd.engine import ABOVE_MAX_RESULTS, Above, above_sort


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _brute(scores, thresholds, excluded, allowed, order):
    """the contract as loops over single f32 values"""
    ptr, ids, out = [0], [], []
    for r in range(scores.shape[0]):
        row = []
        for c in range(scores.shape[1]):
            if not (scores[r, c] >= thresholds[r]):
                continue
            if allowed is not None and not allowed[r, c]:
                continue
            if excluded is not None and c in set(int(x) for x in excluded[r]):
                continue
            row.append((c, scores[r, c]))
        if order == "score":
            done = []
            while row:  # selection by the total order: the best score, the lowest column among equals
                best = 0
                for j in range(1, len(row)):
                    if row[j][1] > row[best][1] or (row[j][1] == row[best][1] and row[j][0] < row[best][0]):
                        best = j
                done.append(row.pop(best))
            row = done
        ids += [c for c, _ in row]
        out += [s for _, s in row]
        ptr.append(len(ids))
    return np.array(ptr, np.uint64), np.array(ids, np.uint32), np.array(out, np.float32)


@pytest.mark.parametrize("order", ["score", "id"])
@pytest.mark.parametrize("tied", [False, True])
def test_above_expect_against_a_brute_force_loop(order, tied):
    rs = np.random.RandomState(3 + tied)
    rows, cols = 9, 70
    scores = rs.randn(rows, cols).astype(np.float32)
    if tied:  # few distinct values, signed zeros among them
        scores = (np.round(scores * 2) / 2).astype(np.float32)
        scores[scores == 0] = np.where(rs.rand(np.count_nonzero(scores == 0)) < 0.5, np.float32(-0.0), np.float32(0.0))
        assert np.signbit(scores[scores == 0]).any() and not np.signbit(scores[scores == 0]).all()
    th = np.array([-np.inf, np.inf, 0.0, -0.0, 0.5, -0.5, 1.0, scores[7].max(), scores[8].min()], np.float32)
    excluded = [rs.randint(0, cols, rs.randint(0, 12)) for _ in range(rows)]
    allowed = rs.rand(rows, cols) < 0.7
    for ex, al in ((None, None), (excluded, None), (None, allowed), (excluded, allowed)):
        got = above_expect(scores, th, ex, al, order)
        want = _brute(scores, th, ex, al, order)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2]))
        assert np.array_equal(counts_expect(scores, th, ex, al), np.diff(want[0]))
    plain = above_expect(scores, th, None, None, order)
    assert np.diff(plain[0])[0] == cols and np.diff(plain[0])[1] == 0 and np.diff(plain[0])[7] >= 1 and np.diff(plain[0])[8] == cols
    named = above_expect(scores, th, None, None, order, ids=np.arange(cols) * 3 + 1)
    assert np.array_equal(named[1], plain[1] * 3 + 1)
    assert len(transposed(*plain, rows)) == int(plain[0][-1])


def test_above_sort_and_the_accessors():
    """Three rows in id order: the score order is stable on top of it — equal scores, and -0.0 against +0.0, keep the lower id first —
    and a row's zero keeps the sign it came with."""
    ptr = np.array([0, 5, 5, 8], np.uint64)
    ids = np.array([2, 3, 7, 9, 11, 1, 4, 6], np.uint32)
    scores = np.array([1.0, 2.0, 1.0, -0.0, 0.0, 0.5, 0.5, 3.0], np.float32)
    same_i, same_s = above_sort(ptr, ids, scores, "id")
    assert np.array_equal(same_i, ids) and np.array_equal(_bits(same_s), _bits(scores))
    si, ss = above_sort(ptr, ids, scores, "score")
    assert si.tolist() == [3, 2, 7, 9, 11, 6, 1, 4]
    assert np.array_equal(_bits(ss), _bits(np.array([2.0, 1.0, 1.0, -0.0, 0.0, 3.0, 0.5, 0.5], np.float32)))
    with pytest.raises(ValueError):
        above_sort(ptr, ids, scores, "rank")
    empty = above_sort(np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), "score")
    assert empty[0].size == 0 and empty[1].size == 0
    a = Above(ptr, si, ss, "score")
    assert len(a) == 3 and a.counts.tolist() == [5, 0, 3] and a.order == "score"
    assert a.row(0)[0].tolist() == [3, 2, 7, 9, 11] and a.row(1)[0].size == 0 and a.row(2)[1].tolist() == [3.0, 0.5, 0.5]
    rows, pi, ps = a.pairs()
    assert rows.tolist() == [0, 0, 0, 0, 0, 2, 2, 2] and pi is a.ids and ps is a.scores
    # against the expectation's own order on a score matrix
    rs = np.random.RandomState(8)
    m = (np.round(rs.randn(6, 40) * 2) / 2).astype(np.float32)
    by_id, by_score = above_expect(m, -0.5, order="id"), above_expect(m, -0.5, order="score")
    gi, gs = above_sort(by_id[0], by_id[1], by_id[2], "score")
    assert np.array_equal(gi, by_score[1]) and np.array_equal(_bits(gs), _bits(by_score[2]))


def _params(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_signatures_and_defaults():
    E = inspect.Parameter.empty
    assert ABOVE_MAX_RESULTS == 1 << 24
    assert _params(engine.Model.recommend_above) == {"user_ptr": E, "item_ids": E, "threshold": E, "include_history": False, "any_of": None,
                                                     "none_of": None, "max_results": None, "order": "score"}
    assert _params(engine.Model.recommend_above_reps) == {"reps": E, "threshold": E, "exclude": None, "any_of": None, "none_of": None,
                                                          "max_results": None, "order": "score"}
    assert _params(engine.Model.audience_above_reps) == {"reps": E, "items": E, "threshold": E, "exclude": None, "max_results": None,
                                                         "order": "score"}
    assert _params(engine.Model.audience_above) == {"user_ptr": E, "item_ids": E, "items": E, "threshold": E, "include_history": False,
                                                    "max_results": None, "order": "score"}
    assert _params(engine.Sessions.recommend_above) == {"slots": E, "threshold": E, "exclude": None, "any_of": None, "none_of": None,
                                                        "include_seen": False, "max_results": None, "order": "score"}
    assert _params(engine.Sessions.audience_above) == {"items": E, "threshold": E, "slots": None, "exclude": None, "include_seen": False,
                                                       "max_results": None, "order": "score"}
    # a count form beside each, with the same leading arguments and neither max_results nor order
    for owner, name, count in ((engine.Model, "recommend_above", "count_above"), (engine.Model, "recommend_above_reps", "count_above_reps"),
                               (engine.Model, "audience_above", "count_audience_above"),
                               (engine.Model, "audience_above_reps", "count_audience_above_reps"),
                               (engine.Sessions, "recommend_above", "count_above"), (engine.Sessions, "audience_above", "count_audience_above")):
        full = _params(getattr(owner, name))
        assert _params(getattr(owner, count)) == {k: v for k, v in full.items() if k not in ("max_results", "order")}, count
    # the model classes spell the arguments as their sibling calls do
    M = lstm._ImplicitSequenceModel
    assert _params(M.recommend_above) == {"interactions_or_histories": E, "threshold": E, "exclude_history": True, "any_of": None,
                                          "none_of": None, "max_results": None, "order": "score"}
    assert _params(M.audience_above) == {"interactions_or_histories": E, "items": E, "threshold": E, "exclude_history": True,
                                         "max_results": None, "order": "score"}
    assert _params(M.recommend_above_reps) == _params(engine.Model.recommend_above_reps)
    assert _params(M.audience_above_reps) == _params(engine.Model.audience_above_reps)
    for name in ("count_above", "count_above_reps", "count_audience_above", "count_audience_above_reps"):
        assert callable(getattr(M, name))


def test_thresholds_argument():
    """a scalar broadcasts, an array must fit, a NaN is refused before anything is called"""
    from sbr_rs_amd.engine import _above_thresholds

    assert np.array_equal(_above_thresholds(0.5, 3), np.full(3, 0.5, np.float32))
    assert np.array_equal(_above_thresholds([1, -np.inf, np.inf], 3), np.array([1, -np.inf, np.inf], np.float32))
    assert _above_thresholds(1.0, 0).size == 1  # a valid pointer for an empty call
    with pytest.raises(ValueError):
        _above_thresholds([1.0, 2.0], 3)
    with pytest.raises(ValueError):
        _above_thresholds([1.0, np.nan, 2.0], 3)
    with pytest.raises(ValueError):
        _above_thresholds(np.nan, 2)
