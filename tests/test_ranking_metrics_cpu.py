"""CPU: sbr.evaluation.ranking_metrics_from_ranks (pure numpy) against an independent list-based implementation that builds
each user's whole ordering from its scores, marks relevance along it and computes the textbook formulas; and the hold-out split
of ranking_metrics.  No device is used.

Tolerances.  precision, recall and hit rate are ratios of small integers: compared exactly.  NDCG is a ratio of two float64 sums
of at most 1 024 terms of magnitude <= 1, summed in different orders by the two implementations: each sum carries at most
k x 2^-53, about 1.1e-13, of relative error, so per-user values must agree to a relative 1e-12."""
import math

import numpy as np
import pytest

import sbr_rs_amd as sbr
from sbr_rs_amd.data import CompressedInteractions
from sbr_rs_amd.evaluation import holdout_split, ranking_metrics_from_ranks

KS = (1, 5, 10, 100, 1024)


def _ranks_from_scores(scores, relevant):
    """The catalogue rank of each relevant item under the reference's rule: #{i : s_i >= s_t}."""
    return np.array([int(np.count_nonzero(scores >= scores[t])) for t in relevant], np.uint32)


def _textbook(scores, relevant, ks):
    """List-based metrics of one user: the full ordering best first, a tie placed AFTER everything it ties with (the pessimistic
    position `>=` gives a relevant item; relevant items that tie share that position), relevance marked along the list."""
    n = len(scores)
    rel = set(int(t) for t in relevant)
    # position of item t (1-based): all items with a higher score, then every item of its own tie class
    pos = {t: sum(1 for i in range(n) if scores[i] >= scores[t]) for t in rel}
    out = {}
    for k in ks:
        hit_positions = sorted(p for p in pos.values() if p <= k)
        hits = len(hit_positions)
        dcg = math.fsum(1.0 / math.log2(1.0 + p) for p in hit_positions)
        idcg = math.fsum(1.0 / math.log2(1.0 + j) for j in range(1, min(len(rel), k) + 1))
        out[k] = (hits / k, hits / len(rel), 1.0 if hits else 0.0, dcg / idcg)
    best = min(pos.values())
    return out, 1.0 / best, math.fsum(pos.values()) / len(pos)


def _check_against_textbook(all_scores, all_relevant, ks=KS):
    ranks = [_ranks_from_scores(s, r) if len(r) else np.zeros(0, np.uint32) for s, r in zip(all_scores, all_relevant)]
    m = ranking_metrics_from_ranks(ranks, ks)
    ranked = [u for u, r in enumerate(all_relevant) if len(r)]
    assert m["num_users_ranked"] == len(ranked) and m["users"].tolist() == ranked and m["ks"] == tuple(ks)
    per = m["per_user"]
    for j, u in enumerate(ranked):
        want, mrr, mean_rank = _textbook(all_scores[u], all_relevant[u], ks)
        for k in ks:
            p, r, h, ndcg = want[k]
            assert per["precision"][k][j] == p and per["recall"][k][j] == r and per["hit_rate"][k][j] == h, (u, k)
            assert per["ndcg"][k][j] == pytest.approx(ndcg, rel=1e-12, abs=0.0), (u, k)
            assert 0.0 <= per["ndcg"][k][j] <= 1.0
        assert per["mrr"][j] == mrr
        assert per["mean_rank"][j] == pytest.approx(mean_rank, rel=1e-12)
    for name in ("precision", "recall", "hit_rate", "ndcg"):
        for k in ks:
            assert m[name][k] == pytest.approx(float(np.mean(per[name][k])), rel=1e-15) if ranked else math.isnan(m[name][k])
    return m


def test_metrics_random_scores():
    rs = np.random.RandomState(1)
    scores = [rs.randn(400) for _ in range(60)]
    relevant = [rs.choice(400, rs.randint(0, 30), replace=False) for _ in range(60)]
    relevant[3] = np.zeros(0, np.int64)  # users without targets are left out
    m = _check_against_textbook(scores, relevant)
    assert 0 < m["num_users_ranked"] < 60
    assert m["recall"][1024] == 1.0 and m["hit_rate"][1024] == 1.0  # k beyond the catalogue


def test_metrics_tied_scores():
    """Scores from 6 values: most relevant items tie with many others and with each other; NDCG stays <= 1 because a relevant
    item's rank counts every item it ties with, the other relevant ones included."""
    rs = np.random.RandomState(2)
    scores = [rs.randint(0, 6, 300).astype(np.float64) for _ in range(40)]
    relevant = [rs.choice(300, rs.randint(1, 40), replace=False) for _ in range(40)]
    scores.append(np.zeros(300))  # everything ties: every rank is 300
    relevant.append(np.arange(5))
    m = _check_against_textbook(scores, relevant)
    assert m["per_user"]["hit_rate"][100][-1] == 0.0 and m["per_user"]["mean_rank"][-1] == 300.0


@pytest.mark.parametrize("r,k", [(3, 10), (10, 3), (5, 5), (1, 1), (40, 1024)])
def test_metrics_more_and_fewer_relevant_than_k(r, k):
    scores = np.arange(100, 0, -1).astype(np.float64)  # item i is at position i + 1
    m = _check_against_textbook([scores], [np.arange(r)], ks=(k,))  # the r best items are the relevant ones
    assert m["ndcg"][k] == pytest.approx(1.0, rel=1e-12) and m["precision"][k] == min(r, k) / k and m["recall"][k] == min(r, k) / r
    m = _check_against_textbook([scores], [np.arange(99, 99 - r, -1)], ks=(k,))  # the r worst
    assert m["ndcg"][k] == 0.0 or k + r > 100


def test_metrics_hand_computed():
    m = ranking_metrics_from_ranks([[1, 3], [], [7], [2, 2, 50]], ks=(2, 5))
    assert m["num_users_ranked"] == 3 and m["users"].tolist() == [0, 2, 3]
    assert m["per_user"]["precision"][2].tolist() == [0.5, 0.0, 1.0] and m["per_user"]["recall"][2].tolist() == [0.5, 0.0, 2 / 3]
    assert m["per_user"]["hit_rate"][5].tolist() == [1.0, 0.0, 1.0]
    ideal2 = 1.0 + 1.0 / math.log2(3.0)
    assert m["per_user"]["ndcg"][5][0] == pytest.approx((1.0 + 0.5) / ideal2, rel=1e-12)
    assert m["per_user"]["ndcg"][2][2] == pytest.approx((2.0 / math.log2(3.0)) / ideal2, rel=1e-12) and m["per_user"]["ndcg"][2][2] <= 1.0
    assert m["per_user"]["mrr"].tolist() == [1.0, 1 / 7, 0.5] and m["per_user"]["mean_rank"].tolist() == [2.0, 7.0, 18.0]
    assert m["mrr"] == pytest.approx((1.0 + 1 / 7 + 0.5) / 3, rel=1e-15)


def test_metrics_empty_input_and_errors():
    for ranks in ([], [[], []]):
        m = ranking_metrics_from_ranks(ranks, ks=(10,))
        assert m["num_users_ranked"] == 0 and m["users"].size == 0
        assert math.isnan(m["mrr"]) and math.isnan(m["mean_rank"]) and math.isnan(m["ndcg"][10]) and math.isnan(m["recall"][10])
    with pytest.raises(ValueError):
        ranking_metrics_from_ranks([[1]], ks=(0,))
    with pytest.raises(ValueError):
        ranking_metrics_from_ranks([[0]], ks=(1,))


def _compressed(seqs, num_items=50):
    ptr = np.zeros(len(seqs) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(s) for s in seqs])
    items = np.concatenate([np.asarray(s, np.uint32) for s in seqs] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return CompressedInteractions(len(seqs), num_items, ptr, items, np.arange(items.size, dtype=np.uint64))


def test_holdout_split():
    seqs = [[1, 2, 3, 4, 5], [], [7], [8, 9], [1, 2, 3], [4, 4, 6, 4, 6, 9], [5, 5, 5, 5]]
    test = _compressed(seqs)
    users, hists, targets = holdout_split(test, 1)
    assert users.tolist() == [0, 3, 4, 5, 6]  # the reference's >= 2 items
    assert [h.tolist() for h in hists] == [[1, 2, 3, 4], [8], [1, 2], [4, 4, 6, 4, 6], [5, 5, 5]]
    assert [t.tolist() for t in targets] == [[5], [9], [3], [9], [5]]
    users, hists, targets = holdout_split(test, 3)
    assert users.tolist() == [0, 5, 6]  # sequences shorter than holdout + 1 are skipped, 3 items included
    assert [h.tolist() for h in hists] == [[1, 2], [4, 4, 6], [5]]
    assert [t.tolist() for t in targets] == [[3, 4, 5], [4, 6, 9], [5]]  # de-duplicated, first occurrence kept
    users, hists, targets = holdout_split(test, 6)
    assert users.size == 0 and hists == [] and targets == []
    with pytest.raises(ValueError):
        holdout_split(test, 0)


def test_python_surface():
    for name in ("ranking_metrics", "ranking_metrics_from_ranks", "rank_targets", "holdout_split", "mrr_score"):
        assert callable(getattr(sbr.evaluation, name)), name
    from sbr_rs_amd.engine import Model

    assert callable(Model.rank_targets) and callable(Model.rank_targets_reps)
    assert callable(sbr.lstm.ImplicitLSTMModel.rank_targets) and callable(sbr.ewma.ImplicitEWMAModel.rank_targets)
