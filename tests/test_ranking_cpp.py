"""GPU: the C++ host layer's rank_targets / ranking_metrics (include/sbr.hpp, tests/cpp/ranking_tests.cpp) on a
MovieLens-trained LSTM give the ranks of the Python call on the same model exactly and its metrics to 1e-12 (float64 sums of
fewer than 1 000 per-user values of magnitude <= 1 taken in different orders; the mean rank relative to its size)."""
import subprocess

import numpy as np
import pytest

from helpers import movielens_protocol
from sbr_rs_amd import build as hip_build
from test_recommend_cpp import movielens_csv  # noqa: F401  (the fixture in the reference's CSV layout)


@pytest.mark.gpu
@pytest.mark.parametrize("holdout", [1, 5])
def test_cpp_ranking_metrics_match_python(movielens_csv, tmp_path, holdout):  # noqa: F811
    import sbr_rs_amd as sbr

    hip_build.build(verbose=False)
    binary = hip_build.build_ranking_tests(verbose=False)
    out = tmp_path / "ranking.bin"
    p = subprocess.run([binary, movielens_csv, str(holdout), str(out)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    model = (sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).learning_rate(0.16).l2_penalty(0.0004)
             .loss(sbr.Loss.WARP).num_epochs(2).batch_sequences(8).rng(rng).build())
    model.fit(train)
    ks = (10, 100)
    users, hists, targets = sbr.evaluation.holdout_split(test, holdout)
    ranks = np.concatenate(sbr.evaluation.rank_targets(model, hists, targets))
    m = sbr.evaluation.ranking_metrics(model, test, ks=ks, holdout=holdout)
    raw = out.read_bytes()
    nr, nm = np.frombuffer(raw[:16], dtype=np.uint64)
    n = m["num_users_ranked"]
    assert n == len(users) > 100 and nm == 3 + 4 * len(ks) and nr == ranks.size
    assert len(raw) == 16 + 8 * int(nm) + 8 * len(ks) * n + 4 * int(nr)
    got = np.frombuffer(raw[16: 16 + 8 * int(nm)], dtype=np.float64)
    got_ndcg = np.frombuffer(raw[16 + 8 * int(nm): 16 + 8 * int(nm) + 8 * len(ks) * n], dtype=np.float64).reshape(n, len(ks))
    got_ranks = np.frombuffer(raw[len(raw) - 4 * int(nr):], dtype=np.uint32)
    assert np.array_equal(got_ranks, ranks)
    want = [float(n)]
    for k in ks:
        want += [m["precision"][k], m["recall"][k], m["hit_rate"][k], m["ndcg"][k]]
    want += [m["mrr"], m["mean_rank"]]
    assert got == pytest.approx(np.array(want), rel=1e-12, abs=1e-12)
    for j, k in enumerate(ks):
        assert got_ndcg[:, j] == pytest.approx(m["per_user"]["ndcg"][k], rel=1e-12, abs=1e-12)
    assert 0.0 < m["recall"][10] <= m["recall"][100] <= 1.0 and 0.0 < m["ndcg"][10] <= 1.0
