"""GPU: the C++ host layer's sequence_ranks / sequence_metrics (include/sbr.hpp, tests/cpp/sequence_ranks_tests.cpp) on a
MovieLens-trained LSTM give the integers of the Python call on the same model exactly and its metrics to 1e-12 relative (both
are float64 sums over the same integers; only the order of summation may differ)."""
import subprocess

import numpy as np
import pytest

from helpers import movielens_protocol
from sbr_rs_amd import build as hip_build
from test_recommend_cpp import movielens_csv  # noqa: F401  (the fixture in the reference's CSV layout)


def _flat(m, ks):
    return [m["mrr"], m["mean_rank"]] + [m["hit_rate"][k] for k in ks] + [m["ndcg"][k] for k in ks]


@pytest.mark.gpu
@pytest.mark.parametrize("last", [0, 5])
def test_cpp_sequence_metrics_match_python(movielens_csv, tmp_path, last):  # noqa: F811
    import sbr_rs_amd as sbr

    hip_build.build(verbose=False)
    binary = hip_build.build_sequence_ranks_tests(verbose=False)
    out = tmp_path / "sequence.bin"
    p = subprocess.run([binary, movielens_csv, str(last), str(out)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    T = 32
    model = (sbr.lstm.Hyperparameters.new(data.num_items(), T).embedding_dim(32).learning_rate(0.16).l2_penalty(0.0004)
             .loss(sbr.Loss.WARP).num_epochs(2).batch_sequences(8).rng(rng).build())
    model.fit(train)
    ks = (10, 100)
    rows = model.sequence_ranks(test, last=last or None)
    m = sbr.evaluation.sequence_metrics(model, test, ks=ks, last=last or None)
    ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.uint64)
    ranks = np.concatenate(rows)
    raw = out.read_bytes()
    n_ptr, nr, nm = (int(x) for x in np.frombuffer(raw[:24], dtype=np.uint64))
    per = 3 + 2 * len(ks)
    assert n_ptr == ptr.size and nr == ranks.size > 100 and nm == per * (2 + T + 1)
    assert len(raw) == 24 + 8 * n_ptr + 8 * nm + 4 * nr
    got_ptr = np.frombuffer(raw[24: 24 + 8 * n_ptr], dtype=np.uint64)
    got = np.frombuffer(raw[24 + 8 * n_ptr: 24 + 8 * n_ptr + 8 * nm], dtype=np.float64).reshape(2 + T + 1, per)
    got_ranks = np.frombuffer(raw[len(raw) - 4 * nr:], dtype=np.uint32)
    assert np.array_equal(got_ptr, ptr) and np.array_equal(got_ranks, ranks)
    assert m["num_positions"] == nr
    assert got[0, 0] == nr and got[1, 0] == m["num_users_ranked"]
    assert got[0, 1:] == pytest.approx(np.array(_flat(m, ks)), rel=1e-12, abs=0)
    assert got[1, 1:] == pytest.approx(np.array(_flat(m["macro"], ks)), rel=1e-12, abs=0)
    by = m["by_history_length"]
    assert np.array_equal(got[2:, 0], by["count"].astype(np.float64)) and by["count"].sum() == nr
    want = np.stack([by["mrr"], by["mean_rank"]] + [by["hit_rate"][k] for k in ks] + [by["ndcg"][k] for k in ks], axis=1)
    assert got[2:, 1:] == pytest.approx(want, rel=1e-12, abs=0, nan_ok=True)
    assert 0.0 < m["hit_rate"][10] <= m["hit_rate"][100] <= 1.0 and 0.0 < m["mrr"] <= 1.0
