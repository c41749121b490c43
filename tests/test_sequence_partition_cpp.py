"""GPU: the C++ host layer's sequence_partition / sequence_log_probs / sequence_log_likelihood (include/sbr.hpp,
tests/cpp/sequence_partition_tests.cpp) on a MovieLens-trained LSTM against the Python call on the same model: equal shift bits,
masses, score bits and mask flags, and log-probabilities equal to 1 ulp of float64 (both are log(w) - log(mass) of the same
integers; the two C libraries' log may differ in the last place)."""
import subprocess

import numpy as np
import pytest

from helpers import movielens_protocol
from sbr_rs_amd import build as hip_build
from test_recommend_cpp import movielens_csv  # noqa: F401  (the fixture in the reference's CSV layout)

TEMPERATURE = 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("last", [0, 5])
def test_cpp_sequence_partition_matches_python(movielens_csv, tmp_path, last):  # noqa: F811
    import sbr_rs_amd as sbr

    hip_build.build(verbose=False)
    binary = hip_build.build_sequence_partition_tests(verbose=False)
    out = tmp_path / "sequence_partition.bin"
    p = subprocess.run([binary, movielens_csv, str(last), str(out)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    T = 32
    model = (sbr.lstm.Hyperparameters.new(data.num_items(), T).embedding_dim(32).learning_rate(0.16).l2_penalty(0.0004)
             .loss(sbr.Loss.WARP).num_epochs(2).batch_sequences(8).rng(rng).build())
    model.fit(train)
    ptr, part, scores, masked = model.params.sequence_partition(test.user_pointers, test.item_ids, temperature=TEMPERATURE,
                                                                last=last or None)
    rows = model.sequence_log_probs(test, temperature=TEMPERATURE, last=last or None)
    ll = sbr.evaluation.sequence_log_likelihood(model, test, temperature=TEMPERATURE, last=last or None)
    lp = np.concatenate(rows)
    n = scores.size
    raw = out.read_bytes()
    n_ptr, nn = (int(x) for x in np.frombuffer(raw[:16], dtype=np.uint64))
    assert n_ptr == ptr.size and nn == n > 100
    assert len(raw) == 16 + 8 * n_ptr + 56 + 8 * n + 8 * n + 4 * n + 4 * n + n
    at = 16
    got_ptr = np.frombuffer(raw[at: at + 8 * n_ptr], dtype=np.uint64)
    at += 8 * n_ptr
    summary = np.frombuffer(raw[at: at + 56], dtype=np.float64)
    at += 56
    got_mass = np.frombuffer(raw[at: at + 8 * n], dtype=np.uint64)
    at += 8 * n
    got_lp = np.frombuffer(raw[at: at + 8 * n], dtype=np.float64)
    at += 8 * n
    got_shift = np.frombuffer(raw[at: at + 4 * n], dtype=np.uint32)
    at += 4 * n
    got_scores = np.frombuffer(raw[at: at + 4 * n], dtype=np.uint32)
    at += 4 * n
    got_masked = np.frombuffer(raw[at: at + n], dtype=np.uint8)
    assert np.array_equal(got_ptr, ptr)
    assert np.array_equal(got_shift, part.shift.view(np.uint32)) and np.array_equal(got_mass, part.mass)
    assert np.array_equal(got_scores, scores.view(np.uint32)) and np.array_equal(got_masked, masked)
    assert not masked.all()
    inf = np.isneginf(lp)
    assert np.array_equal(np.isneginf(got_lp), inf) and inf[masked.astype(bool)].all()
    assert (np.abs(got_lp[~inf] - lp[~inf]) <= np.spacing(np.abs(lp[~inf]))).all(), "log-probabilities to 1 ulp of f64"
    assert summary[0] == ll["positions"] and summary[1] == ll["masked_positions"] and summary[2] == ll["macro"]["users"]
    assert summary[3] == pytest.approx(ll["mean_log_prob"], rel=1e-12, abs=0)
    # exp(-mean): a relative error e of the mean becomes |mean| e of the perplexity
    assert summary[4] == pytest.approx(ll["perplexity"], rel=1e-12 * (1.0 + abs(ll["mean_log_prob"])), abs=0)
    assert summary[5] == pytest.approx(ll["macro"]["mean_log_prob"], rel=1e-12, abs=0)
    assert summary[6] == pytest.approx(ll["macro"]["perplexity"], rel=1e-12 * (1.0 + abs(ll["macro"]["mean_log_prob"])), abs=0)
    assert ll["positions"] > 100 and ll["mean_log_prob"] < 0.0
