"""GPU: the C++ host layer's recommend with `among` and score_candidates (include/sbr.hpp, tests/cpp/candidates_tests.cpp) on a
MovieLens-trained LSTM give the items and score bits of the Python calls on the same model."""
import os
import subprocess

import numpy as np
import pytest

from helpers import load_movielens, movielens_protocol
from sbr_rs_amd import build as hip_build


@pytest.fixture(scope="module")
def movielens_csv(tmp_path_factory):
    """The fixture in the reference's CSV layout (datasets.rs:57-60)."""
    users, items, ts = load_movielens().arrays()
    path = tmp_path_factory.mktemp("ml") / "data.csv"
    with open(path, "w") as f:
        f.write("user_id,item_id,rating,timestamp\n")
        for u, i, t in zip(users, items, ts):
            f.write(f"{int(u)},{int(i)},1,{int(t)}\n")
    return str(path)


def test_cpp_program_builds_without_a_device():
    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_candidates_tests(verbose=False))


@pytest.mark.gpu
def test_cpp_candidates_match_python(movielens_csv, tmp_path):
    import sbr_rs_amd as sbr

    hip_build.build(verbose=False)
    binary = hip_build.build_candidates_tests(verbose=False)
    k = 20
    out = tmp_path / "cand.bin"
    p = subprocess.run([binary, movielens_csv, str(k), str(out)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    model = (sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).learning_rate(0.16).l2_penalty(0.0004)
             .loss(sbr.Loss.WARP).num_epochs(1).batch_sequences(64).rng(rng).build())
    model.fit(train)
    nu = len(train.user_pointers) - 1
    among = np.arange(0, data.num_items(), 7, dtype=np.uint32)  # the program's item set
    items, scores = model.recommend(train, k, among=among)
    cands = [np.arange(100, dtype=np.uint32)] * 50 + [np.zeros(0, np.uint32)] * (nu - 50)  # ... and its candidates
    cand_scores = np.concatenate(model.score_candidates(train, cands))
    raw = np.fromfile(out, dtype=np.uint32)
    n = items.size
    assert raw.size == 2 * n + 5000
    assert np.array_equal(raw[:n].reshape(items.shape), items)
    assert np.array_equal(raw[n: 2 * n].reshape(items.shape), scores.view(np.uint32))
    assert np.array_equal(raw[2 * n:], cand_scores.view(np.uint32))
    assert (items[:, 0] != 0xFFFFFFFF).all() and np.all(items[items != 0xFFFFFFFF] % 7 == 0)
