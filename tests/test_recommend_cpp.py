"""GPU: the C++ host layer's recommend (include/sbr.hpp, tests/cpp/recommend_tests.cpp) on a MovieLens-trained LSTM gives
the items and score bits of the Python call on the same model."""
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


@pytest.mark.gpu
def test_cpp_recommend_matches_python(movielens_csv, tmp_path):
    import sbr_rs_amd as sbr

    hip_build.build(verbose=False)
    binary = hip_build.build_recommend_tests(verbose=False)
    k = 20
    out = tmp_path / "rec.bin"
    p = subprocess.run([binary, movielens_csv, str(k), str(out)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    model = (sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).learning_rate(0.16).l2_penalty(0.0004)
             .loss(sbr.Loss.WARP).num_epochs(2).batch_sequences(8).rng(rng).build())
    model.fit(train)
    items, scores = model.recommend(test, k)
    raw = np.fromfile(out, dtype=np.uint32)
    n = items.size
    assert raw.size == 2 * n and os.path.getsize(out) == 8 * n
    assert np.array_equal(raw[:n].reshape(items.shape), items)
    assert np.array_equal(raw[n:].reshape(items.shape), scores.view(np.uint32))
    assert (items[:, 0] != 0xFFFFFFFF).all()
