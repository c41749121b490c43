"""GPU: the C++ host layer's recommend_diverse (include/sbr.hpp, tests/cpp/diverse_tests.cpp) on a MovieLens-trained LSTM gives
the items and score bits of the Python calls on the same model."""
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
def test_cpp_recommend_diverse_matches_python(movielens_csv, tmp_path):
    import sbr_rs_amd as sbr

    binary = hip_build.build_diverse_tests(verbose=False)
    k, pool = 20, 64
    out = tmp_path / "div.bin"
    p = subprocess.run([binary, movielens_csv, str(k), str(out)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    model = (sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).learning_rate(0.16).l2_penalty(0.0004)
             .loss(sbr.Loss.WARP).num_epochs(1).batch_sequences(64).rng(rng).build())
    model.fit(train)
    up, ids = test.user_pointers, test.item_ids
    hists = [ids[int(up[u]): int(up[u + 1])] for u in range(len(up) - 1)]
    store = model.sessions(len(hists))
    slots = np.arange(len(hists), dtype=np.uint32)
    store.append(slots, hists)
    rows = [model.recommend_diverse(test, k, pool, trade_off=0.3),
            model.recommend_diverse(test, k, pool, trade_off=0.7, metric="dot", exclude_history=False),
            store.recommend_diverse(slots, k, pool, 0.3, exclude=hists)]
    raw = np.fromfile(out, dtype=np.uint32)
    n = rows[0][0].size
    assert raw.size == 6 * n and os.path.getsize(out) == 24 * n
    for r, (items, scores) in enumerate(rows):
        assert np.array_equal(raw[2 * r * n: (2 * r + 1) * n].reshape(items.shape), items)
        assert np.array_equal(raw[(2 * r + 1) * n: (2 * r + 2) * n].reshape(items.shape), scores.view(np.uint32))
    assert (rows[0][0][:, 0] != 0xFFFFFFFF).all()
    plain = model.recommend(test, k)
    assert np.any(rows[0][0] != plain[0])  # the selection did something
