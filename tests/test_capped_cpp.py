"""GPU: the C++ host layer's recommend_capped (include/sbr.hpp, tests/cpp/capped_tests.cpp) on a MovieLens-trained LSTM gives the
items, score bits and flags of the Python calls on the same model: one case the pool settles, one that needs the completion."""
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
def test_cpp_recommend_capped_matches_python(movielens_csv, tmp_path):
    import sbr_rs_amd as sbr

    binary = hip_build.build_capped_tests(verbose=False)
    k = 20
    out = tmp_path / "cap.bin"
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
    ni = data.num_items()
    ga = (np.arange(ni) % 400).astype(np.uint32)
    gb = np.where(np.arange(ni) % 10 != 0, 0, np.arange(ni)).astype(np.uint32)
    model.set_item_groups(ga)
    rows = [model.recommend_capped(test, 10, cap=2, pool=256, exact=False)]
    model.set_item_groups(gb)
    rows += [model.recommend_capped(test, k, cap=1, pool=32, exact=False),
             model.recommend_capped(test, k, cap=1, pool=32),
             store.recommend_capped(slots, k, cap=1, pool=32, exclude=hists)]
    assert rows[0][2].all()                        # the pool settles every row: no completion
    assert not rows[1][2].all() and rows[2][2].all()  # the pool leaves rows short: they are finished through recommend_top
    raw = np.fromfile(out, dtype=np.uint8)
    at = 0
    for r, (items, scores, complete) in enumerate(rows):
        n = items.size
        assert np.array_equal(raw[at: at + 4 * n].view(np.uint32).reshape(items.shape), items), r
        assert np.array_equal(raw[at + 4 * n: at + 8 * n].view(np.uint32).reshape(items.shape), scores.view(np.uint32)), r
        assert np.array_equal(raw[at + 8 * n: at + 8 * n + len(complete)].astype(bool), complete), r
        at += 8 * n + len(complete)
    assert at == raw.size == os.path.getsize(out)
    assert (rows[2][0] != 0xFFFFFFFF).all()  # 1 + 168 groups and more hold eligible items: every finished row is full
    big = (gb[rows[2][0]] == 0).sum(axis=1)
    assert big.max() <= 1 and big.min() >= 0
