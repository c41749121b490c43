"""GPU: the C++ host layer's sampling calls (include/sbr.hpp: recommend_sampled, recommend_sampled_reps, Sessions::recommend_sampled;
tests/cpp/sampled_tests.cpp) give the items, score bits and key bits of the Python calls on the same model."""
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
def test_cpp_sampled_calls_match_python(movielens_csv, tmp_path):
    import sbr_rs_amd as sbr

    binary = hip_build.build_sampled_tests(verbose=False)
    k = 20
    out = tmp_path / "sampled.bin"
    p = subprocess.run([binary, movielens_csv, str(k), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    model = sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).rng(rng).build()
    items = data.num_items()
    model.set_item_tags(((np.arange(items, dtype=np.uint64) * 2654435761) & 0x8000FFFF).astype(np.uint32))
    up, ids = test.user_pointers, test.item_ids
    hists = [ids[int(up[u]): int(up[u + 1])] for u in range(len(up) - 1)]
    u = np.arange(len(hists))
    store = model.sessions(len(hists), remember=8)
    slots = np.arange(len(hists), dtype=np.uint32)
    store.append(slots, hists)
    streams = (1000003 * u.astype(np.uint64) + (np.uint64(1) << np.uint64(40))).astype(np.uint64)
    rows = [model.recommend_sampled(test, k, temperature=0.75, seed=7, any_of=(1 << (u % 5)).astype(np.uint32)),
            model.recommend_sampled_reps(model.user_representations(test), k, temperature=2.0, seed=8, streams=streams, exclude=hists),
            store.recommend_sampled(slots, k, temperature=1.0, seed=9)]
    raw = np.fromfile(out, dtype=np.uint32)
    assert raw.size == 3 * sum(r[0].size for r in rows) and os.path.getsize(out) == 4 * raw.size
    at = 0
    for items_, scores, keys in rows:
        n = items_.size
        assert np.array_equal(raw[at: at + n].reshape(items_.shape), items_)
        assert np.array_equal(raw[at + n: at + 2 * n].reshape(items_.shape), scores.view(np.uint32))
        assert np.array_equal(raw[at + 2 * n: at + 3 * n].reshape(items_.shape), keys.view(np.uint32))
        at += 3 * n
    assert np.any(rows[0][0] != model.recommend(test, k, any_of=(1 << (u % 5)).astype(np.uint32))[0])  # the noise did something
