"""GPU: the C++ host layer's tag filter (include/sbr.hpp: set_item_tags and the *_filtered calls, tests/cpp/filtered_tests.cpp) gives
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
def test_cpp_filtered_calls_match_python(movielens_csv, tmp_path):
    import sbr_rs_amd as sbr

    binary = hip_build.build_filtered_tests(verbose=False)
    k, pool = 20, 64
    out = tmp_path / "filtered.bin"
    p = subprocess.run([binary, movielens_csv, str(k), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    model = sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).rng(rng).build()
    items = data.num_items()
    tags = ((np.arange(items, dtype=np.uint64) * 2654435761) & 0x8000FFFF).astype(np.uint32)
    assert model.set_item_tags(tags) is model and np.array_equal(model.item_tags(), tags)
    up, ids = test.user_pointers, test.item_ids
    hists = [ids[int(up[u]): int(up[u + 1])] for u in range(len(up) - 1)]
    u = np.arange(len(hists))
    any_of = (1 << (u % 5)).astype(np.uint32)
    none_of = np.where(u % 3 == 0, 0x80000000, 0).astype(np.uint32)
    store = model.sessions(len(hists))
    slots = np.arange(len(hists), dtype=np.uint32)
    store.append(slots, hists)
    queries = np.arange(50, dtype=np.uint32)
    rows = [model.recommend(test, k, any_of=any_of, none_of=none_of),
            model.recommend_diverse(test, k, pool, trade_off=0.7, metric="dot", exclude_history=False, any_of=0x00F0),
            model.similar_items(queries, k, any_of=tags[queries]),
            store.recommend(slots, k, exclude=hists, any_of=any_of, none_of=none_of)]
    raw = np.fromfile(out, dtype=np.uint32)
    assert raw.size == 2 * sum(r[0].size for r in rows) and os.path.getsize(out) == 4 * raw.size
    at = 0
    for items_, scores in rows:
        n = items_.size
        assert np.array_equal(raw[at: at + n].reshape(items_.shape), items_)
        assert np.array_equal(raw[at + n: at + 2 * n].reshape(items_.shape), scores.view(np.uint32))
        at += 2 * n
    assert np.any(rows[0][0] != model.recommend(test, k)[0])  # the filter did something
