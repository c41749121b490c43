"""GPU: the C++ host layer's budget calls (include/sbr.hpp: recommend_top, recommend_top_reps, audience_top, audience_top_reps,
Sessions::recommend_top / audience_top and models::Above::cuts; tests/cpp/top_tests.cpp) give the pointers, ids, score bits and
cuts of the Python calls on the same model, in both orders."""
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


def _read(raw, at):
    """one dumped Above at byte offset `at` -> (ptr, ids, score bits, cut bits, the offset behind it)"""
    rows, total = (int(x) for x in raw[at: at + 16].view(np.uint64))
    at += 16
    ptr = raw[at: at + 8 * (rows + 1)].view(np.uint64)
    at += 8 * (rows + 1)
    ids = raw[at: at + 4 * total].view(np.uint32)
    at += 4 * total
    bits = raw[at: at + 4 * total].view(np.uint32)
    at += 4 * total
    cuts = raw[at: at + 4 * rows].view(np.uint32)
    return ptr, ids, bits, cuts, at + 4 * rows


@pytest.mark.gpu
def test_cpp_top_calls_match_python(movielens_csv, tmp_path):
    import sbr_rs_amd as sbr

    binary = hip_build.build_top_tests(verbose=False)
    k = 20
    out = tmp_path / "top.bin"
    p = subprocess.run([binary, movielens_csv, str(k), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    model = sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).rng(rng).build()
    items = data.num_items()
    model.set_item_tags(((np.arange(items, dtype=np.uint64) * 2654435761) & 0x8000FFFF).astype(np.uint32))
    up, ids = test.user_pointers, test.item_ids
    hists = [ids[int(up[u]): int(up[u + 1])] for u in range(len(up) - 1)]
    users = len(hists)
    n = 1 + 37 * np.arange(users, dtype=np.uint64)
    queries = np.arange(12, dtype=np.uint32)
    any_of = (1 << (np.arange(users) % 5)).astype(np.uint32)
    reps = model.user_representations(test)
    store = model.sessions(users, remember=8)
    slots = np.arange(users, dtype=np.uint32)
    store.append(slots, hists)
    want = [model.recommend_top(test, n, any_of=any_of), model.recommend_top(test, n, any_of=any_of, order="id"),
            model.recommend_top_reps(reps, n, exclude=hists), model.recommend_top_reps(reps, n, exclude=hists, order="id"),
            model.audience_top(test, queries, 1500), model.audience_top(test, queries, 1500, order="id"),
            model.audience_top_reps(reps, queries, 5 * np.arange(12), order="id"),
            store.recommend_top(slots, n), store.audience_top(queries, 1500)]
    raw = np.fromfile(out, dtype=np.uint8)
    at = 0
    for j, w in enumerate(want):
        ptr, got_ids, bits, cuts, at = _read(raw, at)
        assert np.array_equal(ptr, w.ptr), j
        assert np.array_equal(got_ids, w.ids), j
        assert np.array_equal(bits, w.scores.view(np.uint32)), j
        assert np.array_equal(cuts, w.cuts.view(np.uint32)), j
        assert int(ptr[-1]) > 0
    assert at == raw.size == os.path.getsize(out)
