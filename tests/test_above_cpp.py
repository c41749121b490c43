"""GPU: the C++ host layer's threshold calls (include/sbr.hpp: recommend_above, recommend_above_reps, audience_above,
audience_above_reps, Sessions::recommend_above / audience_above and models::Above; tests/cpp/above_tests.cpp) give the pointers, ids
and score bits of the Python calls on the same model, in both orders."""
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
    """one dumped Above at byte offset `at` -> (ptr, ids, score bits, the offset behind it)"""
    rows, total = (int(x) for x in raw[at: at + 16].view(np.uint64))
    at += 16
    ptr = raw[at: at + 8 * (rows + 1)].view(np.uint64)
    at += 8 * (rows + 1)
    ids = raw[at: at + 4 * total].view(np.uint32)
    at += 4 * total
    bits = raw[at: at + 4 * total].view(np.uint32)
    return ptr, ids, bits, at + 4 * total


@pytest.mark.gpu
def test_cpp_above_calls_match_python(movielens_csv, tmp_path):
    import sbr_rs_amd as sbr

    binary = hip_build.build_above_tests(verbose=False)
    k = 20
    out = tmp_path / "above.bin"
    p = subprocess.run([binary, movielens_csv, str(k), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    model = sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).rng(rng).build()
    items = data.num_items()
    model.set_item_tags(((np.arange(items, dtype=np.uint64) * 2654435761) & 0x8000FFFF).astype(np.uint32))
    up, ids = test.user_pointers, test.item_ids
    hists = [ids[int(up[u]): int(up[u + 1])] for u in range(len(up) - 1)]
    n = len(hists)
    t = model.recommend(test, k)[1][:, k - 1].copy()
    mid = np.sort(t)[n // 2]
    queries = np.arange(12, dtype=np.uint32)
    any_of = (1 << (np.arange(n) % 5)).astype(np.uint32)
    reps = model.user_representations(test)
    store = model.sessions(n, remember=8)
    slots = np.arange(n, dtype=np.uint32)
    store.append(slots, hists)
    want = [model.recommend_above(test, t, any_of=any_of), model.recommend_above(test, t, any_of=any_of, order="id"),
            model.recommend_above_reps(reps, t, exclude=hists), model.recommend_above_reps(reps, t, exclude=hists, order="id"),
            model.audience_above(test, queries, mid), model.audience_above(test, queries, mid, order="id"),
            model.audience_above_reps(reps, queries, t[:12], order="id"),
            store.recommend_above(slots, t), store.audience_above(queries, mid)]
    raw = np.fromfile(out, dtype=np.uint8)
    at = 0
    for j, w in enumerate(want):
        ptr, got_ids, bits, at = _read(raw, at)
        assert np.array_equal(ptr, w.ptr), j
        assert np.array_equal(got_ids, w.ids), j
        assert np.array_equal(bits, w.scores.view(np.uint32)), j
        assert int(ptr[-1]) > 0
    assert at == raw.size == os.path.getsize(out)
