"""GPU: the C++ host layer's partition calls (include/sbr.hpp: log_partition, log_partition_reps, Sessions::log_partition and
models::Partition; tests/cpp/partition_tests.cpp) give the shift bits and masses of the Python calls on the same model, and the
same slate probabilities for the same draws."""
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
def test_cpp_partition_calls_match_python(movielens_csv, tmp_path):
    import sbr_rs_amd as sbr

    binary = hip_build.build_partition_tests(verbose=False)
    k = 20
    out = tmp_path / "partition.bin"
    p = subprocess.run([binary, movielens_csv, str(k), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    data, train, test, rng = movielens_protocol()
    model = sbr.lstm.Hyperparameters.new(data.num_items(), 32).embedding_dim(32).rng(rng).build()
    items = data.num_items()
    model.set_item_tags(((np.arange(items, dtype=np.uint64) * 2654435761) & 0x8000FFFF).astype(np.uint32))
    up, ids = test.user_pointers, test.item_ids
    hists = [ids[int(up[u]): int(up[u + 1])] for u in range(len(up) - 1)]
    n = len(hists)
    u = np.arange(n)
    store = model.sessions(n, remember=8)
    slots = np.arange(n, dtype=np.uint32)
    store.append(slots, hists)
    any_of = (1 << (u % 5)).astype(np.uint32)
    reps = model.user_representations(test)
    rows = [(model.log_partition(test, 0.75, any_of=any_of), model.recommend_sampled(test, k, temperature=0.75, seed=7, any_of=any_of)),
            (model.log_partition_reps(reps, 2.0, exclude=hists), model.recommend_sampled_reps(reps, k, temperature=2.0, seed=8, exclude=hists)),
            (store.log_partition(slots, 1.0), store.recommend_sampled(slots, k, temperature=1.0, seed=9))]
    raw = np.fromfile(out, dtype=np.uint8)
    per = 4 * n + 8 * n + 8 * n * k
    assert raw.size == 3 * per == os.path.getsize(out)
    for j, (part, draws) in enumerate(rows):
        blob = raw[j * per: (j + 1) * per]
        assert np.array_equal(blob[: 4 * n].view(np.uint32), part.shift.view(np.uint32))
        assert np.array_equal(blob[4 * n: 12 * n].view(np.uint64), part.mass)
        slate = blob[12 * n:].view(np.float64).reshape(n, k)
        want = part.slate_log_prob(draws[1])
        assert np.array_equal(np.isnan(slate), np.isnan(want)) and np.nanmax(np.abs(slate - want)) <= 1e-12
        assert not np.isnan(want[:, 0]).any() or j == 0  # a filtered row may be short; the others draw k real items
    from sbr_rs_amd.engine import softmax_frac_bits

    assert rows[0][0].frac_bits == softmax_frac_bits(items)
