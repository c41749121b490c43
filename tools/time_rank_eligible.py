"""Times rank_targets under a serving policy (the rank_eligible_* kernels: sbr_rank_targets_rows / sbr_item_set_rank_targets) at
catalogue scale — U rows x 1M items, dim 128, untrained model, 10 targets per row — beside the calls it must not slow down and the
only exact route there was before it.

    python tools/time_rank_eligible.py [rows] [--tree DIR] [--out FILE.json] [--route-rows N]

One process measures one library: the tree this file lies in, or with --tree DIR the package of another checkout (the parent
commit, built there), which has no eligible ranks — then only the untouched calls and the old route are timed.  Run it as
alternating processes of parent and change and compare the JSON files.

  untouched   rank_targets_reps, mrr_score, recommend_reps(k = 10), count_above_reps            (both libraries)
  new         rank_targets_reps under tag masks (about 60 % of the items allowed), ItemSet.rank_targets_reps at |S| = 1e5,
              Sessions.rank_targets on a store with memory                                       (the change only)
  old route   score_candidates_reps for each target's score, then one count_above_reps row per target at that score with the
              row's list and masks: exact for targets the policy can show, written against the parent's API.  It scans one row per
              target, so it is timed on the first --route-rows rows (default 1024) and reported per row as well.

A warm-up call of each, then REPS repetitions, calls alternating; a figure is the median of the kernel times (the engine's device
events around the SBR_K_RANK launches).  The new calls are checked against the old route on the rows it ran."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def _arg(flag, default=None):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


TREE = os.path.abspath(_arg("--tree", os.path.join(HERE, "..")))
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.zeros(1, device="cuda")  # PyTorch's HIP runtime first (tests/conftest.py)
from helpers import hparams, synthetic_interactions  # noqa: E402
from sbr_rs_amd._abi import ModelKind  # noqa: E402
from sbr_rs_amd.engine import Model  # noqa: E402

flags = {"--tree", "--out", "--route-rows"}
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags]
U, I, D, T, REPS = int(args[0]) if args else 8192, 1_000_000, 128, 10, 3
ROUTE = min(U, int(_arg("--route-rows", 1024)))

m = Model(hparams(I, 64, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
NEW = hasattr(m, "_L") and hasattr(m._L, "sbr_rank_targets_rows")
rs = np.random.RandomState(9)
ptr, it = synthetic_interactions(U, I, 40, seed=5, min_len=2)
reps = (rs.randn(U, D) * 0.5).astype(np.float32)
tptr = np.arange(U + 1, dtype=np.uint64) * T
tit = rs.randint(0, I, U * T).astype(np.uint32)
excl = [rs.randint(0, I, 20).astype(np.uint32) for _ in range(U)]
tags = (1 << rs.randint(0, 5, I)).astype(np.uint32)
m.set_item_tags(tags)
any_of, none_of = np.full(U, 0x0B, np.uint32), np.full(U, 0x10, np.uint32)  # three of five bits: 60 % of the items, minus none
th = np.zeros(U, np.float32)


def old_route(n):
    """ranks of the first n rows' targets by the route the parent has: exact where the target is not masked"""
    scores = m.score_candidates_reps(reps[:n], tptr[: n + 1], tit[: n * T])
    rows = np.repeat(np.arange(n), T)
    return m.count_above_reps(reps[rows], np.concatenate(scores).astype(np.float32), exclude=[excl[u] for u in rows], any_of=any_of[rows],
                              none_of=none_of[rows]).astype(np.uint32)


calls = {
    "rank_targets_reps": lambda: m.rank_targets_reps(reps, tptr, tit, exclude=excl),
    "mrr_score": lambda: m.mrr_score(ptr, it),
    "recommend_reps_k10": lambda: m.recommend_reps(reps, 10, exclude=excl),
    "count_above_reps": lambda: m.count_above_reps(reps, th, exclude=excl),
    f"old_route_{ROUTE}_rows": lambda: old_route(ROUTE),
}
if NEW:
    S = np.sort(rs.choice(I, 100_000, replace=False)).astype(np.uint32)
    item_set = m.item_set(S)
    store = m.sessions(U, remember=32)
    slots = np.arange(U, dtype=np.uint32)
    store.append(slots, [it[int(ptr[u]): int(ptr[u + 1])][-32:] for u in range(U)])
    calls["rank_targets_reps_filtered"] = lambda: m.rank_targets_reps(reps, tptr, tit, exclude=excl, any_of=any_of, none_of=none_of)
    calls["item_set_100k_rank_targets_reps"] = lambda: item_set.rank_targets_reps(reps, tptr, tit, exclude=excl)
    calls["sessions_rank_targets"] = lambda: store.rank_targets(slots, (tptr, tit), exclude=excl)

for fn in calls.values():  # warm-up (arena growth, first launches)
    fn()
m.timing_enable(True)
kern, wall = {n: [] for n in calls}, {n: [] for n in calls}
for _ in range(REPS):
    for name, fn in calls.items():
        m.timing_read()
        t0 = time.perf_counter()
        fn()
        wall[name].append((time.perf_counter() - t0) * 1e3)
        kern[name].append(m.timing_read()["RANK"][0])
m.timing_enable(False)

res = {"tree": TREE, "has_eligible_ranks": bool(NEW), "rows": U, "items": I, "dim": D, "targets_per_row": T, "reps": REPS,
       "route_rows": ROUTE, "calls": {}}
for name in calls:
    res["calls"][name] = {"kernels_ms_median": float(np.median(kern[name])), "kernels_ms_all": kern[name],
                          "wall_ms_median": float(np.median(wall[name]))}
route = res["calls"][f"old_route_{ROUTE}_rows"]
route["kernels_ms_scaled_to_all_rows"] = route["kernels_ms_median"] * U / ROUTE
if NEW:  # the new call against the old route, where the old route is exact
    got = m.rank_targets_reps(reps[:ROUTE], tptr[: ROUTE + 1], tit[: ROUTE * T], exclude=excl[:ROUTE], any_of=any_of[:ROUTE], none_of=none_of[:ROUTE])
    want = old_route(ROUTE)
    shown = got != I
    res["checked_against_old_route"] = {"targets": int(got.size), "shown": int(shown.sum()), "equal": bool(np.array_equal(got[shown], want[shown]))}
    assert res["checked_against_old_route"]["equal"]
print(json.dumps(res, indent=1), flush=True)
out = _arg("--out")
if out:
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
