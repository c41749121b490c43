"""Times sbr_rank_targets (rank_targets_prepare / _gemm / _finish kernels) at catalogue scale, U users x 1M items, dim 128, at
T = 1, 10 and 32 targets per user, against the two routes to metrics at k the engine had before it: mrr_score on the same users
(the floor: one threshold per user) and recommend(k = 100) (a top-k list to intersect on the host).

    python tools/time_rank_targets.py [users] [--out profiles/rank_targets_8192x1M_d128]     (writes .json and .md)

One process; the seeded untrained LSTM and the synthetic histories of tools/time_recommend.py; targets are uniform random items,
so about half of all scores pass the first compare (the hard case).  A warm-up call of each, then REPS alternating repetitions;
the figure of a call is the median of its kernel times (the engine's device events around the launches of the SBR_K_RANK family).
Acceptance: at T = 10 the rank_targets kernels take less than recommend(k = 100)'s and less than 10 x mrr_score's,
each by more than 3 % (the pool's run-to-run noise)."""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

torch.zeros(1, device="cuda")  # PyTorch's HIP runtime first (tests/conftest.py)
from helpers import hparams, synthetic_interactions  # noqa: E402
from sbr_rs_amd._abi import ModelKind  # noqa: E402
from sbr_rs_amd.engine import Model  # noqa: E402

PEAK_TF = 157.3  # f32 MFMA peak of the MI355X
NOISE = 0.03
out_base = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
args = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_base]
U, I, D = int(args[0]) if args else 8192, 1_000_000, 128
REPS = 5
TS = (1, 10, 32)
K = 100

m = Model(hparams(I, 64, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
ptr, it = synthetic_interactions(U, I, 40, seed=5, min_len=2)
ptr64 = ptr.astype(np.int64)
# mrr_score's split of every user: all but the last item are the history
keep = np.ones(it.size, dtype=bool)
keep[ptr64[1:] - 1] = False
hist_items = np.ascontiguousarray(it[keep])
hist_ptr = (ptr64 - np.arange(U + 1)).astype(np.uint64)
rs = np.random.RandomState(9)
targets = {T: (np.arange(U + 1, dtype=np.uint64) * T, rs.randint(0, I, U * T).astype(np.uint32)) for T in TS}

calls = {"mrr_score": lambda: m.mrr_score(ptr, it), f"recommend_k{K}": lambda: m.recommend(hist_ptr, hist_items, K)}
for T in TS:
    calls[f"rank_targets_T{T}"] = (lambda T=T: m.rank_targets(hist_ptr, hist_items, targets[T][0], targets[T][1]))

for fn in calls.values():  # warm-up (arena growth, first launches)
    fn()
m.timing_enable(True)
kern = {name: [] for name in calls}
wall = {name: [] for name in calls}
for _ in range(REPS):
    for name, fn in calls.items():
        m.timing_read()
        t0 = time.perf_counter()
        fn()
        wall[name].append((time.perf_counter() - t0) * 1e3)
        kern[name].append(m.timing_read()["RANK"][0])
m.timing_enable(False)

# one target per user, the last item: the ranks are mrr_score's
_, mrr_ranks = m.mrr_score(ptr, it)
last = np.ascontiguousarray(it[ptr64[1:] - 1])
assert np.array_equal(m.rank_targets(hist_ptr, hist_items, np.arange(U + 1, dtype=np.uint64), last), mrr_ranks)

flops = 2.0 * U * I * D
res = {"users": U, "items": I, "dim": D, "reps": REPS, "peak_tflops_f32_mfma": PEAK_TF, "calls": {}}
for name in calls:
    k_ms, w_ms = float(np.median(kern[name])), float(np.median(wall[name]))
    res["calls"][name] = {"kernels_ms_median": k_ms, "kernels_ms_all": kern[name], "wall_ms_median": w_ms,
                          "tflops": flops / (k_ms * 1e-3) / 1e12, "peak_share": flops / (k_ms * 1e-3) / 1e12 / PEAK_TF}
floor, route = res["calls"]["mrr_score"]["kernels_ms_median"], res["calls"][f"recommend_k{K}"]["kernels_ms_median"]
t10 = res["calls"]["rank_targets_T10"]["kernels_ms_median"]
res["acceptance"] = {"rank_targets_T10_ms": t10, f"recommend_k{K}_ms": route, "mrr_score_ms": floor,
                     f"below_recommend_k{K}_by_more_than_noise": bool(t10 < route * (1 - NOISE)),
                     "below_10x_mrr_score_by_more_than_noise": bool(t10 < 10 * floor * (1 - NOISE))}
lines = [f"# rank_targets at {U} users x {I} items, d = {D}", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} alternating repetitions in one process",
         f"after a warm-up call; flop = 2 U I d = {flops:.3e}; peak = {PEAK_TF} TFLOP/s (f32 MFMA).", "",
         "| call | kernels ms | x mrr_score | TFLOP/s | of peak | wall ms | all repetitions (kernels ms) |", "|---|---|---|---|---|---|---|"]
for name, r in res["calls"].items():
    r["kernels_over_mrr_score"] = r["kernels_ms_median"] / floor
    lines.append(f"| {name} | {r['kernels_ms_median']:.2f} | {r['kernels_over_mrr_score']:.2f} | {r['tflops']:.1f} | "
                 f"{100 * r['peak_share']:.0f} % | {r['wall_ms_median']:.1f} | {', '.join(f'{x:.2f}' for x in r['kernels_ms_all'])} |")
a = res["acceptance"]
lines += ["", f"Acceptance at T = 10: {t10:.2f} ms against recommend(k = {K}) {route:.2f} ms "
              f"({'met' if a[f'below_recommend_k{K}_by_more_than_noise'] else 'MISSED'}: below by more than 3 %) and against "
              f"10 x mrr_score = {10 * floor:.2f} ms ({'met' if a['below_10x_mrr_score_by_more_than_noise'] else 'MISSED'}).",
          "T = 32 is two scan-users per user (16 thresholds each): two passes over the catalogue.", ""]
print("\n".join(lines), flush=True)
if out_base:
    with open(out_base + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(out_base + ".md", "w") as f:
        f.write("\n".join(lines))
