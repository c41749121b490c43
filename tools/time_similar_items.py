"""Times sbr_similar_items (item_rnorm / similar_query / topk_gemm<ScaleMul> / topk_merge kernels) at catalogue scale: Q uniformly
drawn query items against 1M items, dim 128, untrained model with a zero bias, k = 10 and 100, beside recommend_reps on the same
rows E[q] — the same scan with the BiasAdd epilogue, which on a zero bias produces the scores of the dot metric with the query
included (checked here bit for bit), so the epilogue does identical work.

    python tools/time_similar_items.py [queries] [--once] [--out profiles/similar_items_8192x1M_d128]     (writes .json and .md)

One process.  A warm-up call of each, then REPS alternating repetitions (--once: one, for a profiler run); the figure of a call is
the median of its kernel times (the engine's device events around the launches of the SBR_K_RANK family: for similar_items the
pre-pass over the catalogue and the query gather are inside).  Bar: the dot metric with the query included takes at most 1.05 x
recommend_reps' kernel time at each k (3 % run-to-run noise plus the pre-pass and the gather).  The cosine figures are recorded,
not barred."""
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
from helpers import hparams  # noqa: E402
from sbr_rs_amd._abi import ModelKind, Param  # noqa: E402
from sbr_rs_amd.engine import Model  # noqa: E402

PEAK_TF = 157.3  # f32 MFMA peak of the MI355X
BAR = 1.05
out_base = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
args = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_base]
Q, I, D = int(args[0]) if args else 8192, 1_000_000, 128
REPS = 1 if "--once" in sys.argv else 5
KS = (10, 100)

m = Model(hparams(I, 64, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
m.set_param(Param.ITEM_BIAS, np.zeros(I, np.float32))
q = np.random.RandomState(9).randint(0, I, Q).astype(np.uint32)
rows = m.get_param_rows(Param.ITEM_EMBEDDING, q)

calls = {}
for k in KS:
    calls[f"recommend_reps_k{k}"] = (lambda k=k: m.recommend_reps(rows, k))
    calls[f"similar_dot_self_k{k}"] = (lambda k=k: m.similar_items(q, k, metric="dot", include_self=True))
    calls[f"similar_cosine_k{k}"] = (lambda k=k: m.similar_items(q, k))

for k in KS:  # warm-up (arena growth, first launches) and the claim the bar rests on
    a, b = calls[f"recommend_reps_k{k}"](), calls[f"similar_dot_self_k{k}"]()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    calls[f"similar_cosine_k{k}"]()
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

flops = 2.0 * Q * I * D
res = {"queries": Q, "items": I, "dim": D, "reps": REPS, "peak_tflops_f32_mfma": PEAK_TF, "calls": {}, "bar": {}}
for name in calls:
    k_ms, w_ms = float(np.median(kern[name])), float(np.median(wall[name]))
    res["calls"][name] = {"kernels_ms_median": k_ms, "kernels_ms_all": kern[name], "wall_ms_median": w_ms,
                          "tflops": flops / (k_ms * 1e-3) / 1e12, "peak_share": flops / (k_ms * 1e-3) / 1e12 / PEAK_TF}
lines = [f"# similar_items at {Q} queries x {I} items, d = {D}", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} alternating repetitions in one process",
         f"after a warm-up call; flop = 2 Q I d = {flops:.3e}; peak = {PEAK_TF} TFLOP/s (f32 MFMA).  recommend_reps scans the rows",
         "E[q] on a zero bias; similar_dot_self returns the same items and score bits (asserted).", "",
         "| call | kernels ms | TFLOP/s | of peak | wall ms | all repetitions (kernels ms) |", "|---|---|---|---|---|---|"]
for name, r in res["calls"].items():
    lines.append(f"| {name} | {r['kernels_ms_median']:.2f} | {r['tflops']:.1f} | {100 * r['peak_share']:.0f} % | "
                 f"{r['wall_ms_median']:.1f} | {', '.join(f'{x:.2f}' for x in r['kernels_ms_all'])} |")
lines.append("")
for k in KS:
    base = res["calls"][f"recommend_reps_k{k}"]["kernels_ms_median"]
    dot = res["calls"][f"similar_dot_self_k{k}"]["kernels_ms_median"]
    res["bar"][f"k{k}"] = {"ratio": dot / base, "met": bool(dot <= BAR * base)}
    lines.append(f"Bar at k = {k}: similar_dot_self {dot:.2f} ms / recommend_reps {base:.2f} ms = {dot / base:.3f} "
                 f"({'met' if dot <= BAR * base else 'MISSED'}: at most {BAR}).")
lines.append("")
print("\n".join(lines), flush=True)
if out_base:
    with open(out_base + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(out_base + ".md", "w") as f:
        f.write("\n".join(lines))
