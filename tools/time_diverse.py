"""Times sbr_recommend_diverse_reps (topk_gemm / topk_merge at k = pool, then diverse_select_kernel) at catalogue scale: U
representations against 1M items, dim 128, untrained model, pool = 256, cosine, k = 10 and 100, trade_off 0.3 and 1 — the latter
checked here bit for bit against recommend_reps(k) — beside recommend_reps(k = 256), which is the pool scan alone.

    python tools/time_diverse.py [users] [--once] [--scan-only] [--out profiles/diverse_8192x1M_d128]     (writes .json and .md)

One process.  A warm-up call of each, then REPS alternating repetitions (--once: one, for a kernel trace); the figure of a call is
the median of its kernel times (the engine's device events around the launches of the SBR_K_RANK family: for recommend_diverse the
selection is inside).  select = diverse - pool scan (medians) is derived; the select kernel alone comes from a kernel trace of a
--once run.  Bar: the select kernel takes less time than the pool scan it follows, at both k.  --scan-only times recommend_reps(k =
256) alone: it also runs on a commit that lacks the diverse calls, for the comparison with the parent.
The host route the call replaces — recommend_reps(k = 256) to the host, get_param_rows of the pool's rows, a numpy loop over users —
is timed on 256 users and scaled to U."""
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

out_base = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
args = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_base]
U, I, D, POOL = int(args[0]) if args else 8192, 1_000_000, 128, 256
REPS = 1 if "--once" in sys.argv else 5
SCAN_ONLY = "--scan-only" in sys.argv
KS = (10, 100)

m = Model(hparams(I, 64, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
q = np.random.RandomState(9).randint(0, I, U).astype(np.uint32)
reps = m.get_param_rows(Param.ITEM_EMBEDDING, q)  # representations on the scale of the item rows

calls = {f"recommend_reps_k{POOL}": (lambda: m.recommend_reps(reps, POOL))}
if not SCAN_ONLY:
    for k in KS:
        calls[f"diverse_k{k}_t0.3"] = (lambda k=k: m.recommend_diverse_reps(reps, k, POOL, 0.3))
        calls[f"diverse_k{k}_t1"] = (lambda k=k: m.recommend_diverse_reps(reps, k, POOL, 1.0))
    for k in KS:  # the claim that ties the selection to the scan: trade_off 1 is recommend_reps(k)
        a, b = m.recommend_reps(reps, k), calls[f"diverse_k{k}_t1"]()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
for fn in calls.values():  # warm-up: arena growth, first launches, the LDS grant
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

res = {"users": U, "items": I, "dim": D, "pool": POOL, "reps": REPS, "calls": {}, "bar": {}}
for name in calls:
    res["calls"][name] = {"kernels_ms_median": float(np.median(kern[name])), "kernels_ms_all": kern[name],
                          "wall_ms_median": float(np.median(wall[name]))}
scan = res["calls"][f"recommend_reps_k{POOL}"]["kernels_ms_median"]
lines = [f"# recommend_diverse at {U} users x {I} items, d = {D}, pool = {POOL}, cosine", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} alternating repetitions in one process after a",
         f"warm-up call.  recommend_reps(k = {POOL}) is the pool scan alone; diverse = that scan + diverse_select_kernel in one launch",
         "sequence; trade_off 1 returns recommend_reps(k)'s items and score bits (asserted).", "",
         "| call | kernels ms | wall ms | all repetitions (kernels ms) |", "|---|---|---|---|"]
for name, r in res["calls"].items():
    lines.append(f"| {name} | {r['kernels_ms_median']:.2f} | {r['wall_ms_median']:.1f} | {', '.join(f'{x:.2f}' for x in r['kernels_ms_all'])} |")
lines.append("")
if not SCAN_ONLY:
    gather_bytes = float(U) * POOL * D * 4
    for k in KS:
        for t in ("0.3", "1"):
            sel = res["calls"][f"diverse_k{k}_t{t}"]["kernels_ms_median"] - scan
            res["bar"][f"k{k}_t{t}"] = {"select_ms_by_difference": sel, "met": bool(sel < scan)}
            lines.append(f"k = {k}, trade_off {t}: diverse - pool scan = {sel:.2f} ms ({'below' if sel < scan else 'NOT below'} the scan's {scan:.2f} ms); "
                         f"the gather's {gather_bytes / 2**30:.2f} GiB in that time = {gather_bytes / max(sel, 1e-9) / 1e6:.0f} GB/s (a lower bound: the "
                         "rounds are in it).")
    lines.append("")
    # the host route on 256 users, scaled
    nu = min(256, U)
    t0 = time.perf_counter()
    pi, ps = m.recommend_reps(reps[:nu], POOL)
    rows = m.get_param_rows(Param.ITEM_EMBEDDING, pi.ravel()).reshape(nu, POOL, D)
    fetch = time.perf_counter() - t0
    lam, mu = np.float32(0.3), np.float32(1.0) - np.float32(0.3)
    for k in KS:
        t1 = time.perf_counter()
        for u in range(nu):
            X = rows[u]
            n2 = np.einsum("ij,ij->i", X, X)
            Xh = X * np.where(n2 > 0, 1.0 / np.sqrt(np.where(n2 > 0, n2, 1.0)), 0.0).astype(np.float32)[:, None]
            free = np.ones(POOL, bool)
            free[0] = False
            a, mx = 0, np.full(POOL, -np.inf, np.float32)
            for _ in range(1, k):
                mx = np.maximum(mx, Xh @ Xh[a])
                v = np.where(free, lam * ps[u] - mu * mx, -np.inf)
                a = int(np.argmax(v))
                free[a] = False
        loop = time.perf_counter() - t1
        res["calls"][f"host_route_k{k}"] = {"wall_ms_scaled": (fetch + loop) * 1e3 * U / nu, "users_timed": nu}
        lines.append(f"Host route at k = {k} (recommend_reps(k = {POOL}) + get_param_rows + numpy, {nu} users timed, x {U / nu:.0f}): "
                     f"{(fetch + loop) * 1e3 * U / nu:.0f} ms of wall time against {res['calls'][f'diverse_k{k}_t0.3']['wall_ms_median']:.0f} ms.")
    lines.append("")
print("\n".join(lines), flush=True)
if out_base:
    with open(out_base + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(out_base + ".md", "w") as f:
        f.write("\n".join(lines))
