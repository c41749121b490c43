"""Times sbr_recommend (topk_gemm_kernel + topk_merge_kernel) at catalogue scale, U users x 1M items, dim 128, against
mrr_score on the same users and the plain PyTorch pipeline (torch.addmm + torch.topk, chunked) on the same representations.

    python tools/time_recommend.py [users] [--out profiles/recommend_8192x1M_d128.json]

Kernel times are the engine's device events around the launches of the SBR_K_RANK family (the rank kernels of mrr_score, the
top-k kernels of recommend)."""
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
from sbr_rs_amd._abi import ModelKind, Param  # noqa: E402
from sbr_rs_amd.engine import Model  # noqa: E402

PEAK_TF = 157.3  # f32 MFMA peak of the MI355X
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
U, I, D = int(args[0]) if args else 8192, 1_000_000, 128
REPS = 3


def timed(fn, m):
    fn()  # warm-up (arena growth, first launches)
    m.timing_enable(True)
    m.timing_read()
    t0 = time.perf_counter()
    for _ in range(REPS):
        r = fn()
    wall = (time.perf_counter() - t0) / REPS * 1e3
    kern = m.timing_read()["RANK"][0] / REPS
    m.timing_enable(False)
    return r, wall, kern


m = Model(hparams(I, 64, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
ptr, it = synthetic_interactions(U, I, 40, seed=5, min_len=2)
flops = 2.0 * U * I * D
res = {"users": U, "items": I, "dim": D, "peak_tflops_f32_mfma": PEAK_TF, "k": {}}

(_, ranks), mrr_wall, mrr_kern = timed(lambda: m.mrr_score(ptr, it), m)
res["mrr_score"] = {"users_ranked": int(len(ranks)), "wall_ms": mrr_wall, "rank_kernels_ms": mrr_kern,
                    "tflops": 2.0 * len(ranks) * I * D / (mrr_kern * 1e-3) / 1e12}
print(f"mrr_score: {len(ranks)} users: wall {mrr_wall:.1f} ms, rank kernels {mrr_kern:.2f} ms "
      f"({res['mrr_score']['tflops']:.1f} TFLOP/s)", flush=True)

rs = np.random.RandomState(1)
reps = (rs.randn(U, D) * 0.3).astype(np.float32)
E = torch.from_numpy(m.get_param(Param.ITEM_EMBEDDING).reshape(I, -1)[:, :D].copy()).cuda()
b = torch.from_numpy(m.get_param(Param.ITEM_BIAS).copy()).cuda()
H = torch.from_numpy(reps).cuda()
torch.backends.cuda.matmul.allow_tf32 = False


def torch_pipeline(k, chunk=1024):
    outs = []
    for c in range(0, U, chunk):
        S = torch.addmm(b, H[c: c + chunk], E.t())
        outs.append(torch.topk(S, k, dim=1))
    torch.cuda.synchronize()
    return outs


for k in (10, 100, 1024):
    (items, scores), wall, kern = timed(lambda: m.recommend(ptr, it, k), m)
    (ri, rsc), rwall, rkern = timed(lambda: m.recommend_reps(reps, k), m)
    torch_pipeline(k)
    t0 = time.perf_counter()
    for _ in range(REPS):
        tv = torch_pipeline(k)
    twall = (time.perf_counter() - t0) / REPS * 1e3
    tvals = torch.cat([v.values for v in tv]).cpu().numpy()
    # values only (torch.topk's order among ties is not specified); not expected to hold: hipBLAS's f32 GEMM does not sum in
    # predict's k-ascending chain, so its scores differ from the engine's in the last bits
    agree = bool(np.array_equal(tvals, rsc))
    row = {"recommend_wall_ms": wall, "recommend_kernels_ms": kern, "recommend_tflops": flops / (kern * 1e-3) / 1e12,
           "recommend_peak_share": flops / (kern * 1e-3) / 1e12 / PEAK_TF,
           "recommend_reps_wall_ms": rwall, "recommend_reps_kernels_ms": rkern,
           "torch_addmm_topk_ms": twall, "torch_values_bitwise_equal": agree,
           "kernels_over_mrr_rank_kernels": kern / mrr_kern}
    res["k"][str(k)] = row
    print(f"k={k}: recommend wall {wall:.1f} ms, kernels {kern:.2f} ms = {row['recommend_tflops']:.1f} TFLOP/s "
          f"({100 * row['recommend_peak_share']:.0f} % of peak), {row['kernels_over_mrr_rank_kernels']:.2f}x mrr's rank kernels; "
          f"recommend_reps wall {rwall:.1f} ms kernels {rkern:.2f} ms; torch addmm+topk {twall:.1f} ms (values bitwise equal to the engine's: {agree})",
          flush=True)

if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
