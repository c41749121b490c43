"""Times sbr_sequence_partition (the top-k scan over the shift pool, sequence_shift_kernel, partition_gemm_kernel and
partition_prefix_kernel behind one forward pass per sequence) at catalogue scale: 1M items, dim 128, LSTM, T = 64, U users of 65
items each — 64 positions per user, so U = 8 192 is 64 launches of 8 192 scan rows — in full and with last = 5, masked and
unmasked, beside log_partition_reps over 8 192 rows in the same process, and against the route it replaces: log_partition plus
score_candidates over every explicit prefix as a "user" of its own, timed on PREFIX_USERS users and SCALED to U by the user count
(said so in the output).

    python tools/time_sequence_log_probs.py [users] [--out profiles/sequence_log_probs_8192x1M_d128]     (writes .json and .md)
    python tools/time_sequence_log_probs.py --neighbours [--root DIR]     (one JSON line: the neighbouring calls' kernel ms)
    python tools/time_sequence_log_probs.py --trace     (one masked last = 5 call after a warm-up: for a profiler's kernel trace)

One process; the seeded untrained LSTM of tools/time_sequence_ranks.py.  A warm-up call of each, then REPS alternating
repetitions; kernel time = the engine's device events around the launches of the SBR_K_RANK family (every scan-side kernel of a
launch together) and of SBR_K_RECURRENT_FWD (the forward pass); the split of the scan family by kernel comes from a profiler's
kernel trace of --trace, not from the ledger.  The unresolved rows are counted on the PREFIX_USERS users' prefixes with recommend at
k = 16 without exclusions: a row is unresolved when all 16 lie in its prefix.  --neighbours measures the calls that share kernels
with the new one and nothing else, so it runs unchanged against another checkout (--root: where sbr_rs_amd is imported from), for
the no-regression comparison in alternating processes."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
root_arg = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else None
ROOT = os.path.abspath(root_arg) if root_arg else os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

torch.zeros(1, device="cuda")  # PyTorch's HIP runtime first (tests/conftest.py)
from helpers import hparams  # noqa: E402
from sbr_rs_amd._abi import ModelKind  # noqa: E402
from sbr_rs_amd.engine import Model  # noqa: E402

I, D, T = 1_000_000, 128, 64
REPS = 3
PREFIX_USERS = 32
TEMPERATURE = 1.0
out_base = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in (out_base, root_arg)]
U = int(args[0]) if args else 8192


def timed(m, calls, reps):
    for fn in calls.values():  # warm-up (arena growth, first launches)
        fn()
    m.timing_enable(True)
    out = {name: {"rank_ms": [], "forward_ms": [], "wall_ms": [], "scans": 0} for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            m.timing_read()
            t0 = time.perf_counter()
            fn()
            out[name]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            t = m.timing_read()
            out[name]["rank_ms"].append(t["RANK"][0])
            out[name]["forward_ms"].append(t["RECURRENT_FWD"][0])
            out[name]["scans"] = int(t["RANK"][1])
    m.timing_enable(False)
    for r in out.values():
        for k in ("rank_ms", "forward_ms", "wall_ms"):
            r[k + "_median"] = float(np.median(r[k]))
    return out


m = Model(hparams(I, T, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
rs = np.random.RandomState(5)
n = T + 1
reps8k = (np.random.RandomState(6).randn(8192, D) * 0.1).astype(np.float32)

if "--neighbours" in sys.argv:
    ptr = (np.arange(8192 + 1, dtype=np.uint64) * n)
    it = rs.randint(0, I, 8192 * n).astype(np.uint32)
    res = timed(m, {"log_partition_reps": lambda: m.log_partition_reps(reps8k, TEMPERATURE),
                    "recommend_reps_k1": lambda: m.recommend_reps(reps8k, 1),
                    "recommend_reps_k10": lambda: m.recommend_reps(reps8k, 10),
                    "sequence_ranks_last5": lambda: m.sequence_ranks(ptr, it, last=5)}, REPS)
    print(json.dumps({name: {"rank_ms_median": r["rank_ms_median"], "rank_ms": r["rank_ms"]} for name, r in res.items()}), flush=True)
    sys.exit(0)

ptr = (np.arange(U + 1, dtype=np.uint64) * n)
it = rs.randint(0, I, U * n).astype(np.uint32)
units = U * T

if "--trace" in sys.argv:
    m.sequence_partition(ptr, it, temperature=TEMPERATURE, last=5)
    m.sequence_partition(ptr, it, temperature=TEMPERATURE, last=5)
    sys.exit(0)

# the route it replaces, on the first PREFIX_USERS users: every prefix a history of its own, its next item the one candidate
P = min(PREFIX_USERS, U)
pre_hist = [it[u * n: u * n + p] for u in range(P) for p in range(1, n)]
pre_ptr = np.concatenate([[0], np.cumsum([h.size for h in pre_hist])]).astype(np.uint64)
pre_items = np.ascontiguousarray(np.concatenate(pre_hist))
pre_cp = np.arange(P * T + 1, dtype=np.uint64)
pre_ci = np.ascontiguousarray(np.array([it[u * n + p] for u in range(P) for p in range(1, n)], dtype=np.uint32))


def prefix_route():
    part = m.log_partition(pre_ptr, pre_items, TEMPERATURE)
    return part, np.asarray(m.score_candidates(pre_ptr, pre_items, pre_cp, pre_ci), dtype=np.float32).ravel()


calls = {"sequence_partition": lambda: m.sequence_partition(ptr, it, temperature=TEMPERATURE),
         "sequence_partition_unmasked": lambda: m.sequence_partition(ptr, it, temperature=TEMPERATURE, include_history=True),
         "sequence_partition_last5": lambda: m.sequence_partition(ptr, it, temperature=TEMPERATURE, last=5),
         "sequence_partition_last5_unmasked": lambda: m.sequence_partition(ptr, it, temperature=TEMPERATURE, include_history=True, last=5),
         "log_partition_reps_8192": lambda: m.log_partition_reps(reps8k, TEMPERATURE),
         "recommend_reps_8192_k1": lambda: m.recommend_reps(reps8k, 1),
         "recommend_reps_8192_k16": lambda: m.recommend_reps(reps8k, 16),
         f"prefix_route_{P}_users": prefix_route}
res = timed(m, calls, REPS)

# the same bits by both routes, and last = 5 is the tail of the full call
_p, full, fscores, fmasked = m.sequence_partition(ptr, it, temperature=TEMPERATURE)
part, cand = prefix_route()
assert np.array_equal(full.shift[: P * T].view(np.uint32), part.shift.view(np.uint32)) and np.array_equal(full.mass[: P * T], part.mass)
assert np.array_equal(fscores[: P * T].view(np.uint32), cand.view(np.uint32))
_p5, last5, s5, m5 = m.sequence_partition(ptr, it, temperature=TEMPERATURE, last=5)
assert np.array_equal(full.mass.reshape(U, T)[:, -5:].ravel(), last5.mass) and np.array_equal(fscores.reshape(U, T)[:, -5:].ravel(), s5)
# unresolved rows, counted on the prefix route's rows: the 16 best of the whole catalogue all in the row's prefix
top16 = np.asarray(m.recommend(pre_ptr, pre_items, 16, include_history=True)[0]).reshape(P * T, 16)
unresolved = int(sum(np.isin(top16[r], pre_hist[r]).all() for r in range(P * T)))
lp = full.log_prob(fscores[:, None])[:, 0]

launches = (units + 8191) // 8192
launches5 = (U * 5 + 8191) // 8192
scale = U / P
pre = res[f"prefix_route_{P}_users"]
seq, lpr = res["sequence_partition"], res["log_partition_reps_8192"]
k1, k16 = res["recommend_reps_8192_k1"], res["recommend_reps_8192_k16"]
out = {"users": U, "items": I, "dim": D, "max_sequence_length": T, "temperature": TEMPERATURE, "units": units,
       "launches_of_8192": launches, "reps": REPS, "calls": res, "prefix_route_users": P, "prefix_route_scale": scale,
       "prefix_route_scaled": {k: pre[k + "_median"] * scale for k in ("rank_ms", "forward_ms", "wall_ms")},
       "scan_ms_per_launch": seq["rank_ms_median"] / launches,
       "scan_ms_per_launch_unmasked": res["sequence_partition_unmasked"]["rank_ms_median"] / launches,
       "scan_ms_per_launch_last5": res["sequence_partition_last5"]["rank_ms_median"] / launches5,
       "log_partition_reps_ms": lpr["rank_ms_median"],
       "expected_ms_per_launch": lpr["rank_ms_median"] + k16["rank_ms_median"] - k1["rank_ms_median"],
       "unresolved_rows_of_sample": unresolved, "sample_rows": P * T,
       "masked_targets": int(fmasked.sum()), "mean_log_prob": float(np.mean(lp[fmasked == 0])), "log_uniform": float(-np.log(I))}
lines = [f"# sequence_log_probs at {U} users x {n} items ({units} positions) x {I} items, d = {D}, LSTM, T = {T}, temperature {TEMPERATURE}", "",
         f"Kernel time = device events around the launches of a family, median of {REPS} alternating repetitions in one process after a",
         "warm-up call.  scan = SBR_K_RANK (every scan-side kernel of a launch), forward = SBR_K_RECURRENT_FWD.", "",
         "| call | launches counted | scan kernels ms | forward kernels ms | wall ms | all repetitions (scan ms) |", "|---|---|---|---|---|---|"]
for name, r in res.items():
    lines.append(f"| {name} | {r['scans']} | {r['rank_ms_median']:.2f} | {r['forward_ms_median']:.2f} | {r['wall_ms_median']:.1f} | "
                 f"{', '.join(f'{x:.2f}' for x in r['rank_ms'])} |")
ps = out["prefix_route_scaled"]
lines += ["", f"sequence_partition: {launches} launches of 8 192 scan rows, {out['scan_ms_per_launch']:.2f} ms of scan-side kernels per launch masked, "
              f"{out['scan_ms_per_launch_unmasked']:.2f} ms unmasked; last = 5: {launches5} launches, {out['scan_ms_per_launch_last5']:.2f} ms each.",
          f"log_partition_reps over 8 192 rows: {lpr['rank_ms_median']:.2f} ms; recommend_reps k = 1 / 16: {k1['rank_ms_median']:.2f} / "
          f"{k16['rank_ms_median']:.2f} ms.  Expected per masked launch = log_partition + (k = 16 scan - k = 1 scan) = "
          f"{out['expected_ms_per_launch']:.2f} ms; measured {out['scan_ms_per_launch']:.2f} ms.",
          f"Unresolved rows: {unresolved} of the {P * T} rows of the first {P} users (untrained model).  Masked targets: {out['masked_targets']} of {units}.",
          f"Mean log-prob at T = {TEMPERATURE}: {out['mean_log_prob']:.4f} (uniform: {out['log_uniform']:.4f}).",
          f"The route it replaces — log_partition + score_candidates over every explicit prefix — was run on {P} users and is SCALED by {scale:.0f} to "
          f"{U} users: scan {ps['rank_ms']:.0f} ms, forward {ps['forward_ms']:.0f} ms, wall {ps['wall_ms']:.0f} ms (scaled, not measured at that size; "
          f"its {P * T} scan rows are one launch where {U} users would fill {launches}).", ""]
print("\n".join(lines), flush=True)
if out_base:
    with open(out_base + ".json", "w") as f:
        json.dump(out, f, indent=1)
    with open(out_base + ".md", "w") as f:
        f.write("\n".join(lines))
