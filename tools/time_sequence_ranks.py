"""Times sbr_sequence_ranks (rank_test_score / rank_gemm / rank_prefix kernels behind one forward pass per sequence) at catalogue
scale: 1M items, dim 128, LSTM, T = 64, U users of 65 items each — 64 positions per user, so U = 8 192 is 64 launches of 8 192
scan rows — in full and with last = 5, against the route it replaces: rank_targets over every explicit prefix as a "user" of its
own, timed on PREFIX_USERS users and SCALED to U by the user count (said so in the output).

    python tools/time_sequence_ranks.py [users] [--out profiles/sequence_ranks_8192x1M_d128]     (writes .json and .md)
    python tools/time_sequence_ranks.py --neighbours [--root DIR]     (one JSON line: mrr_score and rank_targets kernel ms)

One process; the seeded untrained LSTM of tools/time_rank_targets.py.  A warm-up call of each, then REPS alternating repetitions;
kernel time = the engine's device events around the launches of the SBR_K_RANK family (the three scan kernels of a launch
together) and of SBR_K_RECURRENT_FWD (the forward pass); the split of the scan family by kernel comes from a profiler's kernel
trace of this script, not from the ledger.  --neighbours measures the two calls next to the new one and nothing else, so it runs
unchanged against another checkout (--root: where sbr_rs_amd is imported from), for the no-regression comparison in alternating
processes."""
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
from helpers import hparams, synthetic_interactions  # noqa: E402
from sbr_rs_amd._abi import ModelKind  # noqa: E402
from sbr_rs_amd.engine import Model  # noqa: E402

I, D, T = 1_000_000, 128, 64
REPS = 3
PREFIX_USERS = 32
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

if "--neighbours" in sys.argv:
    ptr, it = synthetic_interactions(8192, I, 40, seed=5, min_len=2)
    ptr64 = ptr.astype(np.int64)
    keep = np.ones(it.size, dtype=bool)
    keep[ptr64[1:] - 1] = False
    hist_items = np.ascontiguousarray(it[keep])
    hist_ptr = (ptr64 - np.arange(8192 + 1)).astype(np.uint64)
    tp = np.arange(8192 + 1, dtype=np.uint64) * 10
    ti = np.random.RandomState(9).randint(0, I, 8192 * 10).astype(np.uint32)
    res = timed(m, {"mrr_score": lambda: m.mrr_score(ptr, it), "rank_targets_T10": lambda: m.rank_targets(hist_ptr, hist_items, tp, ti)}, REPS)
    print(json.dumps({name: {"rank_ms_median": r["rank_ms_median"], "rank_ms": r["rank_ms"]} for name, r in res.items()}), flush=True)
    sys.exit(0)

rs = np.random.RandomState(5)
n = T + 1
ptr = (np.arange(U + 1, dtype=np.uint64) * n)
it = rs.randint(0, I, U * n).astype(np.uint32)
units = U * T
# the route it replaces, on the first PREFIX_USERS users: every prefix a history of its own, its next item the one target
P = min(PREFIX_USERS, U)
pre_hist = [it[u * n: u * n + p] for u in range(P) for p in range(1, n)]
pre_ptr = np.concatenate([[0], np.cumsum([h.size for h in pre_hist])]).astype(np.uint64)
pre_items = np.ascontiguousarray(np.concatenate(pre_hist))
pre_tp = np.arange(P * T + 1, dtype=np.uint64)
pre_ti = np.ascontiguousarray(np.array([it[u * n + p] for u in range(P) for p in range(1, n)], dtype=np.uint32))

calls = {"sequence_ranks": lambda: m.sequence_ranks(ptr, it),
         "sequence_ranks_last5": lambda: m.sequence_ranks(ptr, it, last=5),
         "mrr_score": lambda: m.mrr_score(ptr, it),
         f"rank_targets_prefixes_{P}_users": lambda: m.rank_targets(pre_ptr, pre_items, pre_tp, pre_ti)}
res = timed(m, calls, REPS)

# the same integers by both routes, and the last position is mrr_score's rank
_p, full = m.sequence_ranks(ptr, it)
assert np.array_equal(full[: P * T], m.rank_targets(pre_ptr, pre_items, pre_tp, pre_ti))
assert np.array_equal(full.reshape(U, T)[:, -1], m.mrr_score(ptr, it)[1])
assert np.array_equal(full.reshape(U, T)[:, -5:].ravel(), m.sequence_ranks(ptr, it, last=5)[1])

launches = (units + 8191) // 8192
scale = U / P
pre = res[f"rank_targets_prefixes_{P}_users"]
seq, mrr = res["sequence_ranks"], res["mrr_score"]
out = {"users": U, "items": I, "dim": D, "max_sequence_length": T, "units": units, "launches_of_8192": launches, "reps": REPS,
       "calls": res, "prefix_route_users": P, "prefix_route_scale": scale,
       "prefix_route_scaled": {k: pre[k + "_median"] * scale for k in ("rank_ms", "forward_ms", "wall_ms")},
       "scan_ms_per_launch": seq["rank_ms_median"] / launches,
       "mrr_score_scan_ms_per_launch": mrr["rank_ms_median"] / max(1, mrr["scans"])}
lines = [f"# sequence_ranks at {U} users x {n} items ({units} positions) x {I} items, d = {D}, LSTM, T = {T}", "",
         f"Kernel time = device events around the launches of a family, median of {REPS} alternating repetitions in one process after a",
         "warm-up call.  scan = SBR_K_RANK (rank_test_score + rank_gemm + rank_prefix of every launch), forward = SBR_K_RECURRENT_FWD.", "",
         "| call | scans | scan kernels ms | forward kernels ms | wall ms | all repetitions (scan ms) |", "|---|---|---|---|---|---|"]
for name, r in res.items():
    lines.append(f"| {name} | {r['scans']} | {r['rank_ms_median']:.2f} | {r['forward_ms_median']:.2f} | {r['wall_ms_median']:.1f} | "
                 f"{', '.join(f'{x:.2f}' for x in r['rank_ms'])} |")
ps = out["prefix_route_scaled"]
lines += ["", f"sequence_ranks: {launches} launches of 8 192 scan rows, {out['scan_ms_per_launch']:.2f} ms of scan kernels per launch; "
              f"mrr_score on the same users: {out['mrr_score_scan_ms_per_launch']:.2f} ms per launch.",
          f"The route it replaces — rank_targets over every explicit prefix — was run on {P} users and is SCALED by {scale:.0f} to {U} users: "
          f"scan {ps['rank_ms']:.0f} ms, forward {ps['forward_ms']:.0f} ms, wall {ps['wall_ms']:.0f} ms (scaled, not measured at that size; "
          f"its {P * T} scan rows are one launch where {U} users would fill {launches}).", ""]
print("\n".join(lines), flush=True)
if out_base:
    with open(out_base + ".json", "w") as f:
        json.dump(out, f, indent=1)
    with open(out_base + ".md", "w") as f:
        f.write("\n".join(lines))
