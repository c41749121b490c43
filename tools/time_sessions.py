"""Times the session store against what a caller does without it: U sessions x 1M items, dim 128, LSTM, histories of 128 items
(= max_sequence_length).

    python tools/time_sessions.py [sessions] [--out profiles/sessions_8192x1M_d128]     (writes .json and .md)

With a store   : append one item to every session (session_lstm_step_kernel + session_commit_kernel), and
                 sessions.recommend(k = 100), the scan reading the store's rows in place.
Without a store: user_representations of the same sessions' full 128-item histories (the forward pass a new event costs today),
                 recommend(k = 100) from those histories, and recommend_reps(k = 100) from host rows — the same scan as
                 sessions.recommend on the same rows, fed from the host.  Nothing is excluded in any of the three recommends.

One process; a seeded untrained LSTM and synthetic histories.  A warm-up call of each, then REPS alternating repetitions; kernel
time = the engine's device events around the launches of the SBR_K_RECURRENT_FWD and SBR_K_RANK families, wall time = host clock
around the call (every call ends in a stream synchronise); medians.  Before timing, the store filled with the histories must give
user_representations' bits."""
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
from sbr_rs_amd._abi import ModelKind  # noqa: E402
from sbr_rs_amd.engine import Model, device_info  # noqa: E402

out_base = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
args = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_base]
U, I, D, T = int(args[0]) if args else 8192, 1_000_000, 128, 128
REPS, K = 7, 100

m = Model(hparams(I, T, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
rs = np.random.RandomState(5)
items = rs.randint(0, I, U * T).astype(np.uint32)
ptr = np.arange(U + 1, dtype=np.uint64) * T
slots = np.arange(U, dtype=np.uint32)
one_ptr = np.arange(U + 1, dtype=np.uint64)
one = rs.randint(0, I, U).astype(np.uint32)

st = m.sessions(U)
st.append(slots, (ptr, items))
reps = m.user_representations(ptr, items)
assert np.array_equal(st.representations(slots).view(np.uint32), reps.view(np.uint32)), "store and forward pass disagree"
a = st.recommend(slots, K)
b = m.recommend_reps(reps, K)
assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "in-place scan and recommend_reps disagree"

calls = {
    "sessions.append (1 item each)": lambda: st.append(slots, (one_ptr, one)),
    f"sessions.recommend k={K}": lambda: st.recommend(slots, K),
    f"user_representations ({T}-item histories)": lambda: m.user_representations(ptr, items),
    f"recommend k={K} (from histories)": lambda: m.recommend(ptr, items, K, include_history=True),
    f"recommend_reps k={K} (host rows)": lambda: m.recommend_reps(reps, K),
}
for fn in calls.values():  # warm-up (arena growth, first launches)
    fn()
m.timing_enable(True)
fwd = {name: [] for name in calls}
scan = {name: [] for name in calls}
wall = {name: [] for name in calls}
for _ in range(REPS):
    for name, fn in calls.items():
        m.timing_read()
        t0 = time.perf_counter()
        fn()
        wall[name].append((time.perf_counter() - t0) * 1e3)
        t = m.timing_read()
        fwd[name].append(t["RECURRENT_FWD"][0])
        scan[name].append(t["RANK"][0])
m.timing_enable(False)

name_dev, cus, hbm = device_info()
res = {"device": name_dev, "cus": cus, "sessions": U, "items": I, "dim": D, "history": T, "reps": REPS, "k": K, "calls": {}}
for name in calls:
    res["calls"][name] = {"recurrent_kernels_ms_median": float(np.median(fwd[name])), "scan_kernels_ms_median": float(np.median(scan[name])),
                          "wall_ms_median": float(np.median(wall[name])), "recurrent_kernels_ms_all": fwd[name],
                          "scan_kernels_ms_all": scan[name], "wall_ms_all": wall[name]}
lines = [f"# sessions at {U} sessions x {I} items, d = {D}, LSTM, {T}-item histories", "",
         f"Device: {name_dev}, {cus} CUs.  One process, a warm-up call of each, then {REPS} alternating repetitions; medians.",
         "Kernel ms = device events around the launches of the recurrent family (forward pass / session step + commit) and of the",
         "scan family (top-k GEMM + merge, row copies); wall ms = host clock around the call, which ends in a stream synchronise and",
         "includes packing, uploads and the copy of the results.", "",
         "| call | recurrent kernels ms | scan kernels ms | wall ms | all repetitions (wall ms) |", "|---|---|---|---|---|"]
for name, r in res["calls"].items():
    lines.append(f"| {name} | {r['recurrent_kernels_ms_median']:.3f} | {r['scan_kernels_ms_median']:.3f} | {r['wall_ms_median']:.2f} | "
                 f"{', '.join(f'{x:.2f}' for x in r['wall_ms_all'])} |")
c = res["calls"]
ap, fw = c["sessions.append (1 item each)"], c[f"user_representations ({T}-item histories)"]
sr, rr, rh = c[f"sessions.recommend k={K}"], c[f"recommend_reps k={K} (host rows)"], c[f"recommend k={K} (from histories)"]
res["ratios"] = {"forward_over_append_kernels": fw["recurrent_kernels_ms_median"] / max(ap["recurrent_kernels_ms_median"], 1e-9),
                 "forward_over_append_wall": fw["wall_ms_median"] / max(ap["wall_ms_median"], 1e-9),
                 "sessions_recommend_over_recommend_reps_wall": sr["wall_ms_median"] / max(rr["wall_ms_median"], 1e-9),
                 "recommend_from_histories_over_sessions_recommend_wall": rh["wall_ms_median"] / max(sr["wall_ms_median"], 1e-9)}
r = res["ratios"]
lines += ["", f"One-item append against the full forward pass it replaces: kernels x{r['forward_over_append_kernels']:.1f}, "
              f"wall x{r['forward_over_append_wall']:.1f} in the append's favour.",
          f"sessions.recommend against recommend_reps on the same rows: wall x{r['sessions_recommend_over_recommend_reps_wall']:.3f} "
          f"(scan kernels {sr['scan_kernels_ms_median']:.3f} vs {rr['scan_kernels_ms_median']:.3f} ms); "
          f"recommend from the histories takes x{r['recommend_from_histories_over_sessions_recommend_wall']:.2f} its wall time.", ""]
print("\n".join(lines), flush=True)
if out_base:
    with open(out_base + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(out_base + ".md", "w") as f:
        f.write("\n".join(lines))
st.close()
