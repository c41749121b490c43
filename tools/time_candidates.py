"""Times the candidates family at catalogue scale — recommend_among_reps, score_candidates_reps, user_representations — beside what a
caller had before them: 8 192 users x 1M items, d = 128 (score_candidates also at d = 32), untrained models, one process per run.

    python tools/time_candidates.py --baseline [--tree DIR] --out base.json      # the calls that predate the family
    python tools/time_candidates.py [--baseline-json base.json] [--out profiles/candidates_8192x1M_d128]   (writes .json and .md)

--baseline measures, with the package of DIR (default: this tree; point it at a checkout of the parent commit):
  (a) recommend_reps with the complement of S as every user's exclusion list — the only way to the answer without recommend_among.
      The lists are num_users x (num_items - |S|) ids on the host, so (a) runs on A_USERS users and its times are scaled to 8 192
      (the scan is linear in 128-user tiles; the host work in users): the figures say so;
  (b) the floor: recommend_reps on a model whose table is exactly the |S| gathered rows;
  256 predict calls of 1 000 candidates and 256 user_representation calls of 64 items, wall time, scaled by 32 to 8 192.
The default run measures the new calls (and (b) again in its own process).  Kernel time = the engine's device events around the
launches of the SBR_K_RANK family, median of REPS repetitions after a warm-up call; wall time = the whole call."""
import json
import os
import sys
import time

argv = sys.argv[1:]


def _opt(name):
    return argv[argv.index(name) + 1] if name in argv else None


ROOT = os.path.abspath(_opt("--tree") or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

torch.zeros(1, device="cuda")  # PyTorch's HIP runtime first (tests/conftest.py)
from helpers import hparams  # noqa: E402
from sbr_rs_amd._abi import ModelKind, Param  # noqa: E402
from sbr_rs_amd.engine import Model  # noqa: E402

BASELINE = "--baseline" in argv
U, I, D, T = 8192, 1_000_000, 128, 64
A_USERS = 256
SIZES = (10_000, 100_000, 500_000, 1_000_000)
KS = (10, 100)
REPS = 3
CANDS = 1000
SCALE_CALLS = 256


def make_model(items, d):
    return Model(hparams(items, T, d, int(ModelKind.LSTM_NORMAL), 2, B=1024))


def subset(n):
    return np.sort(np.random.RandomState(n % 1000 + 1).choice(I, n, replace=False)).astype(np.uint32) if n < I else np.arange(I, dtype=np.uint32)


def timed(model, fn, reps=REPS, warm=True):
    """-> (median RANK kernel ms, median wall ms, median RECURRENT_FWD kernel ms)"""
    if warm:
        fn()
    model.timing_enable(True)
    kern, wall, fwd = [], [], []
    for _ in range(reps):
        model.timing_read()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        t = model.timing_read()
        kern.append(t["RANK"][0])
        fwd.append(t["RECURRENT_FWD"][0])
    model.timing_enable(False)
    return float(np.median(kern)), float(np.median(wall)), float(np.median(fwd))


def floor_model(m, S):
    """a model whose table is exactly the rows of S"""
    if S.size == I:
        return m
    f = make_model(S.size, D)
    f.set_param(Param.ITEM_EMBEDDING, m.get_param_rows(Param.ITEM_EMBEDDING, S))
    f.set_param(Param.ITEM_BIAS, m.get_param_rows(Param.ITEM_BIAS, S))
    return f


m = make_model(I, D)
m.set_param(Param.ITEM_BIAS, (np.random.RandomState(1).randn(I) * 0.1).astype(np.float32))
reps = m.get_param_rows(Param.ITEM_EMBEDDING, np.random.RandomState(9).randint(0, I, U).astype(np.uint32))
res = {"users": U, "items": I, "dim": D, "reps": REPS, "tree": "baseline" if BASELINE else "candidates", "among": {}, "floor": {}}

for n in SIZES:
    S = subset(n)
    f = floor_model(m, S)
    for k in KS:
        kern, wall, _ = timed(f, lambda: f.recommend_reps(reps, k))
        res["floor"][f"S{n}_k{k}"] = {"kernels_ms": kern, "wall_ms": wall}
        print(f"floor |S|={n} k={k}: kernels {kern:.2f} ms wall {wall:.1f} ms", flush=True)
    if not BASELINE:
        for k in KS:
            kern, wall, _ = timed(m, lambda: m.recommend_among_reps(reps, k, S))
            res["among"][f"S{n}_k{k}"] = {"kernels_ms": kern, "wall_ms": wall}
            print(f"among |S|={n} k={k}: kernels {kern:.2f} ms wall {wall:.1f} ms", flush=True)
        gi, gs = m.recommend_among_reps(reps[:256], 10, S)  # the floor's answer, position for position
        fi, fs = f.recommend_reps(reps[:256], 10)
        assert np.array_equal(gi, S[fi]) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32))
    if f is not m:
        f.close()

if BASELINE:
    res["complement"] = {"users": A_USERS, "scale": U / A_USERS}
    for n in SIZES[:-1]:
        outside = np.setdiff1d(np.arange(I, dtype=np.uint32), subset(n))
        excl = [outside] * A_USERS
        for k in KS:
            kern, wall, _ = timed(m, lambda: m.recommend_reps(reps[:A_USERS], k, exclude=excl), reps=1, warm=(n == SIZES[0] and k == KS[0]))
            res["complement"][f"S{n}_k{k}"] = {"kernels_ms": kern, "wall_ms": wall, "kernels_ms_scaled": kern * U / A_USERS,
                                               "wall_ms_scaled": wall * U / A_USERS, "host_list_bytes": int(outside.size) * 4 * A_USERS}
            print(f"complement |S|={n} k={k} ({A_USERS} users): kernels {kern:.2f} ms wall {wall:.1f} ms", flush=True)
        del excl

# ---- score_candidates_reps (and the 8 192 predict calls it replaces), user_representations (and 8 192 single calls) ----
res["score"] = {}
rs = np.random.RandomState(5)
for d in (128, 32):
    md = m if d == D else make_model(I, d)
    rd = reps if d == D else md.get_param_rows(Param.ITEM_EMBEDDING, rs.randint(0, I, U).astype(np.uint32))
    ci = rs.randint(0, I, U * CANDS).astype(np.uint32)
    cp = np.arange(0, U * CANDS + 1, CANDS, dtype=np.uint64)
    r = {}
    if BASELINE:
        def loop():
            for u in range(SCALE_CALLS):
                md.predict(rd[u], ci[u * CANDS: (u + 1) * CANDS])
        _, wall, _ = timed(md, loop)
        r = {"predict_calls": SCALE_CALLS, "wall_ms": wall, "wall_ms_scaled": wall * U / SCALE_CALLS}
        print(f"predict d={d}: {SCALE_CALLS} calls {wall:.1f} ms -> {r['wall_ms_scaled']:.0f} ms for {U}", flush=True)
    else:
        kern, wall, _ = timed(md, lambda: md.score_candidates_reps(rd, cp, ci))
        nbytes = float(U * CANDS) * (4 * d + 4 + 12)
        r = {"pairs": U * CANDS, "kernels_ms": kern, "wall_ms": wall, "algorithmic_bytes": nbytes, "GBps": nbytes / kern / 1e6,
             "gflops": 2.0 * d * U * CANDS / kern / 1e6}
        got = md.score_candidates_reps(rd[:4], cp[:5], ci)
        for u in range(4):
            assert np.array_equal(got[u].view(np.uint32), md.predict(rd[u], ci[u * CANDS: (u + 1) * CANDS]).view(np.uint32))
        print(f"score_candidates d={d}: kernels {kern:.3f} ms ({r['GBps']:.0f} GB/s) wall {wall:.1f} ms", flush=True)
    res["score"][f"d{d}"] = r
    if md is not m:
        md.close()

hist = rs.randint(0, I, U * T).astype(np.uint32)
hp = np.arange(0, U * T + 1, T, dtype=np.uint64)
if BASELINE:
    def loop():
        for u in range(SCALE_CALLS):
            m.user_representation(hist[u * T: (u + 1) * T])
    _, wall, _ = timed(m, loop)
    res["representations"] = {"calls": SCALE_CALLS, "wall_ms": wall, "wall_ms_scaled": wall * U / SCALE_CALLS}
else:
    kern, wall, fwd = timed(m, lambda: m.user_representations(hp, hist))
    res["representations"] = {"rows_kernel_ms": kern, "forward_kernels_ms": fwd, "wall_ms": wall}
    got = m.user_representations(hp[:5], hist)
    for u in range(4):
        assert np.array_equal(got[u].view(np.uint32), m.user_representation(hist[u * T: (u + 1) * T]).view(np.uint32))
print("representations:", res["representations"], flush=True)

out = _opt("--out")
if BASELINE:
    if out:
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
    sys.exit(0)

base = json.load(open(_opt("--baseline-json"))) if _opt("--baseline-json") else None
res["baseline"] = base
L = [f"# The candidates family at {U} users x {I} items, d = {D}", "",
     f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} repetitions after a warm-up call, one process;",
     "wall = the whole call from Python.  `floor` = recommend_reps on a model whose table is exactly the |S| gathered rows ((b));",
     "`floor (parent)` = the same on the parent commit, in its own process; `complement` = recommend_reps on the parent with the",
     f"complement of S as every user's exclusion list ((a)), run on {A_USERS} users and scaled by {U // A_USERS} to {U}.", "",
     "## recommend_among_reps", "",
     "| S | k | among kernels ms | floor kernels ms | among / floor | floor (parent) ms | among / floor (parent) | among wall ms | complement kernels ms (scaled) | complement wall ms (scaled) | complement host lists |",
     "|---|---|---|---|---|---|---|---|---|---|---|"]
for n in SIZES:
    for k in KS:
        key = f"S{n}_k{k}"
        a, fl = res["among"][key], res["floor"][key]
        pf = base["floor"][key]["kernels_ms"] if base else None
        c = base["complement"].get(key) if base else None
        L.append(f"| {n} | {k} | {a['kernels_ms']:.2f} | {fl['kernels_ms']:.2f} | {a['kernels_ms'] / fl['kernels_ms']:.3f} | "
                 + (f"{pf:.2f} | {a['kernels_ms'] / pf:.3f} | " if pf else "- | - | ") + f"{a['wall_ms']:.1f} | "
                 + (f"{c['kernels_ms_scaled']:.0f} | {c['wall_ms_scaled']:.0f} | {c['host_list_bytes'] * (U // A_USERS) / 2**30:.1f} GiB at {U} users |" if c else "- | - | - |"))
L += ["", "## score_candidates_reps", "",
      f"{U} users x {CANDS} uniformly random candidates.  Algorithmic bytes per pair = 4 d + 4 (row, bias) + 12 (id, user row, score);",
      "the figure includes both launches (the call's pairs exceed one launch's cap).", "",
      "| d | kernels ms | GB/s on algorithmic bytes | GFLOP/s | wall ms | 8 192 predict calls on the parent (256 timed, x 32) ms |", "|---|---|---|---|---|---|"]
for d in (128, 32):
    r = res["score"][f"d{d}"]
    b = base["score"][f"d{d}"]["wall_ms_scaled"] if base else None
    L.append(f"| {d} | {r['kernels_ms']:.3f} | {r['GBps']:.0f} | {r['gflops']:.0f} | {r['wall_ms']:.1f} | " + (f"{b:.0f} |" if b else "- |"))
r = res["representations"]
L += ["", "## user_representations", "", f"{U} histories of {T} items.", "",
      f"Batched: wall {r['wall_ms']:.1f} ms (forward kernels {r['forward_kernels_ms']:.2f} ms, row gather {r['rows_kernel_ms']:.3f} ms)."
      + (f"  {U} single calls on the parent (256 timed, x 32): {base['representations']['wall_ms_scaled']:.0f} ms." if base else ""), ""]
print("\n".join(L), flush=True)
if out:
    with open(out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    with open(out + ".md", "w") as fh:
        fh.write("\n".join(L))
