"""Times log_partition at catalogue scale: 8 192 users x 1M items, d = 128, T = 1, untrained model, one process per measurement run.

    python tools/time_log_partition.py --parent-tree DIR [--rounds 3] [--out profiles/log_partition_8192x1M_d128]   (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child ...`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. recommend_reps(k = 1) and recommend_sampled_reps(k = 10), parent tree and this tree ALTERNATING, `--rounds` processes each: the
     existing instantiations must not have slowed (the project's noise floor is 3 %);
  2. log_partition_reps of the same rows in the same process as a measurement of this tree, without and with exclusion lists
     (EXCL entries per user).  The ledger times the SBR_K_RANK family as a whole, so the parts are differences of calls in one
     process: k = 1 scan = recommend_reps(k = 1); sum scan (with the one-block shift kernel) = log_partition_reps without lists
     minus that; finish = log_partition_reps with lists minus recommend_reps(k = 1) with the same lists minus the sum scan;
  3. the host route it replaces, on HOST_USERS users: predict over the whole catalogue per user, then a float64 numpy logsumexp.

Kernel time = the engine's device events around the launches of the SBR_K_RANK family, median of REPS repetitions after a warm-up
call; wall time = the whole call from Python."""
import json
import os
import subprocess
import sys
import time

argv = sys.argv[1:]


def _opt(name, default=None):
    return argv[argv.index(name) + 1] if name in argv else default


HERE = os.path.dirname(os.path.abspath(__file__))
U, I, D, T = 8192, 1_000_000, 128, 64
REPS = 5
EXCL = 20
HOST_USERS = 128


def child():
    root = os.path.abspath(_opt("--tree"))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import torch

    torch.zeros(1, device="cuda")  # PyTorch's HIP runtime first (tests/conftest.py)
    from helpers import hparams
    from sbr_rs_amd._abi import ModelKind, Param
    from sbr_rs_amd.engine import Model

    def timed(fn, reps=REPS, warm=True):
        if warm:
            fn()
        m.timing_enable(True)
        kern, wall = [], []
        for _ in range(reps):
            m.timing_read()
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(m.timing_read()["RANK"][0])
        m.timing_enable(False)
        return {"kernels_ms": float(np.median(kern)), "wall_ms": float(np.median(wall)), "kernels_all_ms": [float(x) for x in kern]}

    m = Model(hparams(I, T, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
    bias = (np.random.RandomState(1).randn(I) * 0.1).astype(np.float32)
    m.set_param(Param.ITEM_BIAS, bias)
    reps = m.get_param_rows(Param.ITEM_EMBEDDING, np.random.RandomState(9).randint(0, I, U).astype(np.uint32))
    res = {"recommend_k1": timed(lambda: m.recommend_reps(reps, 1)),
           "sampled_k10": timed(lambda: m.recommend_sampled_reps(reps, 10, temperature=1.0, seed=11))}
    print(res, flush=True)
    if "--partition" in argv:
        excl = [r for r in np.random.RandomState(3).randint(0, I, (U, EXCL)).astype(np.uint32)]
        res["recommend_k1_lists"] = timed(lambda: m.recommend_reps(reps, 1, exclude=excl))
        res["partition"] = timed(lambda: m.log_partition_reps(reps, 1.0))
        res["partition_lists"] = timed(lambda: m.log_partition_reps(reps, 1.0, exclude=excl))
        res["sampled_k10_log_prob"] = timed(lambda: m.recommend_sampled_reps(reps, 10, temperature=1.0, seed=11, log_prob=True), reps=3)
        a, b = m.log_partition_reps(reps[:300], 1.0), m.log_partition_reps(reps, 1.0)
        assert np.array_equal(a.shift.view(np.uint32), b.shift[:300].view(np.uint32)) and np.array_equal(a.mass, b.mass[:300])
        res["mass_over_2F"] = {"min": float(b.mass.min()) / 2.0 ** b.frac_bits, "max": float(b.mass.max()) / 2.0 ** b.frac_bits,
                               "frac_bits": b.frac_bits}
        for key in ("recommend_k1_lists", "partition", "partition_lists", "sampled_k10_log_prob", "mass_over_2F"):
            print(key, res[key], flush=True)
        # 3. the host route: predict of the catalogue per user, float64 logsumexp in numpy
        all_items = np.arange(I, dtype=np.uint32)
        t_pred = t_np = 0.0
        worst = 0.0
        part = m.log_partition_reps(reps[:HOST_USERS], 1.0)
        for u in range(HOST_USERS):
            t0 = time.perf_counter()
            s = m.predict(reps[u], all_items)
            t1 = time.perf_counter()
            z = s.astype(np.float64)
            lz = z.max() + np.log(np.exp(z - z.max()).sum())
            t2 = time.perf_counter()
            t_pred += t1 - t0
            t_np += t2 - t1
            worst = max(worst, abs(lz - part.log_z[u]))
        res["host_route"] = {"users": HOST_USERS, "predict_ms": t_pred * 1e3, "numpy_ms": t_np * 1e3, "max_abs_log_z_difference": worst,
                             "log_partition": timed(lambda: m.log_partition_reps(reps[:HOST_USERS], 1.0), reps=3)}
        print("host route", res["host_route"], flush=True)
    with open(_opt("--out"), "w") as fh:
        json.dump(res, fh, indent=1)


def run_child(tree, out, partition=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--out", out] + (["--partition"] if partition else [])
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=600)  # a child that fails or hangs ends the whole run
    return json.load(open(out))


def driver():
    this_tree = os.path.abspath(os.path.join(HERE, ".."))
    parent_tree = os.path.abspath(_opt("--parent-tree"))
    rounds = int(_opt("--rounds", "3"))
    out = _opt("--out", os.path.join(this_tree, "profiles", "log_partition_8192x1M_d128"))
    tmp = out + ".child.json"
    res = {"users": U, "items": I, "dim": D, "reps": REPS, "rounds": rounds, "parent": [], "change": []}
    for r in range(rounds):  # alternating: parent, change, parent, change, ...
        res["parent"].append(run_child(parent_tree, tmp))
        last = run_child(this_tree, tmp, partition=(r == rounds - 1))
        res["change"].append({k: last[k] for k in ("recommend_k1", "sampled_k10")})
    os.remove(tmp)
    res["partition_run"] = last
    med = lambda runs, key, what: sorted(x[key][what] for x in runs)[len(runs) // 2]  # noqa: E731
    L = [f"# log_partition at {U} users x {I} items, d = {D}, T = 1", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} repetitions after a warm-up call; wall = the whole",
         "call from Python.  Untrained model, representations = rows of the item table.", "",
         "## 1. the existing scans: parent commit against this build", "",
         f"{rounds} processes of each build, alternating (parent, this build, parent, ...); every process's median, then the median of those.", "",
         "| call | parent kernels ms (each process) | this build kernels ms (each process) | parent median | this build median | this / parent | parent wall ms | this build wall ms |",
         "|---|---|---|---|---|---|---|---|"]
    for key, name in (("recommend_k1", "recommend_reps(k = 1)"), ("sampled_k10", "recommend_sampled_reps(k = 10)")):
        p, c = med(res["parent"], key, "kernels_ms"), med(res["change"], key, "kernels_ms")
        L.append(f"| {name} | " + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["parent"]) + " | "
                 + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["change"])
                 + f" | {p:.2f} | {c:.2f} | {c / p:.4f} | {med(res['parent'], key, 'wall_ms'):.1f} | {med(res['change'], key, 'wall_ms'):.1f} |")
    k1, k1l, pa, pl = (last[x] for x in ("recommend_k1", "recommend_k1_lists", "partition", "partition_lists"))
    sum_scan = pa["kernels_ms"] - k1["kernels_ms"]
    finish = pl["kernels_ms"] - k1l["kernels_ms"] - sum_scan
    L += ["", "## 2. log_partition_reps of the same rows (same process, this build)", "",
          f"Four launches without exclusion lists (scan, merge, shift, sum scan), five with ({EXCL} random entries per user: the finish).", "",
          "| call | kernels ms | wall ms |", "|---|---|---|",
          f"| recommend_reps(k = 1) | {k1['kernels_ms']:.2f} | {k1['wall_ms']:.1f} |",
          f"| recommend_reps(k = 1), lists | {k1l['kernels_ms']:.2f} | {k1l['wall_ms']:.1f} |",
          f"| log_partition_reps | {pa['kernels_ms']:.2f} | {pa['wall_ms']:.1f} |",
          f"| log_partition_reps, lists | {pl['kernels_ms']:.2f} | {pl['wall_ms']:.1f} |",
          f"| recommend_sampled_reps(k = 10) | {last['sampled_k10']['kernels_ms']:.2f} | {last['sampled_k10']['wall_ms']:.1f} |",
          f"| recommend_sampled_reps(k = 10, log_prob=True) | {last['sampled_k10_log_prob']['kernels_ms']:.2f} | {last['sampled_k10_log_prob']['wall_ms']:.1f} |",
          "", "| part (differences of the rows above) | kernels ms | against recommend_reps(k = 1) |", "|---|---|---|",
          f"| k = 1 scan and merge | {k1['kernels_ms']:.2f} | 1 |",
          f"| shift + sum scan | {sum_scan:.2f} | {sum_scan / k1['kernels_ms']:.3f} |",
          f"| finish ({EXCL} entries per user) | {finish:.2f} | {finish / k1['kernels_ms']:.3f} |",
          "", f"mass / 2^F over the {U} rows: {last['mass_over_2F']['min']:.1f} .. {last['mass_over_2F']['max']:.1f} (F = {last['mass_over_2F']['frac_bits']}).",
          "", f"## 3. the host route it replaces, on {HOST_USERS} users", "",
          "predict over the whole catalogue per user, then a float64 logsumexp in numpy.", "",
          "| predict ms | numpy ms | host route ms | log_partition_reps kernels ms | wall ms | max abs log_z difference |", "|---|---|---|---|---|---|"]
    h = last["host_route"]
    L.append(f"| {h['predict_ms']:.0f} | {h['numpy_ms']:.0f} | {h['predict_ms'] + h['numpy_ms']:.0f} | {h['log_partition']['kernels_ms']:.2f} | "
             f"{h['log_partition']['wall_ms']:.1f} | {h['max_abs_log_z_difference']:.2e} |")
    L.append("")
    print("\n".join(L), flush=True)
    with open(out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    with open(out + ".md", "w") as fh:
        fh.write("\n".join(L))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
