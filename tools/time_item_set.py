"""Times the item-set calls at catalogue scale: 8 192 rows x 1M items, d = 128, untrained model, one process per measurement run.

    python tools/time_item_set.py --parent-tree DIR [--rounds 3] [--trace] [--out profiles/item_set_8192x1M_d128]   (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child ...`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. the untouched calls — recommend_reps (k = 1, 10, 100), recommend_sampled_reps (k = 10), log_partition_reps, the above count
     scan and recommend_among_reps (|S| = 1e5, k = 10) — parent tree and this tree ALTERNATING, `--rounds` processes each;
  2. recommend_among_reps of the parent (the last of its processes) against the set's recommend_reps of this tree (the last of
     its processes) for the same S at |S| = 1e4, 1e5, 1e6, k = 10 and 100;
  3. this tree: every other family through a set of 1e5 items against the only exact route the parent has, the plain call under a
     tag filter whose bit marks S — kernel time and wall time;
  4. this tree: recommend_sampled_reps through the set against recommend_sampled_reps on a second model whose table is exactly
     the set's rows — the difference is the cost of the id stream;
  5. with --trace (needs rocprofv3 on the path): one more process of this tree under `rocprofv3 --kernel-trace`, in a run of its
     own: a store of 8 192 slots with W = 128 and 128 items each, recommend through a set of 1e5 items; the per-dispatch durations
     of session_seen_lists_kernel and subset_positions_kernel.

Kernel time = the engine's device events around the launches of the SBR_K_RANK family, median of the repetitions after a warm-up
call; wall time = the whole call from Python."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

argv = sys.argv[1:]


def _opt(name, default=None):
    return argv[argv.index(name) + 1] if name in argv else default


HERE = os.path.dirname(os.path.abspath(__file__))
U, I, D, T = 8192, 1_000_000, 128, 64
SIZES = (10_000, 100_000, 1_000_000)
KS = (10, 100)
REPS = 5
UNTOUCHED = ("recommend_k1", "recommend_k10", "recommend_k100", "sampled_k10", "log_partition", "count_above", "among_1e5_k10")


def item_set_of(np, n):
    return np.sort(np.random.RandomState(n % 1000 + 3).choice(I, n, replace=False)).astype(np.uint32) if n < I else np.arange(I, dtype=np.uint32)


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

    def timed(m, fn, reps=REPS):
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

    m = Model(hparams(I, T, D, int(ModelKind.EWMA), 2, B=1024))
    bias = (np.random.RandomState(1).randn(I) * 0.1).astype(np.float32)
    m.set_param(Param.ITEM_BIAS, bias)
    reps = m.get_param_rows(Param.ITEM_EMBEDDING, np.random.RandomState(9).randint(0, I, U).astype(np.uint32))
    res = {}
    if "--trace" in argv:  # under rocprofv3: a warm-up call, then one call
        W = 128
        store = m.sessions(U, remember=W)
        slots = np.arange(U, dtype=np.uint32)
        rs = np.random.RandomState(4)
        ptr = np.arange(U + 1, dtype=np.uint64) * W
        store.append(slots, (ptr, rs.randint(0, I, U * W).astype(np.uint32)))
        on = m.item_set(item_set_of(np, 100_000)).on(store)
        on.recommend(slots, 10)
        on.recommend(slots, 10)
        return
    th = float(np.sort(m.recommend_reps(reps[:64], 100)[1][:, -1])[32])  # a bar about 100 items per row pass
    res["threshold"] = th
    S5 = item_set_of(np, 100_000)
    calls = {"recommend_k1": lambda: m.recommend_reps(reps, 1), "recommend_k10": lambda: m.recommend_reps(reps, 10),
             "recommend_k100": lambda: m.recommend_reps(reps, 100), "sampled_k10": lambda: m.recommend_sampled_reps(reps, 10, seed=1),
             "log_partition": lambda: m.log_partition_reps(reps), "count_above": lambda: m.count_above_reps(reps, th),
             "among_1e5_k10": lambda: m.recommend_among_reps(reps, 10, S5)}
    for name in UNTOUCHED:
        res[name] = timed(m, calls[name])
        print(f"{name}: {res[name]}", flush=True)
    if "--among" in argv:  # the parent's route within a set: the sub-table gathered by every launch
        res["among"] = {}
        for n in SIZES:
            S = item_set_of(np, n)
            for k in KS:
                res["among"][f"{n}_k{k}"] = timed(m, lambda: m.recommend_among_reps(reps, k, S))
                print(f"among |S|={n} k={k}: {res['among'][f'{n}_k{k}']}", flush=True)
    if "--sets" in argv:
        res["set"] = {}
        for n in SIZES:
            S = item_set_of(np, n)
            t0 = time.perf_counter()
            s = m.item_set(S)
            m.synchronize()
            res["set"][f"{n}_create_wall_ms"] = (time.perf_counter() - t0) * 1e3
            for k in KS:
                res["set"][f"{n}_k{k}"] = timed(m, lambda: s.recommend_reps(reps, k))
                print(f"set |S|={n} k={k}: {res['set'][f'{n}_k{k}']}", flush=True)
            if n == 100_000:  # the identity at scale, on 512 rows
                a, b = s.recommend_reps(reps[:512], 10), m.recommend_among_reps(reps[:512], 10, S)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            s.close()
        # every other family: the set against the plain call under a tag filter that selects S
        s = m.item_set(S5)
        tags = np.zeros(I, np.uint32)
        tags[S5] = 1
        m.set_item_tags(tags)
        m.set_item_groups((np.arange(I, dtype=np.uint32) * np.uint32(2654435761)) % np.uint32(100_000))
        ths = float(np.sort(s.recommend_reps(reps[:64], 100)[1][:, -1])[32])
        fam = {"recommend_k10": (lambda: s.recommend_reps(reps, 10), lambda: m.recommend_reps(reps, 10, any_of=1)),
               "recommend_k100": (lambda: s.recommend_reps(reps, 100), lambda: m.recommend_reps(reps, 100, any_of=1)),
               "sampled_k10": (lambda: s.recommend_sampled_reps(reps, 10, seed=1), lambda: m.recommend_sampled_reps(reps, 10, seed=1, any_of=1)),
               "log_partition": (lambda: s.log_partition_reps(reps), lambda: m.log_partition_reps(reps, any_of=1)),
               "count_above": (lambda: s.count_above_reps(reps, ths), lambda: m.count_above_reps(reps, ths, any_of=1)),
               "recommend_above": (lambda: s.recommend_above_reps(reps, ths), lambda: m.recommend_above_reps(reps, ths, any_of=1)),
               "nth_score_100": (lambda: s.nth_score_reps(reps, 100), lambda: m.nth_score_reps(reps, 100, any_of=1)),
               "capped_k10": (lambda: s.recommend_capped_reps(reps, 10, exact=False), lambda: m.recommend_capped_reps(reps, 10, any_of=1, exact=False)),
               "diverse_k10_pool40": (lambda: s.recommend_diverse_reps(reps, 10, 40), lambda: m.recommend_diverse_reps(reps, 10, 40, any_of=1))}
        res["families"] = {}
        for name, (through_set, by_tags) in fam.items():
            res["families"][name] = {"set": timed(m, through_set, 3), "tags": timed(m, by_tags, 3)}
            print(f"family {name}: {res['families'][name]}", flush=True)
        a, b = s.recommend_sampled_reps(reps[:512], 10, seed=1), m.recommend_sampled_reps(reps[:512], 10, seed=1, any_of=1)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))  # the same draws by both routes
        # mapped noise: the same scan on a model whose table is exactly the set's rows
        m2 = Model(hparams(S5.size, T, D, int(ModelKind.EWMA), 2, B=1024))
        m2.set_param(Param.ITEM_EMBEDDING, m.get_param_rows(Param.ITEM_EMBEDDING, S5))
        m2.set_param(Param.ITEM_BIAS, bias[S5])
        res["noise"] = {"set": timed(m, lambda: s.recommend_sampled_reps(reps, 10, seed=1)),
                        "own_table": timed(m2, lambda: m2.recommend_sampled_reps(reps, 10, seed=1)),
                        "set_plain": timed(m, lambda: s.recommend_reps(reps, 10)), "own_table_plain": timed(m2, lambda: m2.recommend_reps(reps, 10))}
        print(f"noise: {res['noise']}", flush=True)
    json.dump(res, open(_opt("--out"), "w"), indent=1)


def run_child(tree, out, flags=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--out", out] + list(flags)
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=900)  # a child that fails or hangs ends the whole run
    return json.load(open(out))


def trace(tree, out_dir):
    """{kernel: [ms of every dispatch, in order]} of the traced child"""
    shutil.rmtree(out_dir, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out_dir, "-o", "run", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--trace", "--tree", tree, "--out", os.devnull]
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=900)
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    rows.sort()
    out = {"session_seen_lists_kernel": [], "subset_positions_kernel": [], "topk_gemm_kernel": [], "topk_merge_kernel": []}
    for _, name, ms in rows:
        for key in out:
            if key in name:
                out[key].append(ms)
    return out


def driver():
    this_tree = os.path.abspath(os.path.join(HERE, ".."))
    parent_tree = os.path.abspath(_opt("--parent-tree"))
    rounds = int(_opt("--rounds", "3"))
    out = _opt("--out", os.path.join(this_tree, "profiles", "item_set_8192x1M_d128"))
    tmp = out + ".child.json"
    res = {"rows": U, "columns": I, "dim": D, "reps": REPS, "rounds": rounds, "parent": [], "change": []}
    keep = lambda x: {k: v for k, v in x.items() if k in UNTOUCHED}  # noqa: E731
    for r in range(rounds):  # alternating: parent, change, parent, change, ...
        lastp = run_child(parent_tree, tmp, ["--among"] if r == rounds - 1 else [])
        res["parent"].append(keep(lastp))
        last = run_child(this_tree, tmp, ["--sets"] if r == rounds - 1 else [])
        res["change"].append(keep(last))
    os.remove(tmp)
    res["among"], res["set"], res["families"], res["noise"] = lastp["among"], last["set"], last["families"], last["noise"]
    if "--trace" in argv:  # the timings above stand without it: a failed trace is recorded, not fatal
        try:
            res["trace"] = trace(this_tree, out + ".trace")
        except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
            res["trace"] = {"error": repr(e)}
            print("trace failed:", e, flush=True)
        shutil.rmtree(out + ".trace", ignore_errors=True)
    med = lambda runs, key: sorted(x[key]["kernels_ms"] for x in runs)[len(runs) // 2]  # noqa: E731
    L = [f"# Item sets at {U} rows x {I} items, d = {D}", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} repetitions (3 in sections 3) after a warm-up call;",
         "wall = the whole call from Python.  Untrained EWMA model, representations = rows of the item table.", "",
         "## 1. the untouched calls: parent commit against this build", "",
         f"{rounds} processes of each build, alternating (parent, this build, parent, ...); every process's median, then the median of those.", "",
         "| call | parent kernels ms (each process) | this build kernels ms (each process) | parent median | this build median | this / parent |",
         "|---|---|---|---|---|---|"]
    for key in UNTOUCHED:
        p, c = med(res["parent"], key), med(res["change"], key)
        L.append(f"| {key} | " + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["parent"]) + " | "
                 + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["change"]) + f" | {p:.2f} | {c:.2f} | {c / p:.4f} |")
    L += ["", "## 2. the set's recommend_reps (this build) against the parent's recommend_among_reps of the same S", "",
          "| items in S | k | parent among: kernels ms (wall) | set: kernels ms (wall) | set / among, kernels | set / among, wall | set creation wall ms |",
          "|---|---|---|---|---|---|---|"]
    for n in SIZES:
        for k in KS:
            a, s = res["among"][f"{n}_k{k}"], res["set"][f"{n}_k{k}"]
            L.append(f"| {n} | {k} | {a['kernels_ms']:.2f} ({a['wall_ms']:.1f}) | {s['kernels_ms']:.2f} ({s['wall_ms']:.1f}) | "
                     f"{s['kernels_ms'] / a['kernels_ms']:.3f} | {s['wall_ms'] / a['wall_ms']:.3f} | {res['set'][f'{n}_create_wall_ms']:.1f} |")
    L += ["", "## 3. every family through a set of 1e5 items against the plain call under a tag filter that selects S (this build)", "",
          "| call | through the set: kernels ms (wall) | by tags: kernels ms (wall) | set / tags, kernels | set / tags, wall |", "|---|---|---|---|---|"]
    for name, r in res["families"].items():
        s, t = r["set"], r["tags"]
        L.append(f"| {name} | {s['kernels_ms']:.2f} ({s['wall_ms']:.1f}) | {t['kernels_ms']:.2f} ({t['wall_ms']:.1f}) | "
                 f"{s['kernels_ms'] / t['kernels_ms']:.3f} | {s['wall_ms'] / t['wall_ms']:.3f} |")
    nz = res["noise"]
    L += ["", "## 4. the id stream: recommend_sampled_reps (k = 10) through the set of 1e5 items against a model whose table is the set's rows", "",
          f"Through the set {nz['set']['kernels_ms']:.2f} ms of kernels, on the table of its own {nz['own_table']['kernels_ms']:.2f} ms: "
          f"{nz['set']['kernels_ms'] / nz['own_table']['kernels_ms']:.3f}.  The plain recommend_reps (k = 10) beside it, which has no id stream and one "
          f"more launch through the set (positions to ids): {nz['set_plain']['kernels_ms']:.2f} against {nz['own_table_plain']['kernels_ms']:.2f} ms."]
    tr = res.get("trace", {})
    if tr.get("subset_positions_kernel"):
        L += ["", "## 5. sessions: a store of 8 192 slots, W = 128, 128 items each, recommend (k = 10) through a set of 1e5 items (a kernel trace, a run of its own)", "",
              "Per dispatch, in order (a warm-up call and one call), ms: session_seen_lists_kernel " +
              ", ".join(f"{x:.3f}" for x in tr["session_seen_lists_kernel"]) + "; subset_positions_kernel " +
              ", ".join(f"{x:.3f}" for x in tr["subset_positions_kernel"]) + "; topk_gemm_kernel " +
              ", ".join(f"{x:.3f}" for x in tr["topk_gemm_kernel"]) + "; topk_merge_kernel " + ", ".join(f"{x:.3f}" for x in tr["topk_merge_kernel"]) + "."]
    elif "--trace" in argv:
        L += ["", "## 5. sessions", "", "Not measured: the kernel trace failed (" + str(tr.get("error")) + ")."]
    else:
        L += ["", "## 5. sessions", "", "Not measured: run without --trace."]
    L += ["", "## Not measured", "", "A trained model; d = 256; sets on a partitioned item table."]
    L.append("")
    print("\n".join(L), flush=True)
    json.dump(res, open(out + ".json", "w"), indent=1)
    with open(out + ".md", "w") as fh:
        fh.write("\n".join(L))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
