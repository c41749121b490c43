"""Times the capped top-k (recommend_capped_reps) at catalogue scale: 8 192 rows x 1M items, d = 128, untrained model, one process per
measurement run.

    python tools/time_capped.py --parent-tree DIR [--rounds 3] [--trace] [--out profiles/capped_8192x1M_d128]   (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child ...`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. recommend_reps(k = 10, 100), parent tree and this tree ALTERNATING, `--rounds` processes each: topk_gemm_kernel is not edited
     and shares a translation unit with the new kernel, so these must sit inside the project's noise floor (3 %);
  2. this tree, in the last of its processes: for uniform groups (1e5 of them) and Zipf-sized groups whose largest holds about 30 %
     of the items, k = 10 and 100, cap = 1 and 2, the default pool — the library call (exact=False: the scan at k = pool and the
     select, kernel time and wall time), the plain scan at k = pool beside it, the share of rows the pool leaves incomplete, and
     the wall time of the whole exact call, whose difference to the library call is the completion;
  3. the route this replaces, written against the parent's API and run on the parent's library in the last of ITS processes:
     recommend_reps(k = pool) to the host and the rule in numpy over the rows (which is not exact: its incomplete rows stay short);
  4. with --trace (needs rocprofv3 on the path): one more process of this tree under `rocprofv3 --kernel-trace`, in a run of its
     own, one library call per (groups, k, cap) after a warm-up; the per-dispatch durations give the scan's and
     capped_select_kernel's kernel time apart.

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
KS = (10, 100)
CAPS = (1, 2)
REPS = 5
NO_GROUP = 0xFFFFFFFF


def default_pool(k):
    return min(1024, max(64, 4 * k))


def group_sets(np):
    """uniform: 1e5 groups of 10 items; zipf: group sizes ~ rank^-a over 1e5 groups with a found by bisection so that the largest
    holds 30 % of the items"""
    rs = np.random.RandomState(5)
    uniform = rs.permutation(I).astype(np.uint32) % np.uint32(100_000)
    ranks = np.arange(1, 100_001, dtype=np.float64)
    lo, hi = 1.0, 3.0
    for _ in range(60):
        a = (lo + hi) / 2
        lo, hi = (a, hi) if 1.0 / np.sum(ranks ** -a) < 0.30 else (lo, a)
    p = ranks ** -lo
    zipf = rs.choice(100_000, size=I, p=p / p.sum()).astype(np.uint32)
    return {"uniform": uniform, "zipf": zipf}


def host_rule(np, ids, groups, cap, k):
    """the rule on one pool row (padding cut off), in numpy: the positions kept"""
    ids = ids[ids != NO_GROUP]
    g = groups[ids]
    by = np.argsort(g, kind="stable")
    first = np.searchsorted(g[by], g[by], side="left")
    ordinal = np.empty(g.size, np.int64)
    ordinal[by] = np.arange(g.size) - first
    return np.flatnonzero((g == NO_GROUP) | (ordinal < cap))[:k]


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

    m = Model(hparams(I, T, D, int(ModelKind.EWMA), 2, B=1024))
    m.set_param(Param.ITEM_BIAS, (np.random.RandomState(1).randn(I) * 0.1).astype(np.float32))
    reps = m.get_param_rows(Param.ITEM_EMBEDDING, np.random.RandomState(9).randint(0, I, U).astype(np.uint32))
    res = {}
    if "--trace" in argv:  # under rocprofv3: a warm-up call, then one library call per case
        m.set_item_groups(np.arange(I, dtype=np.uint32))
        m.recommend_capped_reps(reps, 10, 1, exact=False)
        for name, groups in group_sets(np).items():
            m.set_item_groups(groups)
            for k in KS:
                for cap in CAPS:
                    m.recommend_capped_reps(reps, k, cap, exact=False)
        return
    for k in KS:
        res[f"recommend_k{k}"] = timed(lambda: m.recommend_reps(reps, k))
        print(f"recommend_reps k={k}: {res[f'recommend_k{k}']}", flush=True)
    if "--route" in argv:  # the parent's only way: the pool to the host, the rule there
        res["route"] = {}
        for name, groups in group_sets(np).items():
            for k in KS:
                for cap in CAPS:
                    pool = default_pool(k)
                    short = [0]

                    def route():
                        items, scores = m.recommend_reps(reps, pool)
                        out_i = np.full((U, k), NO_GROUP, np.uint32)
                        out_s = np.full((U, k), -np.inf, np.float32)
                        short[0] = 0
                        for u in range(U):
                            kept = host_rule(np, items[u], groups, cap, k)
                            out_i[u, : kept.size], out_s[u, : kept.size] = items[u, kept], scores[u, kept]
                            short[0] += kept.size < k
                        return out_i, out_s

                    r = timed(route, reps=3)
                    r["short_rows"] = int(short[0])
                    res["route"][f"{name}_k{k}_cap{cap}"] = r
                    print(f"route {name} k={k} cap={cap}: {r}", flush=True)
    if "--capped" in argv:
        res["capped"] = {}
        for k in KS:
            res[f"scan_pool_k{k}"] = timed(lambda: m.recommend_reps(reps, default_pool(k)))
        for name, groups in group_sets(np).items():
            m.set_item_groups(groups)
            for k in KS:
                for cap in CAPS:
                    lib = timed(lambda: m.recommend_capped_reps(reps, k, cap, exact=False))
                    flags = m.recommend_capped_reps(reps, k, cap, exact=False)[2]
                    whole = timed(lambda: m.recommend_capped_reps(reps, k, cap), reps=3)
                    r = {"library": lib, "exact": whole, "pool": default_pool(k), "incomplete_rows": int((~flags).sum()),
                         "completion_wall_ms": whole["wall_ms"] - lib["wall_ms"]}
                    res["capped"][f"{name}_k{k}_cap{cap}"] = r
                    print(f"capped {name} k={k} cap={cap}: {r}", flush=True)
        own = np.arange(I, dtype=np.uint32)
        m.set_item_groups(own)  # the identity, at scale: every item its own group is recommend
        a, b = m.recommend_capped_reps(reps[:512], 10), m.recommend_reps(reps[:512], 10)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2].all()
    json.dump(res, open(_opt("--out"), "w"), indent=1)


def run_child(tree, out, flags=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--out", out] + list(flags)
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=900)  # a child that fails or hangs ends the whole run
    return json.load(open(out))


def trace(tree, out_dir):
    """kernel time per kernel of the traced child: {short name: [ms of every dispatch, in order]}"""
    shutil.rmtree(out_dir, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "run", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--trace", "--tree", tree, "--out", os.devnull]
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=900)
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    rows.sort()
    out = {"topk_gemm_kernel": [], "topk_merge_kernel": [], "capped_select_kernel": []}
    for _, name, ms in rows:
        for key in out:
            if key in name:
                out[key].append(ms)
    return out


def driver():
    this_tree = os.path.abspath(os.path.join(HERE, ".."))
    parent_tree = os.path.abspath(_opt("--parent-tree"))
    rounds = int(_opt("--rounds", "3"))
    out = _opt("--out", os.path.join(this_tree, "profiles", "capped_8192x1M_d128"))
    tmp = out + ".child.json"
    res = {"rows": U, "columns": I, "dim": D, "reps": REPS, "rounds": rounds, "parent": [], "change": []}
    keep = lambda x: {k: v for k, v in x.items() if k.startswith("recommend_k")}  # noqa: E731
    for r in range(rounds):  # alternating: parent, change, parent, change, ...
        lastp = run_child(parent_tree, tmp, ["--route"] if r == rounds - 1 else [])
        res["parent"].append(keep(lastp))
        last = run_child(this_tree, tmp, ["--capped"] if r == rounds - 1 else [])
        res["change"].append(keep(last))
    os.remove(tmp)
    res["capped"], res["route"] = last["capped"], lastp["route"]
    res["scan_pool"] = {str(k): last[f"scan_pool_k{k}"] for k in KS}
    if "--trace" in argv:  # the timings above stand without it: a failed trace is recorded, not fatal
        try:
            res["trace"] = trace(this_tree, out + ".trace")
        except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
            res["trace"] = {"error": repr(e)}
            print("trace failed:", e, flush=True)
        shutil.rmtree(out + ".trace", ignore_errors=True)
    med = lambda runs, key, what: sorted(x[key][what] for x in runs)[len(runs) // 2]  # noqa: E731
    L = [f"# recommend_capped at {U} rows x {I} items, d = {D}", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} repetitions (3 for the exact calls and the route)",
         "after a warm-up call; wall = the whole call from Python.  Untrained EWMA model, representations = rows of the item table.", "",
         "## 1. the unchanged calls: parent commit against this build", "",
         f"{rounds} processes of each build, alternating (parent, this build, parent, ...); every process's median, then the median of those.", "",
         "| call | parent kernels ms (each process) | this build kernels ms (each process) | parent median | this build median | this / parent |",
         "|---|---|---|---|---|---|"]
    for k in KS:
        key = f"recommend_k{k}"
        p, c = med(res["parent"], key, "kernels_ms"), med(res["change"], key, "kernels_ms")
        L.append(f"| recommend_reps(k = {k}) | " + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["parent"]) + " | "
                 + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["change"]) + f" | {p:.2f} | {c:.2f} | {c / p:.4f} |")
    L += ["", "## 2. the capped call (this build, one process) against the route it replaces (the parent's library, one process)", "",
          "Library call: recommend_capped_reps(exact=False) — the scan at k = pool and capped_select_kernel.  Scan alone: recommend_reps(k = pool).",
          "Exact call: exact=True, the incomplete rows finished through recommend_top_reps; completion = its wall time less the library",
          "call's.  Route: recommend_reps(k = pool) to the host and the rule in numpy, row by row; its short rows stay short.", "",
          "| groups | k | cap | pool | scan alone kernels ms | library call kernels ms (wall) | incomplete rows | exact call wall ms | completion wall ms | route wall ms (short rows) | library / route | exact / route |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in ("uniform", "zipf"):
        for k in KS:
            for cap in CAPS:
                c, r = res["capped"][f"{name}_k{k}_cap{cap}"], res["route"][f"{name}_k{k}_cap{cap}"]
                L.append(f"| {name} | {k} | {cap} | {c['pool']} | {res['scan_pool'][str(k)]['kernels_ms']:.2f} | {c['library']['kernels_ms']:.2f} "
                         f"({c['library']['wall_ms']:.1f}) | {c['incomplete_rows']} ({100.0 * c['incomplete_rows'] / U:.1f} %) | {c['exact']['wall_ms']:.1f} | "
                         f"{c['completion_wall_ms']:.1f} | {r['wall_ms']:.0f} ({r['short_rows']}) | {c['library']['wall_ms'] / r['wall_ms']:.3f} | "
                         f"{c['exact']['wall_ms'] / r['wall_ms']:.3f} |")
    tr = res.get("trace", {})
    if tr.get("capped_select_kernel"):
        cs, n = tr["capped_select_kernel"], len(KS) * len(CAPS)
        L += ["", "## 3. the kernels apart, from a kernel trace (a run of its own: one library call per case)", "",
              f"capped_select_kernel, {len(cs)} dispatches in call order — a warm-up call (k = 10, every item its own group), then uniform / zipf x k = {KS} x cap = {CAPS}; a call whose pool makes the scan run in two chunks of 4 096 rows (k = 100: pool 400) has two (ms): " +
              ", ".join(f"{x:.3f}" for x in cs) + ".",
              f"topk_gemm_kernel: {len(tr['topk_gemm_kernel'])} dispatches, {sum(tr['topk_gemm_kernel']):.1f} ms in all; topk_merge_kernel: "
              f"{len(tr['topk_merge_kernel'])} dispatches, {sum(tr['topk_merge_kernel']):.1f} ms in all; capped_select_kernel: {sum(cs):.2f} ms in all, "
              f"{100.0 * sum(cs) / (sum(tr['topk_gemm_kernel']) + sum(tr['topk_merge_kernel']) + sum(cs)):.2f} % of the three ({2 * n} cases and the warm-up)."]
    elif "--trace" in argv:
        L += ["", "## 3. the kernels apart", "", "Not measured: the kernel trace failed (" + str(tr.get("error")) + ")."]
    else:
        L += ["", "## 3. the kernels apart", "", "Not measured: run without --trace.  The select's share is the library call less the scan alone above."]
    L.append("")
    print("\n".join(L), flush=True)
    json.dump(res, open(out + ".json", "w"), indent=1)
    with open(out + ".md", "w") as fh:
        fh.write("\n".join(L))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
