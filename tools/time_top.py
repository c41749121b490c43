"""Times the budget scans (recommend_top / audience_top) at catalogue scale: 8 192 rows x 1M columns, d = 128, untrained model, one
process per measurement run.

    python tools/time_top.py --parent-tree DIR [--rounds 3] [--out profiles/top_8192x1M_d128]   (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child ...`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. recommend_reps(k = 1, 10, 100), log_partition_reps and count_above_reps, parent tree and this tree ALTERNATING, `--rounds`
     processes each: the existing instantiations share a translation unit with the new kernels and must not have slowed (the
     project's noise floor is 3 %);
  2. this tree, in the last of its processes: the select alone (nth_score_reps) and the whole call (recommend_top_reps, order="id")
     for 8 192 rows at n = 1 000 and 50 000 — kernel time and wall time; the same through a session store of 1M sessions for 100
     query items (nth_audience_score, audience_top);
  3. the only route the parent offers, written against the parent's API and run on the parent's library in the last of ITS
     processes: a host bisection on count_above_reps (count_audience_above) over the scores' monotone integer keys, per row, down to
     adjacent f32 values, then recommend_above_reps (audience_above) at the thresholds found, order="id".  It returns more than n
     where scores tie at the bar;
  4. with --trace (needs rocprofv3 on the path): one more process of this tree under `rocprofv3 --kernel-trace`, which runs
     nth_score_reps and recommend_top_reps once each at n = 50 000 after a warm-up; the per-dispatch durations give the launch count
     and the cost of each round, the first one — where every score is binned — apart.

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
KS = (1, 10, 100)
REPS = 5
BUDGETS = (1000, 50_000)
ROUTE_Q = 100


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
    if "--trace" in argv:  # under rocprofv3: one call of each form after a warm-up, marked by a count scan between them
        m.nth_score_reps(reps, BUDGETS[-1])
        m.count_above_reps(reps, 1e30)
        m.nth_score_reps(reps, BUDGETS[-1])
        m.count_above_reps(reps, 1e30)
        m.recommend_top_reps(reps, BUDGETS[0], order="id", max_results=U * BUDGETS[0])
        return
    for k in KS:
        res[f"recommend_k{k}"] = timed(lambda: m.recommend_reps(reps, k))
        print(f"recommend_reps k={k}: {res[f'recommend_k{k}']}", flush=True)
    res["partition"] = timed(lambda: m.log_partition_reps(reps, 1.0))
    print(f"log_partition_reps: {res['partition']}", flush=True)
    bar = np.full(U, 0.25, np.float32)
    res["count"] = timed(lambda: m.count_above_reps(reps, bar))
    print(f"count_above_reps: {res['count']}", flush=True)
    rs = np.random.RandomState(3)
    if "--top" not in argv and "--route" not in argv:
        json.dump(res, open(_opt("--out"), "w"), indent=1)
        return

    def key_of(x):
        b = np.where(x == 0, np.float32(0.0), x).astype(np.float32).view(np.uint32)
        return np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000)).astype(np.uint64)

    def unkey(k):
        k = k.astype(np.uint32)
        return np.where(k >> 31 == 1, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)

    def bisect(count, rows, n):
        """per row the largest f32 at which `count` still passes at least n columns: 32 halvings over the keys of the finite f32
        values, one count call each — the parent's only way to an order statistic"""
        lo = np.full(rows, int(key_of(np.float32(-3.0e38))[()]), np.uint64)  # count(lo) >= n is taken for granted
        hi = np.full(rows, int(key_of(np.float32(3.0e38))[()]), np.uint64)  # count(hi) < n
        calls = 0
        while np.any(hi - lo > 1):
            mid = (lo + hi) // 2
            ok = count(unkey(mid)) >= n
            calls += 1
            lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid)
        return unkey(lo), calls

    S = I
    slots = np.arange(S, dtype=np.uint32)
    st = m.sessions(S)
    st.append(slots, (np.arange(S + 1, dtype=np.uint64), rs.randint(0, I, S).astype(np.uint32)))
    qs = rs.randint(0, I, ROUTE_Q).astype(np.uint32)
    if "--route" in argv:
        res["route"] = {}
        for n in BUDGETS:
            t0 = time.perf_counter()
            th, calls = bisect(lambda x: m.count_above_reps(reps, x), U, n)
            bis_ms = (time.perf_counter() - t0) * 1e3
            cnt = m.count_above_reps(reps, th)
            t0 = time.perf_counter()
            got = m.recommend_above_reps(reps, th, max_results=int(cnt.sum()), order="id")
            fill_ms = (time.perf_counter() - t0) * 1e3
            r = {"bisection_wall_ms": bis_ms, "count_calls": calls, "above_wall_ms": fill_ms, "wall_ms": bis_ms + fill_ms,
                 "pairs": int(got.ptr[-1]), "rows_over_n": int(np.count_nonzero(got.counts > n)), "cuts_head": [float(x) for x in th[:4]]}
            del got
            t0 = time.perf_counter()
            tq, calls = bisect(lambda x: st.count_audience_above(qs, x), ROUTE_Q, n)
            bis_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            got = st.audience_above(qs, tq, max_results=int(st.count_audience_above(qs, tq).sum()), order="id")
            fill_ms = (time.perf_counter() - t0) * 1e3
            r["audience"] = {"bisection_wall_ms": bis_ms, "count_calls": calls, "above_wall_ms": fill_ms, "wall_ms": bis_ms + fill_ms,
                             "pairs": int(got.ptr[-1]), "cuts_head": [float(x) for x in tq[:4]]}
            res["route"][str(n)] = r
            print(f"route n={n}: {r}", flush=True)
    if "--top" in argv:
        res["top"] = {}
        for n in BUDGETS:
            sel = timed(lambda: m.nth_score_reps(reps, n))
            cuts, counts = m.nth_score_reps(reps, n)
            full = timed(lambda: m.recommend_top_reps(reps, n, max_results=U * n, order="id"), reps=3)
            r = {"select": sel, "call": full, "pairs": int(counts.sum()), "cuts_head": [float(x) for x in cuts[:4]],
                 "tied_at_cut": int(m.count_above_reps(reps, cuts).sum() - counts.sum())}
            sel_a = timed(lambda: st.nth_audience_score(qs, n))
            full_a = timed(lambda: st.audience_top(qs, n, max_results=ROUTE_Q * n, order="id"), reps=3)
            cuts_a, counts_a = st.nth_audience_score(qs, n)
            r["audience"] = {"select": sel_a, "call": full_a, "pairs": int(counts_a.sum()), "cuts_head": [float(x) for x in cuts_a[:4]]}
            res["top"][str(n)] = r
            print(f"top n={n}: {r}", flush=True)
        top = m.recommend_reps(reps[:256], 10)
        got = m.recommend_top_reps(reps[:256], 10)
        assert all(np.array_equal(got.row(u)[0], top[0][u]) for u in range(256))
    st.close()
    json.dump(res, open(_opt("--out"), "w"), indent=1)


def run_child(tree, out, flags=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--out", out] + list(flags)
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=900)  # a child that fails or hangs ends the whole run
    return json.load(open(out))


def trace(tree, out_dir):
    """the dispatches of the traced child, in order: [(kernel name, ms)]"""
    shutil.rmtree(out_dir, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out_dir, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
           "--child", "--trace", "--tree", tree, "--out", os.devnull]
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=900)
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    rows.sort()
    names = [("select_gemm_kernel", "select scan"), ("select_step_kernel", "select step"), ("above_gemm_kernel", "above scan"),
             ("above_offsets_kernel", "offsets"), ("top_trim_kernel", "trim")]
    seq = [(next((short for key, short in names if key in name), None), ms) for _, name, ms in rows]
    seq = [x for x in seq if x[0]]
    # the child's calls: warm-up select (17 dispatches) | count (2) | select (17) | count (2) | whole call
    count = ["above scan", "offsets"]
    a_select = ["select step"] + ["select scan", "select step"] * 8
    ok = [x[0] for x in seq[:38]] == a_select + count + a_select + count
    return {"all": seq, "select": seq[19:36] if ok else [], "call": seq[38:] if ok else []}


def driver():
    this_tree = os.path.abspath(os.path.join(HERE, ".."))
    parent_tree = os.path.abspath(_opt("--parent-tree"))
    rounds = int(_opt("--rounds", "3"))
    out = _opt("--out", os.path.join(this_tree, "profiles", "top_8192x1M_d128"))
    tmp = out + ".child.json"
    res = {"rows": U, "columns": I, "dim": D, "reps": REPS, "rounds": rounds, "parent": [], "change": []}
    keep = lambda x: {k: v for k, v in x.items() if k.startswith("recommend_k") or k in ("partition", "count")}  # noqa: E731
    for r in range(rounds):  # alternating: parent, change, parent, change, ...
        lastp = run_child(parent_tree, tmp, ["--route"] if r == rounds - 1 else [])
        res["parent"].append(keep(lastp))
        last = run_child(this_tree, tmp, ["--top"] if r == rounds - 1 else [])
        res["change"].append(keep(last))
    os.remove(tmp)
    res["top"], res["route"] = last["top"], lastp["route"]
    if "--trace" in argv:  # the timings above stand without it: a failed trace is recorded, not fatal
        try:
            res["trace"] = trace(this_tree, out + ".trace")
        except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
            res["trace"] = {"error": repr(e)}
            print("trace failed:", e, flush=True)
        shutil.rmtree(out + ".trace", ignore_errors=True)
    med = lambda runs, key, what: sorted(x[key][what] for x in runs)[len(runs) // 2]  # noqa: E731
    L = [f"# recommend_top / audience_top at {U} rows x {I} columns, d = {D}", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} repetitions (3 for the whole calls) after a warm-up",
         "call; wall = the whole call from Python.  Untrained EWMA model, representations = rows of the item table.", "",
         "## 1. the existing scans: parent commit against this build", "",
         f"{rounds} processes of each build, alternating (parent, this build, parent, ...); every process's median, then the median of those.", "",
         "| call | parent kernels ms (each process) | this build kernels ms (each process) | parent median | this build median | this / parent |",
         "|---|---|---|---|---|---|"]
    names = [(f"recommend_k{k}", f"recommend_reps(k = {k})") for k in KS] + [("partition", "log_partition_reps"), ("count", "count_above_reps")]
    for key, name in names:
        p, c = med(res["parent"], key, "kernels_ms"), med(res["change"], key, "kernels_ms")
        L.append(f"| {name} | " + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["parent"]) + " | "
                 + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["change"]) + f" | {p:.2f} | {c:.2f} | {c / p:.4f} |")
    cnt = med(res["change"], "count", "kernels_ms")
    L += ["", "## 2. the budget calls (this build, one process) against the parent's route (the parent's library, one process)", "",
          "The route: a host bisection on the count form over the f32 keys, per row, down to adjacent values, then the *_above call at the",
          "thresholds found (order=\"id\").  The new call: order=\"id\", max_results = rows x n.  Wall time of one call, ms.", "",
          "| question | n | route: count calls | route: bisection | route: *_above | route total | new: select alone (kernels) | new: whole call (kernels) | new / route |",
          "|---|---|---|---|---|---|---|---|---|"]
    for n in BUDGETS:
        t, r = res["top"][str(n)], res["route"][str(n)]
        L.append(f"| recommend_top_reps, {U} rows | {n} | {r['count_calls']} | {r['bisection_wall_ms']:.0f} | {r['above_wall_ms']:.0f} | {r['wall_ms']:.0f} | "
                 f"{t['select']['wall_ms']:.1f} ({t['select']['kernels_ms']:.1f}) | {t['call']['wall_ms']:.0f} ({t['call']['kernels_ms']:.1f}) | "
                 f"{t['call']['wall_ms'] / r['wall_ms']:.3f} |")
        ta, ra = t["audience"], r["audience"]
        L.append(f"| audience_top, {ROUTE_Q} queries x {I} sessions | {n} | {ra['count_calls']} | {ra['bisection_wall_ms']:.0f} | {ra['above_wall_ms']:.0f} | "
                 f"{ra['wall_ms']:.0f} | {ta['select']['wall_ms']:.1f} ({ta['select']['kernels_ms']:.1f}) | {ta['call']['wall_ms']:.1f} "
                 f"({ta['call']['kernels_ms']:.1f}) | {ta['call']['wall_ms'] / ra['wall_ms']:.3f} |")
    L += ["", "Pairs returned: " + "; ".join(f"n = {n}: {res['top'][str(n)]['pairs']} (route: {res['route'][str(n)]['pairs']}, "
                                              f"{res['route'][str(n)]['rows_over_n']} rows over n; tied at the cut beyond n: {res['top'][str(n)]['tied_at_cut']})"
                                              for n in BUDGETS) + ".",
          f"The select alone is 8 scans and 9 steps; against the count scan ({cnt:.2f} ms) it is " +
          ", ".join(f"{res['top'][str(n)]['select']['kernels_ms'] / cnt:.2f}x at n = {n}" for n in BUDGETS) + "."]
    if res.get("trace", {}).get("select"):
        sel, call = res["trace"]["select"], res["trace"]["call"]
        scans = [ms for name, ms in sel if name == "select scan"]
        steps = [ms for name, ms in sel if name == "select step"]
        L += ["", f"## 3. the rounds, from a kernel trace (one nth_score_reps at n = {BUDGETS[-1]}, one recommend_top_reps at n = {BUDGETS[0]})", "",
              f"The select's dispatches: {len(scans)} select scans and {len(steps)} steps, {len(sel)} launches and nothing else between them.",
              "", "| round | digit | select scan ms | / count scan |", "|---|---|---|---|"]
        for i, ms in enumerate(scans):
            L.append(f"| {i} | bits {31 - 4 * i}..{28 - 4 * i} | {ms:.2f} | {ms / cnt:.2f} |")
        L += ["", f"Steps: {sum(steps) * 1e3:.0f} us in all.  The whole call's dispatches after the select: " +
              ", ".join(f"{name} {ms:.2f}" for name, ms in call if name not in ("select scan", "select step")) + " (ms)."]
    L.append("")
    print("\n".join(L), flush=True)
    json.dump(res, open(out + ".json", "w"), indent=1)
    with open(out + ".md", "w") as fh:
        fh.write("\n".join(L))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
