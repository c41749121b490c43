"""Times the threshold scans at catalogue scale: 8 192 rows x 1M columns, d = 128, untrained model, one process per measurement run.

    python tools/time_above.py --parent-tree DIR [--rounds 3] [--out profiles/above_8192x1M_d128]   (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child ...`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. recommend_reps(k = 1, 10, 100) and log_partition_reps, parent tree and this tree ALTERNATING, `--rounds` processes each: the
     existing instantiations share a translation unit with the new kernel and must not have slowed (the project's noise floor is
     3 %).  The sum scan of log_partition is log_partition_reps minus recommend_reps(k = 1), as tools/time_log_partition.py takes it;
  2. the count scan of this tree in the last of its processes: count_above_reps at per-row thresholds that pass about 10, 1 000 and
     100 000 items per row (found per row by bisection on count_above_reps itself), against (1)'s k = 1 scan and sum scan; the same
     through a session store of 1M sessions, count_audience_above of 8 192 query items;
  3. the fill: recommend_above_reps(order="id") at those thresholds — kernel time of the whole call and, minus the count form's, of
     the fill launches; wall time including the copy out; bytes written per second against the sequential-copy figure of
     tools/hbm_ceiling.hip (profiles/r02_hbm_ceiling.jsonl: read + write traffic; the tool records no write-only figure);
  4. the route it replaces, 100 queries x 1M sessions, in the last process of EACH tree (the two host routes are calls the parent has
     too): store.score_candidates on all pairs + numpy >=, and store.representations + a host matmul + numpy >=, against this
     tree's store.audience_above.

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
KS = (1, 10, 100)
REPS = 5
TARGETS = (10, 1000, 100_000)
ROUTE_Q = 100
COPY_GBPS = 4619.0  # tools/hbm_ceiling.hip, sequential copy, read + write traffic (profiles/r02_hbm_ceiling.jsonl); it has no write-only figure


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
    for k in KS:
        res[f"recommend_k{k}"] = timed(lambda: m.recommend_reps(reps, k))
        print(f"recommend_reps k={k}: {res[f'recommend_k{k}']}", flush=True)
    res["partition"] = timed(lambda: m.log_partition_reps(reps, 1.0))
    print(f"log_partition_reps: {res['partition']}", flush=True)
    rs = np.random.RandomState(3)
    if "--above" in argv:
        def thresholds_for(count, rows, target):
            """per row the threshold at which `count` passes about `target` columns: 30 halvings of [-8, 8]"""
            lo, hi = np.full(rows, -8.0, np.float32), np.full(rows, 8.0, np.float32)
            for _ in range(30):
                mid = ((lo + hi) / 2).astype(np.float32)
                more = count(mid) > target
                lo, hi = np.where(more, mid, lo), np.where(more, hi, mid)
            return hi

        res["count"], res["fill"] = {}, {}
        for target in TARGETS:
            t = thresholds_for(lambda x: m.count_above_reps(reps, x), U, target)
            n = m.count_above_reps(reps, t)
            c = timed(lambda: m.count_above_reps(reps, t))
            c["pairs"] = int(n.sum())
            c["per_row"] = [int(n.min()), float(np.median(n)), int(n.max())]
            res["count"][str(target)] = c
            print(f"count_above_reps ~{target}/row: {c}", flush=True)
            cap = int(n.sum())
            f = timed(lambda: m.recommend_above_reps(reps, t, max_results=cap, order="id"), reps=3)
            f["pairs"] = cap
            f["fill_kernels_ms"] = f["kernels_ms"] - c["kernels_ms"]
            f["written_GBps"] = cap * 8 / (f["fill_kernels_ms"] * 1e-3) / 1e9 if f["fill_kernels_ms"] > 0 else None
            res["fill"][str(target)] = f
            print(f"recommend_above_reps ~{target}/row: {f}", flush=True)
        top = m.recommend_reps(reps[:256], 10)
        got = m.recommend_above_reps(reps[:256], top[1][:, 9].copy())
        assert all(np.array_equal(got.row(u)[0][:10], top[0][u]) for u in range(256))
    if "--route" in argv or "--above" in argv:
        S = I
        slots = np.arange(S, dtype=np.uint32)
        st = m.sessions(S)
        st.append(slots, (np.arange(S + 1, dtype=np.uint64), rs.randint(0, I, S).astype(np.uint32)))
        queries = rs.randint(0, I, U).astype(np.uint32)
        qs = queries[:ROUTE_Q]
        t0 = time.perf_counter()
        flat = st.score_candidates(slots, (np.arange(S + 1, dtype=np.uint64) * ROUTE_Q, np.tile(qs, S)))
        sc = np.concatenate(flat).reshape(S, ROUTE_Q).T
        bar = np.float32(np.quantile(sc[:, ::97], 0.999))  # about 1 000 sessions per query
        hits = [np.flatnonzero(row >= bar) for row in sc]
        pairs_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        h = st.representations(slots)
        e = m.get_param_rows(Param.ITEM_EMBEDDING, qs)
        b = m.get_param_rows(Param.ITEM_BIAS, qs).ravel()
        sc2 = e @ h.T + b[:, None]
        hits2 = [np.flatnonzero(row >= bar) for row in sc2]
        matmul_ms = (time.perf_counter() - t0) * 1e3
        res["route"] = {"queries": ROUTE_Q, "sessions": S, "threshold": float(bar), "pairs": int(sum(x.size for x in hits)),
                        "score_candidates_numpy_wall_ms": pairs_ms, "representations_matmul_wall_ms": matmul_ms,
                        "matmul_route_pairs": int(sum(x.size for x in hits2))}
        del flat, sc2, h
        if "--above" in argv:
            a = timed(lambda: st.audience_above(qs, bar, order="id"), reps=3)
            got = st.audience_above(qs, bar, order="id")
            a["rows_equal_the_pairs_route"] = bool(all(np.array_equal(got.row(j)[0], hits[j]) and
                                                       np.array_equal(got.row(j)[1].view(np.uint32), sc[j][hits[j]].view(np.uint32))
                                                       for j in range(ROUTE_Q)))
            assert a["rows_equal_the_pairs_route"]
            res["route"]["audience_above"] = a
            res["route"]["audience_above_score_order"] = timed(lambda: st.audience_above(qs, bar), reps=3)
            tq = np.full(U, bar, np.float32)
            res["audience_count"] = timed(lambda: st.count_audience_above(queries, tq))
            res["audience_count"]["pairs"] = int(st.count_audience_above(queries, tq).sum())
            print(f"count_audience_above: {res['audience_count']}", flush=True)
        print(f"route: {res['route']}", flush=True)
        st.close()
    with open(_opt("--out"), "w") as fh:
        json.dump(res, fh, indent=1)


def run_child(tree, out, flags=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--out", out] + list(flags)
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=900)  # a child that fails or hangs ends the whole run
    return json.load(open(out))


def driver():
    this_tree = os.path.abspath(os.path.join(HERE, ".."))
    parent_tree = os.path.abspath(_opt("--parent-tree"))
    rounds = int(_opt("--rounds", "3"))
    out = _opt("--out", os.path.join(this_tree, "profiles", "above_8192x1M_d128"))
    tmp = out + ".child.json"
    res = {"rows": U, "columns": I, "dim": D, "reps": REPS, "rounds": rounds, "parent": [], "change": []}
    for r in range(rounds):  # alternating: parent, change, parent, change, ...
        lastp = run_child(parent_tree, tmp, ["--route"] if r == rounds - 1 else [])
        res["parent"].append(lastp)
        last = run_child(this_tree, tmp, ["--above"] if r == rounds - 1 else [])
        res["change"].append({k: v for k, v in last.items() if k.startswith("recommend_k") or k == "partition"})
    os.remove(tmp)
    res["above_run"], res["parent_route"] = last, lastp["route"]
    ceiling = COPY_GBPS
    med = lambda runs, key, what: sorted(x[key][what] for x in runs)[len(runs) // 2]  # noqa: E731
    L = [f"# recommend_above / audience_above at {U} rows x {I} columns, d = {D}", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} repetitions after a warm-up call; wall = the whole",
         "call from Python.  Untrained EWMA model, representations = rows of the item table.", "",
         "## 1. the existing scans: parent commit against this build", "",
         f"{rounds} processes of each build, alternating (parent, this build, parent, ...); every process's median, then the median of those.", "",
         "| call | parent kernels ms (each process) | this build kernels ms (each process) | parent median | this build median | this / parent |",
         "|---|---|---|---|---|---|"]
    names = [(f"recommend_k{k}", f"recommend_reps(k = {k})") for k in KS] + [("partition", "log_partition_reps")]
    for key, name in names:
        p, c = med(res["parent"], key, "kernels_ms"), med(res["change"], key, "kernels_ms")
        L.append(f"| {name} | " + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["parent"]) + " | "
                 + ", ".join(f"{x[key]['kernels_ms']:.2f}" for x in res["change"]) + f" | {p:.2f} | {c:.2f} | {c / p:.4f} |")
    k1 = last["recommend_k1"]["kernels_ms"]
    k1p = med(res["parent"], "recommend_k1", "kernels_ms")
    sum_p = med(res["parent"], "partition", "kernels_ms") - k1p
    L += ["", "## 2. the count scan (this build, one process)", "",
          f"Against the parent's k = 1 scan ({k1p:.2f} ms) and its sum scan (log_partition_reps minus that: {sum_p:.2f} ms).  Two launches: the",
          "scan and the offsets kernel.", "",
          "| per-row thresholds that pass about | pairs | per row min / median / max | kernels ms | / parent k = 1 scan | / parent sum scan | wall ms |",
          "|---|---|---|---|---|---|---|"]
    for target in TARGETS:
        c = last["count"][str(target)]
        L.append(f"| {target} | {c['pairs']} | {c['per_row'][0]} / {c['per_row'][1]:.0f} / {c['per_row'][2]} | {c['kernels_ms']:.2f} | "
                 f"{c['kernels_ms'] / k1p:.3f} | {c['kernels_ms'] / sum_p:.3f} | {c['wall_ms']:.1f} |")
    ac = last["audience_count"]
    L += ["", f"The audience orientation, count_audience_above of {U} query items x {I} sessions at one threshold ({ac['pairs']} pairs): "
          f"{ac['kernels_ms']:.2f} ms of kernels, {ac['wall_ms']:.1f} ms wall (the wall time holds the once-per-call gather of the state table).",
          "", "## 3. the fill (this build, the same process)", "",
          "recommend_above_reps(order=\"id\", max_results = the count): the count scan, the offsets, then the fill launches.  fill = the call's",
          "kernel time minus the count form's.  Bytes written = 8 per pair (id and score)."
          f"  Sequential copy moves {ceiling:.0f} GB/s of read + write traffic (tools/hbm_ceiling.hip; it records no write-only figure).", "",
          "| about per row | pairs | call kernels ms | fill kernels ms | fill / count scan | written GB/s | of the copy figure | wall ms |", "|---|---|---|---|---|---|---|---|"]
    for target in TARGETS:
        f, c = last["fill"][str(target)], last["count"][str(target)]
        gb = f["written_GBps"]
        L.append(f"| {target} | {f['pairs']} | {f['kernels_ms']:.2f} | {f['fill_kernels_ms']:.2f} | {f['fill_kernels_ms'] / c['kernels_ms']:.3f} | "
                 + (f"{gb:.0f}" if gb else "-") + " | " + (f"{gb / ceiling:.2f}" if gb and ceiling else "-") + f" | {f['wall_ms']:.0f} |")
    ro, pr = last["route"], res["parent_route"]
    L += ["", f"## 4. the route it replaces: {ROUTE_Q} queries x {ro['sessions']} sessions, wall time, one call each", "",
          f"One threshold for all queries ({ro['threshold']:.4f}: {ro['pairs']} pairs).", "",
          "| route | parent commit wall ms | this build wall ms |", "|---|---|---|",
          f"| store.score_candidates on all pairs + numpy >= | {pr['score_candidates_numpy_wall_ms']:.0f} | {ro['score_candidates_numpy_wall_ms']:.0f} |",
          f"| store.representations + host matmul + numpy >= | {pr['representations_matmul_wall_ms']:.0f} | {ro['representations_matmul_wall_ms']:.0f} |",
          f"| store.audience_above(order=\"id\") | - | {ro['audience_above']['wall_ms']:.1f} ({ro['audience_above']['kernels_ms']:.2f} of kernels) |",
          f"| store.audience_above (score order) | - | {ro['audience_above_score_order']['wall_ms']:.1f} |", "",
          f"audience_above's rows equal the first route's, ids and score bits: {ro['audience_above']['rows_equal_the_pairs_route']}.  The matmul route sums in",
          f"numpy's own order and selects {ro['matmul_route_pairs']} pairs at the same threshold.", ""]
    print("\n".join(L), flush=True)
    with open(out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    with open(out + ".md", "w") as fh:
        fh.write("\n".join(L))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
