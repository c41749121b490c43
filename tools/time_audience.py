"""Times the audience scan at catalogue scale: 8 192 query items x 1M sessions, d = 128, untrained model, one process per
measurement run.

    python tools/time_audience.py --parent-tree DIR [--rounds 2] [--out profiles/audience_8192x1M_d128]     (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child ...`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. scan parity: recommend_reps of 8 192 users x 1M items at the PARENT commit and in this tree, and store.audience of 8 192 queries
     x 1M sessions in this tree — the same GEMM shape — processes ALTERNATING (parent, this tree, ...), `--rounds` of each;
  2. small Q: store.audience of 1, 32 and 128 queries x 1M sessions: the scan against the time to read the state table once
     (the sequential-read figure of tools/hbm_ceiling.hip recorded in profiles/r02_hbm_ceiling.jsonl, 5.8 TB/s);
  3. against doing without: wall time of store.audience for 100 queries, k = 1 000, against store.score_candidates on every
     (slot, item) pair + numpy argpartition, and against store.representations + a host matmul + argpartition;
  4. the seen-list build: a store with W = 128 and 128 remembered items per session, the call against include_seen=True;
  1b. (last) the same score matrix through recommend_reps and audience in one process: no item bias, slot s holding item s.

Kernel time = the engine's device events around the launches of the SBR_K_RANK family (for audience: the scan, the merge and the
id mapping of every chunk — not the once-per-call gather, nor the seen-list build, which are in the wall time), median of REPS
repetitions after a warm-up call; wall time = the whole call from Python."""
import json
import os
import subprocess
import sys
import time

argv = sys.argv[1:]


def _opt(name, default=None):
    return argv[argv.index(name) + 1] if name in argv else default


HERE = os.path.dirname(os.path.abspath(__file__))
Q, S, I, D, T = 8192, 1_000_000, 1_000_000, 128, 64
KS = (10, 100)
REPS = 5
SMALL_Q = (1, 32, 128)
WITHOUT_Q, WITHOUT_K = 100, 1000
W = 128
SEQ_READ_GBPS = 5800.0  # tools/hbm_ceiling.hip, sequential read (profiles/r02_hbm_ceiling.jsonl)


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
    reps = m.get_param_rows(Param.ITEM_EMBEDDING, np.random.RandomState(9).randint(0, I, Q).astype(np.uint32))
    res = {"recommend_reps": {}}
    for k in KS:
        res["recommend_reps"][f"k{k}"] = timed(lambda: m.recommend_reps(reps, k))
        print(f"recommend_reps k={k}: {res['recommend_reps'][f'k{k}']}", flush=True)
    if "--audience" in argv:
        rs = np.random.RandomState(3)
        slots = np.arange(S, dtype=np.uint32)
        queries = rs.randint(0, I, Q).astype(np.uint32)
        st = m.sessions(S)
        st.append(slots, (np.arange(S + 1, dtype=np.uint64), rs.randint(0, I, S).astype(np.uint32)))
        res["audience"] = {}
        for k in KS:
            res["audience"][f"k{k}"] = timed(lambda: st.audience(queries, k))
            print(f"audience k={k}: {res['audience'][f'k{k}']}", flush=True)
        if "--all" in argv:
            res["small_q"] = {}
            for q in SMALL_Q:
                r = timed(lambda: st.audience(queries[:q], 10))
                r["table_GBps"] = S * D * 4 / (r["kernels_ms"] * 1e-3) / 1e9
                res["small_q"][f"q{q}"] = r
                print(f"small Q={q}: {r}", flush=True)
            # against doing without, wall time, one call each behind one warm-up of the audience call
            qs = queries[:WITHOUT_Q]
            a = timed(lambda: st.audience(qs, WITHOUT_K), reps=3)
            got = st.audience(qs, WITHOUT_K)
            t0 = time.perf_counter()
            flat = st.score_candidates(slots, (np.arange(S + 1, dtype=np.uint64) * WITHOUT_Q, np.tile(qs, S)))
            sc = np.concatenate(flat).reshape(S, WITHOUT_Q).T
            top = np.argpartition(-sc, WITHOUT_K, axis=1)[:, :WITHOUT_K]
            pairs_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            h = st.representations(slots)
            e = m.get_param_rows(Param.ITEM_EMBEDDING, qs)
            b = m.get_param_rows(Param.ITEM_BIAS, qs).ravel()
            sc2 = e @ h.T + b[:, None]
            top2 = np.argpartition(-sc2, WITHOUT_K, axis=1)[:, :WITHOUT_K]
            matmul_ms = (time.perf_counter() - t0) * 1e3
            agree = float(np.mean([np.intersect1d(top[j], got[0][j]).size / WITHOUT_K for j in range(WITHOUT_Q)]))
            agree2 = float(np.mean([np.intersect1d(top2[j], got[0][j]).size / WITHOUT_K for j in range(WITHOUT_Q)]))
            res["without"] = {"audience": a, "score_candidates_argpartition_wall_ms": pairs_ms, "representations_matmul_wall_ms": matmul_ms,
                              "overlap_with_pairs_route": agree, "overlap_with_matmul_route": agree2}
            print(f"without: {res['without']}", flush=True)
            del flat, sc, sc2, h, top, top2
            st.close()
            # the seen-list build
            sm = m.sessions(S, remember=W)
            sm.append(slots, (np.arange(S + 1, dtype=np.uint64), rs.randint(0, I, S).astype(np.uint32)))
            sm.set_seen(slots, (np.arange(S + 1, dtype=np.uint64) * W, rs.randint(0, I, S * W).astype(np.uint32)))
            res["seen"] = {}
            for k in KS:
                on = timed(lambda: sm.audience(queries, k), reps=3)
                off = timed(lambda: sm.audience(queries, k, include_seen=True), reps=3)
                rows = sm.audience(queries, k)[0]
                res["seen"][f"k{k}"] = {"with_lists": on, "include_seen": off, "build_wall_ms": on["wall_ms"] - off["wall_ms"],
                                        "expected_keys": float(Q) * S * W / I}
                assert rows.shape == (Q, k)
                print(f"seen k={k}: {res['seen'][f'k{k}']}", flush=True)
            sm.close()
            # the same score matrix through both scans: no item bias, slot s holds item s, so its state row IS E[s] (EWMA's first
            # step) and recommend_reps of the queries' rows ranks what audience ranks, bit for bit
            m.set_param(Param.ITEM_BIAS, np.zeros(I, np.float32))
            se = m.sessions(S)
            se.append(slots, (np.arange(S + 1, dtype=np.uint64), slots))
            qrows = m.get_param_rows(Param.ITEM_EMBEDDING, queries)
            res["same_scores"] = {}
            for k in KS:
                r = timed(lambda: m.recommend_reps(qrows, k))
                a = timed(lambda: se.audience(queries, k))
                x, y = m.recommend_reps(qrows, k), se.audience(queries, k)
                same = bool(np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)))
                res["same_scores"][f"k{k}"] = {"recommend_reps": r, "audience": a, "rows_equal": same}
                print(f"same scores k={k}: {res['same_scores'][f'k{k}']}", flush=True)
                assert same
            se.close()
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
    rounds = int(_opt("--rounds", "2"))
    out = _opt("--out", os.path.join(this_tree, "profiles", "audience_8192x1M_d128"))
    tmp = out + ".child.json"
    res = {"queries": Q, "sessions": S, "items": I, "dim": D, "reps": REPS, "rounds": rounds, "parent": [], "change": []}
    for r in range(rounds):  # alternating: parent, change, parent, change, ...
        res["parent"].append(run_child(parent_tree, tmp))
        last = run_child(this_tree, tmp, ["--audience"] + (["--all"] if r == rounds - 1 else []))
        res["change"].append(last)
    os.remove(tmp)
    med = lambda runs, what, k: sorted(x[what][f"k{k}"]["kernels_ms"] for x in runs)[len(runs) // 2]  # noqa: E731
    each = lambda runs, what, k: ", ".join(f"{x[what][f'k{k}']['kernels_ms']:.2f}" for x in runs)  # noqa: E731
    L = [f"# The audience scan at {Q} queries x {S} sessions, d = {D}", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} repetitions after a warm-up call; wall = the whole",
         "call from Python.  Untrained EWMA model; one item appended to every slot.", "",
         "## 1. scan parity: audience against recommend_reps of the parent commit (the same GEMM shape)", "",
         f"{rounds} processes of each build, alternating (parent, this build, ...); every process's median, then the median of those.", "",
         "| k | parent recommend_reps ms (each process) | this build recommend_reps ms | this build audience ms | parent median | recommend_reps this / parent | audience / parent recommend_reps |",
         "|---|---|---|---|---|---|---|"]
    for k in KS:
        p, c, a = med(res["parent"], "recommend_reps", k), med(res["change"], "recommend_reps", k), med(res["change"], "audience", k)
        L.append(f"| {k} | {each(res['parent'], 'recommend_reps', k)} | {each(res['change'], 'recommend_reps', k)} | {each(res['change'], 'audience', k)} | "
                 f"{p:.2f} | {c / p:.4f} | {a / p:.4f} |")
    L += ["", "## 1b. the same score matrix through both scans (this build, one process)", "",
          "No item bias and slot s holding item s, so the state table is the item table and recommend_reps of the queries' rows ranks",
          "exactly what audience ranks; the rows of the two calls are compared and are equal, ids and score bits.", "",
          "| k | recommend_reps kernels ms | audience kernels ms | audience / recommend_reps | rows equal |", "|---|---|---|---|---|"]
    for k in KS:
        r = last["same_scores"][f"k{k}"]
        L.append(f"| {k} | {r['recommend_reps']['kernels_ms']:.2f} | {r['audience']['kernels_ms']:.2f} | "
                 f"{r['audience']['kernels_ms'] / r['recommend_reps']['kernels_ms']:.4f} | {r['rows_equal']} |")
    L += ["", "## 2. small Q: the scan against one read of the state table", "",
          f"The table is {S} x {D} floats = {S * D * 4 / 2**20:.0f} MiB; sequential-read ceiling {SEQ_READ_GBPS:.0f} GB/s (tools/hbm_ceiling.hip,",
          "profiles/r02_hbm_ceiling.jsonl).  k = 10.", "",
          "| queries | kernels ms | table bytes / kernel time GB/s | of the ceiling | wall ms |", "|---|---|---|---|---|"]
    for q in SMALL_Q:
        r = last["small_q"][f"q{q}"]
        L.append(f"| {q} | {r['kernels_ms']:.3f} | {r['table_GBps']:.0f} | {r['table_GBps'] / SEQ_READ_GBPS:.2f} | {r['wall_ms']:.1f} |")
    w = last["without"]
    L += ["", f"## 3. against doing without: {WITHOUT_Q} queries, k = {WITHOUT_K}, wall time", "",
          "| route | wall ms |", "|---|---|",
          f"| store.audience | {w['audience']['wall_ms']:.1f} |",
          f"| store.score_candidates on all {WITHOUT_Q} x {S} pairs + numpy argpartition (one call) | {w['score_candidates_argpartition_wall_ms']:.0f} |",
          f"| store.representations + host matmul + argpartition (one call) | {w['representations_matmul_wall_ms']:.0f} |", "",
          f"Share of audience's rows the two host routes also select: {w['overlap_with_pairs_route']:.4f} and {w['overlap_with_matmul_route']:.4f}.  The first route's",
          "scores are audience's bits, so what it selects differently are ties at the k-th score, which argpartition breaks arbitrarily",
          "(sessions that hold the same single item have identical rows); the second route also sums in numpy's own order.", "",
          f"## 4. the seen-list build: W = {W}, {W} remembered items per session", "",
          "| k | with lists wall ms | include_seen wall ms | build = difference ms | with lists kernels ms | include_seen kernels ms | expected keys |",
          "|---|---|---|---|---|---|---|"]
    for k in KS:
        r = last["seen"][f"k{k}"]
        L.append(f"| {k} | {r['with_lists']['wall_ms']:.1f} | {r['include_seen']['wall_ms']:.1f} | {r['build_wall_ms']:.1f} | "
                 f"{r['with_lists']['kernels_ms']:.2f} | {r['include_seen']['kernels_ms']:.2f} | {r['expected_keys']:.0f} |")
    L.append("")
    print("\n".join(L), flush=True)
    with open(out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    with open(out + ".md", "w") as fh:
        fh.write("\n".join(L))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
