"""Times rollout and beam search within an item set at catalogue scale: 8 192 sessions x 1M items, d = 128, untrained LSTM, 10
steps, |S| in {1e4, 1e5, 1e6}, one process per measurement run.

    python tools/time_item_set_rollout.py --parent-tree DIR [--rounds 3] [--out profiles/item_set_rollout_8192x1M_d128]
    python tools/time_item_set_rollout.py --sweep [--out ...]    (the |S| sweep, added to OUT.json under "sweep")
    python tools/time_item_set_rollout.py --report [--out ...]   (the .md again from OUT.json)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child --tree T`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. the untouched calls — store.rollout (greedy), store.beam_search (W = 4), recommend_reps (k = 1, 10) and the set's
     recommend_reps (|S| = 1e5, k = 1) — parent tree and this tree ALTERNATING, `--rounds` processes each;
  2. in each of this tree's processes also the four workloads — greedy rollout, sampled rollout, rollout with log_prob, beam W = 4 —
     through the set of all 1e6 items against the same plain calls, alternating call by call;
  3. `--sweep`, this tree, one process: the four workloads through sets of 1e4, 1e5 and 1e6 items beside the set's own scans over
     the same rows in the same process — recommend_reps(k = 1) per rollout step, recommend_reps(k = W) + log_partition_reps over the
     n W rows per beam step, and the same form's own call (recommend_sampled_reps(k = 1), log_partition_reps) for the sampled and
     log_prob rollouts — and the route this replaces, the store's call with the complement of S as lists, at 128 sessions.

Kernel time = the engine's device events around the launches of a family (`rank`: SBR_K_RANK, the scan side; `fwd`:
SBR_K_RECURRENT_FWD, the cell steps), median of the repetitions after a warm-up call; wall time = the whole call from Python."""
import json
import os
import subprocess
import sys
import time

argv = sys.argv[1:]


def _opt(name, default=None):
    return argv[argv.index(name) + 1] if name in argv else default


HERE = os.path.dirname(os.path.abspath(__file__))
U, I, D, T, STEPS, W, HOST_U = 8192, 1_000_000, 128, 64, 10, 4, 128
SIZES = (10_000, 100_000, 1_000_000)
REPS = 5
UNTOUCHED = ("rollout_greedy", "beam_w4", "recommend_k1", "recommend_k10", "set_recommend_k1")
WORKLOADS = ("greedy", "sample", "log_prob", "beam_w4")


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
        rank, fwd, wall = [], [], []
        for _ in range(reps):
            m.timing_read()
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            led = m.timing_read()
            rank.append(led["RANK"][0])
            fwd.append(led["RECURRENT_FWD"][0])
        m.timing_enable(False)
        return {"rank_ms": float(np.median(rank)), "fwd_ms": float(np.median(fwd)), "wall_ms": float(np.median(wall))}

    m = Model(hparams(I, T, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
    m.set_param(Param.ITEM_BIAS, (np.random.RandomState(1).randn(I) * 0.1).astype(np.float32))
    rs = np.random.RandomState(4)
    slots = np.arange(U, dtype=np.uint32)
    store = m.sessions(U)
    store.append(slots, (np.arange(U + 1, dtype=np.uint64) * 8, rs.randint(0, I, U * 8).astype(np.uint32)))
    reps = store.representations(slots)
    res = {}

    def log(name):
        print(f"{name}: {res[name]}", flush=True)

    def workload(target, name, rows=slots, **kw):
        if name == "beam_w4":
            return lambda: target.beam_search(rows, STEPS, width=W, **kw)
        mode = {"greedy": dict(), "sample": dict(mode="sample"), "log_prob": dict(log_prob=True)}[name]
        return lambda: target.rollout(rows, STEPS, **mode, **kw)

    if "--untouched" in argv:
        s5 = m.item_set(item_set_of(np, 100_000))
        calls = {"rollout_greedy": lambda: store.rollout(slots, STEPS), "beam_w4": lambda: store.beam_search(slots, STEPS, width=W),
                 "recommend_k1": lambda: m.recommend_reps(reps, 1), "recommend_k10": lambda: m.recommend_reps(reps, 10),
                 "set_recommend_k1": lambda: s5.recommend_reps(reps, 1)}
        for name in UNTOUCHED:
            res[name] = timed(m, calls[name])
            log(name)
        s5.close()
    if "--all-set" in argv:  # the set of every item against the plain call, alternating call by call
        on = m.item_set(item_set_of(np, I)).on(store)
        for name in WORKLOADS:
            res[f"plain_{name}"] = timed(m, workload(store, name))
            res[f"all_{name}"] = timed(m, workload(on, name))
            log(f"plain_{name}")
            log(f"all_{name}")
        on.item_set.close()
    if "--sweep" in argv:
        wide = np.ascontiguousarray(np.repeat(reps, W, axis=0))
        hs = slots[:HOST_U]
        for n in SIZES:
            S = item_set_of(np, n)
            s = m.item_set(S)
            on = s.on(store)
            for name in WORKLOADS:
                res[f"set{n}_{name}"] = timed(m, workload(on, name))
                log(f"set{n}_{name}")
            res[f"set{n}_scan_k1"] = timed(m, lambda: s.recommend_reps(reps, 1))
            res[f"set{n}_sampled_k1"] = timed(m, lambda: s.recommend_sampled_reps(reps, 1))
            res[f"set{n}_partition_k1"] = timed(m, lambda: s.log_partition_reps(reps))
            res[f"set{n}_scan_k{W}_nw"] = timed(m, lambda: s.recommend_reps(wide, W))
            res[f"set{n}_partition_nw"] = timed(m, lambda: s.log_partition_reps(wide))
            for k in (f"set{n}_scan_k1", f"set{n}_sampled_k1", f"set{n}_partition_k1", f"set{n}_scan_k{W}_nw", f"set{n}_partition_nw"):
                log(k)
            # the route this replaces: the complement as every row's list, at 128 sessions
            res[f"set{n}_host_u_set_greedy"] = timed(m, workload(on, "greedy", rows=hs), reps=3)
            res[f"set{n}_host_u_set_beam_w4"] = timed(m, workload(on, "beam_w4", rows=hs), reps=3)
            comp = np.setdiff1d(np.arange(I, dtype=np.uint32), S).astype(np.uint32)
            lists = [comp] * HOST_U
            for name in ("greedy", "beam_w4"):
                key = f"set{n}_host_u_lists_{name}"
                try:
                    res[key] = timed(m, workload(store, name, rows=hs, exclude=lists), reps=3)
                except Exception as e:  # noqa: BLE001 — recorded, not hidden: the route may not fit
                    res[key] = {"error": f"{type(e).__name__}: {e}"}
            for k in (f"set{n}_host_u_set_greedy", f"set{n}_host_u_lists_greedy", f"set{n}_host_u_set_beam_w4", f"set{n}_host_u_lists_beam_w4"):
                log(k)
            s.close()
        # the same picks both ways, once, at 128 sessions and |S| = 1e4
        S = item_set_of(np, SIZES[0])
        s = m.item_set(S)
        comp = np.setdiff1d(np.arange(I, dtype=np.uint32), S).astype(np.uint32)
        a = s.on(store).rollout(hs, STEPS)
        b = store.rollout(hs, STEPS, exclude=[comp] * HOST_U)
        assert np.array_equal(a.items, b.items) and np.array_equal(a.scores.view(np.uint32), b.scores.view(np.uint32)), "set != lists"
        s.close()
    with open(_opt("--json"), "w") as f:
        json.dump(res, f)


def _child(tree, path, *flags):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--json", path, *flags]
    subprocess.run(cmd, check=True, timeout=900)
    out = json.load(open(path))
    os.remove(path)
    return out


def _load(out):
    return json.load(open(out + ".json")) if os.path.exists(out + ".json") else {}


def report(out):
    data = _load(out)
    runs = data if "parent" in data else None
    sweep = data.get("sweep")
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    k = lambda x: x["rank_ms"] + x["fwd_ms"]  # noqa: E731
    lines = [f"# rollout and beam search within an item set: {U} sessions x {I} items, d = {D}, untrained LSTM, {STEPS} steps", "",
             "Written by `tools/time_item_set_rollout.py`; every figure is a median in milliseconds.  `rank` = kernel time of the scan",
             "side (SBR_K_RANK), `fwd` = kernel time of the cell steps (SBR_K_RECURRENT_FWD), `wall` = the call from Python.", ""]
    if runs:
        rounds = len(runs["parent"])
        lines += ["## The untouched calls, parent against this tree", "",
                  f"{rounds} alternating processes each; the median over the processes of each process's median kernel time (rank + fwd),",
                  "and the parent's own spread (min .. max over its processes).", "",
                  "| call | parent kernels | parent spread | this kernels | ratio | within spread | parent wall | this wall |",
                  "|---|---|---|---|---|---|---|---|"]
        for name in UNTOUCHED:
            kp = [k(x[name]) for x in runs["parent"]]
            kt = [k(x[name]) for x in runs["this"]]
            inside = min(kp) <= med(kt) <= max(kp)
            lines.append(f"| {name} | {med(kp):.3f} | {min(kp):.3f} .. {max(kp):.3f} | {med(kt):.3f} | {med(kt) / med(kp):.4f} | "
                         f"{'yes' if inside else 'no'} | {med([x[name]['wall_ms'] for x in runs['parent']]):.1f} | "
                         f"{med([x[name]['wall_ms'] for x in runs['this']]):.1f} |")
        lines += ["", "## The set of all 1e6 items against the plain call, this tree", "",
                  f"The same {rounds} processes, the two calls alternating within each; the plain call's spread is min .. max of its",
                  "per-process medians.  The set path adds subset_positions_kernel (only where there are lists), the tag words' gather",
                  "(only with masks) and the id mapping in the advance / select kernels.", "",
                  "| workload | plain kernels | plain spread | set kernels | ratio | within spread | plain wall | set wall |",
                  "|---|---|---|---|---|---|---|---|"]
        for name in WORKLOADS:
            kp = [k(x[f"plain_{name}"]) for x in runs["this"]]
            ks = [k(x[f"all_{name}"]) for x in runs["this"]]
            inside = min(kp) <= med(ks) <= max(kp)
            lines.append(f"| {name} | {med(kp):.2f} | {min(kp):.2f} .. {max(kp):.2f} | {med(ks):.2f} | {med(ks) / med(kp):.4f} | "
                         f"{'yes' if inside else 'no'} | {med([x[f'plain_{name}']['wall_ms'] for x in runs['this']]):.1f} | "
                         f"{med([x[f'all_{name}']['wall_ms'] for x in runs['this']]):.1f} |")
        lines.append("")
    if sweep:
        lines += ["## Through sets of 1e4, 1e5 and 1e6 items, this tree, one process", "",
                  "`per step` = rank / steps.  `own scans` = what the set's own calls cost over the same rows in the same process:",
                  f"recommend_reps(k = 1) over the {U} rows (rollout), recommend_reps(k = {W}) + log_partition_reps over the {U} x {W}",
                  "beam rows (beam).  `share` = (per step - own scans) / per step: for greedy the advance kernel and the segments; a",
                  "sampled step runs the sampled scan and a log_prob step the partition's two scans, which a k = 1 scan does not, so",
                  "`same form` compares them with the set's recommend_sampled_reps(k = 1) and log_partition_reps; a beam step after the",
                  "first scans the n W rows but takes its shift from the scan's first column, so it runs one scan fewer than the sum.", "",
                  "| |S| | workload | rank | fwd | wall | per step | own scans | share | same form | share |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        same_form = {"sample": "sampled_k1", "log_prob": "partition_k1"}
        for n in SIZES:
            for name in WORKLOADS:
                x = sweep[f"set{n}_{name}"]
                per = x["rank_ms"] / STEPS
                own = (sweep[f"set{n}_scan_k{W}_nw"]["rank_ms"] + sweep[f"set{n}_partition_nw"]["rank_ms"] if name == "beam_w4"
                       else sweep[f"set{n}_scan_k1"]["rank_ms"])
                form = sweep.get(f"set{n}_{same_form[name]}") if name in same_form else None
                tail = f"{form['rank_ms']:.3f} | {(per - form['rank_ms']) / per:+.4f} |" if form else "| |"
                lines.append(f"| {n:.0e} | {name} | {x['rank_ms']:.2f} | {x['fwd_ms']:.2f} | {x['wall_ms']:.1f} | {per:.3f} | {own:.3f} | "
                             f"{(per - own) / per:+.4f} | {tail}")
        lines += ["", f"## The route this replaces, at {HOST_U} sessions", "",
                  "The store's own call with the complement of S as every row's list (what was needed before) against the call through",
                  f"the set, wall time.  {U} sessions do not fit in host memory by the list route at |S| = 1e4 (8 192 lists of 990 000 ids).", "",
                  "| |S| | workload | lists: rank | lists: wall | set: rank | set: wall |", "|---|---|---|---|---|---|"]
        for n in SIZES:
            for name in ("greedy", "beam_w4"):
                a, b = sweep[f"set{n}_host_u_lists_{name}"], sweep[f"set{n}_host_u_set_{name}"]
                if "error" in a:
                    lines.append(f"| {n:.0e} | {name} | {a['error']} | | {b['rank_ms']:.2f} | {b['wall_ms']:.1f} |")
                else:
                    lines.append(f"| {n:.0e} | {name} | {a['rank_ms']:.2f} | {a['wall_ms']:.1f} | {b['rank_ms']:.2f} | {b['wall_ms']:.1f} |")
        lines.append("")
    open(out + ".md", "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def driver():
    here = os.path.dirname(HERE)
    out = _opt("--out", os.path.join(here, "profiles", "item_set_rollout_8192x1M_d128"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if "--report" in argv:
        return report(out)
    if "--sweep" in argv:
        sweep = _child(here, out + ".sweep.tmp.json", "--sweep")
        data = _load(out)
        data["sweep"] = sweep
        json.dump(data, open(out + ".json", "w"), indent=1)
        return report(out)
    parent = os.path.abspath(_opt("--parent-tree"))
    rounds = int(_opt("--rounds", "3"))
    runs = _load(out)
    runs["parent"], runs["this"] = [], []
    for r in range(rounds):
        runs["parent"].append(_child(parent, f"{out}.parent{r}.tmp.json", "--untouched"))
        runs["this"].append(_child(here, f"{out}.this{r}.tmp.json", "--untouched", "--all-set"))
    json.dump(runs, open(out + ".json", "w"), indent=1)
    report(out)


if __name__ == "__main__":
    child() if "--child" in argv else driver()
