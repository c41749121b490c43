"""Times Sessions.beam_search at catalogue scale: 8 192 sessions x 1M items, d = 128, LSTM, steps = 10, W in {1, 4, 8}, untrained
model, one process per measurement run.

    python tools/time_beam.py --parent-tree DIR [--rounds 3] [--out profiles/beam_8192x1M_d128]   (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child --tree T`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. the untouched calls — rollout greedy, recommend_reps (k = 1, 10), log_partition_reps and a one-item append of every slot — parent
     tree and this tree ALTERNATING, `--rounds` processes each; in the parent's first process also the host loop a beam search
     replaces, written against the parent's API, at 128 sessions: per step W temporary slots per row filled by state / set_state,
     append of the picks, recommend(k = W) and log_partition over the beams' rebuilt exclusion lists, the selection in numpy;
  2. this tree only, in the last of its processes: beam_search at each W — kernel time by family (the scan side, SBR_K_RANK: the
     k = W scan, the partition sum, beam_select_kernel, beam_segments_kernel and beam_backtrack_kernel; the state side,
     SBR_K_RECURRENT_FWD: the cell step with the carry, or the gather) and wall time — beside what the same process measures for
     recommend_reps(k = W) + log_partition_reps over the n W beam rows, and W = 1 beside rollout(log_prob=True); the beam call at 128
     sessions for the host loop's comparison.

Kernel time = the engine's device events around the launches of a family, median of the repetitions after a warm-up call; wall
time = the whole call from Python."""
import json
import os
import subprocess
import sys
import time

argv = sys.argv[1:]


def _opt(name, default=None):
    return argv[argv.index(name) + 1] if name in argv else default


HERE = os.path.dirname(os.path.abspath(__file__))
U, I, D, T, STEPS, WIDTHS, HOST_U = 8192, 1_000_000, 128, 64, 10, (1, 4, 8), 128
REPS = 5
UNTOUCHED = ("rollout_greedy", "recommend_k1", "recommend_k10", "log_partition", "append_one")


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

    def timed(m, fn, reps=REPS, before=None):
        if before:
            before()
        fn()
        m.timing_enable(True)
        rank, fwd, wall = [], [], []
        for _ in range(reps):
            if before:
                before()
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
    hist_ptr = np.arange(U + 1, dtype=np.uint64) * 8
    hist = rs.randint(0, I, U * 8).astype(np.uint32)
    store = m.sessions(U + HOST_U * max(WIDTHS))

    def restart():
        store.reset()
        store.append(slots, (hist_ptr, hist))

    restart()
    reps = store.representations(slots)
    one_ptr = np.arange(U + 1, dtype=np.uint64)
    one = rs.randint(0, I, U).astype(np.uint32)
    res = {}
    calls = {"rollout_greedy": lambda: store.rollout(slots, STEPS), "recommend_k1": lambda: m.recommend_reps(reps, 1),
             "recommend_k10": lambda: m.recommend_reps(reps, 10), "log_partition": lambda: m.log_partition_reps(reps),
             "append_one": lambda: store.append(slots, (one_ptr, one))}
    for name in UNTOUCHED:
        res[name] = timed(m, calls[name], before=restart if name == "append_one" else None)
        print(f"{name}: {res[name]}", flush=True)
    restart()

    hs = slots[:HOST_U]

    def host_loop(w, temperature=1.0):
        """What a caller does without the beam call, on the parent's API: the beams live in W temporary slots per row."""
        n = hs.size
        tmp = (U + np.arange(n * w)).astype(np.uint32)
        inv_t = np.float32(1.0) / np.float32(temperature)
        paths = [[] for _ in range(n)]
        cum = np.zeros(n, np.float32)
        cur, per = hs, 1
        for j in range(STEPS):
            lists = [sorted(p) for p in paths]
            it, sc = store.recommend(cur, w, exclude=lists)
            part = store.log_partition(cur, temperature, exclude=lists)
            fb = part.frac_bits
            L = np.log((part.mass.astype(np.float64) / 2.0 ** fb)).astype(np.float32)
            lp = (sc * inv_t - part.shift[:, None]) - L[:, None]
            tot = (cum[:, None] + lp).reshape(n, per * w)
            tot[(it == 0xFFFFFFFF).reshape(n, per * w)] = -np.inf
            pick = np.argsort(-tot, axis=1, kind="stable")[:, :w]
            parent = (np.arange(n)[:, None] * per + pick // w).ravel()
            item = it.reshape(n, per * w)[np.arange(n)[:, None], pick].ravel()
            cum = tot[np.arange(n)[:, None], pick].ravel()
            src, which = np.unique(cur[parent], return_inverse=True)  # a call names a slot once
            h, c, ln = store.state(src)
            store.set_state(tmp, h[which], None if c is None else c[which], ln[which])
            store.append(tmp, (np.arange(n * w + 1, dtype=np.uint64), np.where(item == 0xFFFFFFFF, 0, item).astype(np.uint32)))
            paths = [paths[p] + [int(x)] for p, x in zip(parent, item)]
            cur, per = tmp, w
        return paths

    if "--host-loop" in argv:
        for w in WIDTHS:
            res[f"host_loop_w{w}"] = timed(m, lambda: host_loop(w), reps=3)
            print(f"host_loop_w{w}: {res[f'host_loop_w{w}']}", flush=True)
    if "--beam" in argv:
        for w in WIDTHS:
            wide = np.ascontiguousarray(np.repeat(reps, w, axis=0))
            res[f"scan_k{w}_nw"] = timed(m, lambda: m.recommend_reps(wide, w))
            res[f"partition_nw{w}"] = timed(m, lambda: m.log_partition_reps(wide))
            res[f"beam_w{w}"] = timed(m, lambda: store.beam_search(slots, STEPS, width=w))
            res[f"beam_w{w}_host_u"] = timed(m, lambda: store.beam_search(hs, STEPS, width=w))
            for k in (f"scan_k{w}_nw", f"partition_nw{w}", f"beam_w{w}", f"beam_w{w}_host_u"):
                print(f"{k}: {res[k]}", flush=True)
            del wide
        res["rollout_log_prob"] = timed(m, lambda: store.rollout(slots, STEPS, log_prob=True))
        print(f"rollout_log_prob: {res['rollout_log_prob']}", flush=True)
        one_beam = store.beam_search(slots, STEPS, width=1)
        assert np.array_equal(one_beam.items[:, 0], store.rollout(slots, STEPS).items), "W = 1 is not greedy rollout"
    with open(_opt("--json"), "w") as f:
        json.dump(res, f)


def driver():
    parent = os.path.abspath(_opt("--parent-tree"))
    here = os.path.dirname(HERE)
    rounds = int(_opt("--rounds", "3"))
    out = _opt("--out", os.path.join(here, "profiles", "beam_8192x1M_d128"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    runs = {"parent": [], "this": []}
    for r in range(rounds):
        for which, tree in (("parent", parent), ("this", here)):
            path = f"{out}.{which}{r}.tmp.json"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--json", path]
            if which == "parent" and r == 0:
                cmd.append("--host-loop")
            if which == "this" and r == rounds - 1:
                cmd.append("--beam")
            subprocess.run(cmd, check=True, timeout=1100)
            runs[which].append(json.load(open(path)))
            os.remove(path)
    json.dump(runs, open(out + ".json", "w"), indent=1)
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    last = runs["this"][-1]
    lines = [f"# beam_search: {U} sessions x {I} items, d = {D}, LSTM, steps = {STEPS}, W in {WIDTHS}", "",
             "Written by `tools/time_beam.py`; every figure is a median in milliseconds.  `rank` = kernel time of the scan side",
             "(SBR_K_RANK), `fwd` = kernel time of the state side (SBR_K_RECURRENT_FWD), `wall` = the call from Python.", "",
             "## The untouched calls, parent against this tree", "",
             f"{rounds} alternating processes each; the median over the processes of each process's median, and the parent's own",
             "spread (min .. max over its processes) of rank + fwd.", "",
             "| call | parent kernels | parent spread | this kernels | ratio | parent wall | this wall |", "|---|---|---|---|---|---|---|"]
    for name in UNTOUCHED:
        kp = [x[name]["rank_ms"] + x[name]["fwd_ms"] for x in runs["parent"]]
        kt = [x[name]["rank_ms"] + x[name]["fwd_ms"] for x in runs["this"]]
        lines.append(f"| {name} | {med(kp):.3f} | {min(kp):.3f} .. {max(kp):.3f} | {med(kt):.3f} | {med(kt) / med(kp):.4f} | "
                     f"{med([x[name]['wall_ms'] for x in runs['parent']]):.1f} | {med([x[name]['wall_ms'] for x in runs['this']]):.1f} |")
    if "beam_w1" in last:
        lines += ["", "## beam_search, this tree, one process", "",
                  "`scan side per step` = rank / steps; `sum` = recommend_reps(k = W) + log_partition_reps over the n W beam rows (n rows",
                  "with W copies each), measured in the same process; their ratio should be below 1 by about one k = 1 scan, the",
                  "partition's pre-scan the beam call does not run.  Steps after the first scan n W rows; the first scans n.", "",
                  "| W | rank | fwd | wall | scan side per step | sum | ratio | rest per step (rank/steps - sum) |", "|---|---|---|---|---|---|---|---|"]
        for w in WIDTHS:
            b = last[f"beam_w{w}"]
            s = last[f"scan_k{w}_nw"]["rank_ms"] + last[f"partition_nw{w}"]["rank_ms"]
            per = b["rank_ms"] / STEPS
            lines.append(f"| {w} | {b['rank_ms']:.2f} | {b['fwd_ms']:.2f} | {b['wall_ms']:.1f} | {per:.3f} | {s:.3f} | {per / s:.4f} | "
                         f"{per - s:.3f} |")
        r1 = last["rollout_log_prob"]
        lines += ["", f"W = 1 against rollout(log_prob=True) in the same process: rank {last['beam_w1']['rank_ms']:.2f} vs "
                  f"{r1['rank_ms']:.2f}, fwd {last['beam_w1']['fwd_ms']:.2f} vs {r1['fwd_ms']:.2f}, wall {last['beam_w1']['wall_ms']:.1f} vs "
                  f"{r1['wall_ms']:.1f}.", ""]
    hl = runs["parent"][0]
    if "host_loop_w1" in hl and "beam_w1_host_u" in last:
        lines += ["## The host loop it replaces, at 128 sessions", "",
                  "The parent's library, its own process: per step state / set_state of W temporary slots per row, append, recommend(k = W),",
                  "log_partition, the selection in numpy.  This tree: beam_search over the same 128 slots.", "",
                  "| W | host loop wall | beam_search wall |", "|---|---|---|"]
        for w in WIDTHS:
            lines.append(f"| {w} | {hl[f'host_loop_w{w}']['wall_ms']:.1f} | {last[f'beam_w{w}_host_u']['wall_ms']:.1f} |")
        lines.append("")
    open(out + ".md", "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
