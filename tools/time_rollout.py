"""Times Sessions.rollout at catalogue scale: 8 192 sessions x 1M items, d = 128, LSTM, steps = 10, untrained model, one process per
measurement run.

    python tools/time_rollout.py --parent-tree DIR [--rounds 3] [--out profiles/rollout_8192x1M_d128]   (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child --tree T`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. the untouched calls — recommend_reps (k = 1, 10), store.recommend (k = 1), a one-item append of every slot and
     log_partition_reps — and the host loop a rollout replaces (recommend(k = 1) + append + a rebuilt exclude, 10 steps, written
     against the parent's API), parent tree and this tree ALTERNATING, `--rounds` processes each;
  2. this tree only, in the last of its processes: rollout greedy, greedy with log_prob, and sampled — kernel time by family (the
     scan side, SBR_K_RANK: the k = 1 scan, the partition, the sampled epilogue and rollout_advance_kernel; the state side,
     SBR_K_RECURRENT_FWD: the cell step and the ended rows' carry) and wall time — beside the expectation measured in the same
     process: steps x (one recommend_reps(k = 1) scan + one one-item append [+ one log_partition_reps]).

Kernel time = the engine's device events around the launches of a family, median of the repetitions after a warm-up call; wall
time = the whole call from Python.  The host loop's wall time is split by timing its three parts separately: the two device calls
(with their round trips) and the rebuild of the exclusion lists on the host."""
import json
import os
import subprocess
import sys
import time

argv = sys.argv[1:]


def _opt(name, default=None):
    return argv[argv.index(name) + 1] if name in argv else default


HERE = os.path.dirname(os.path.abspath(__file__))
U, I, D, T, STEPS = 8192, 1_000_000, 128, 64, 10
REPS = 5
UNTOUCHED = ("recommend_k1", "recommend_k10", "store_recommend_k1", "append_one", "log_partition")


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
    store = m.sessions(U)

    def restart():
        store.reset()
        store.append(slots, (hist_ptr, hist))

    restart()
    reps = store.representations(slots)
    one_ptr = np.arange(U + 1, dtype=np.uint64)
    one = rs.randint(0, I, U).astype(np.uint32)
    res = {}
    calls = {"recommend_k1": lambda: m.recommend_reps(reps, 1), "recommend_k10": lambda: m.recommend_reps(reps, 10),
             "store_recommend_k1": lambda: store.recommend(slots, 1), "append_one": lambda: store.append(slots, (one_ptr, one)),
             "log_partition": lambda: m.log_partition_reps(reps)}
    for name in UNTOUCHED:
        res[name] = timed(m, calls[name])
        print(f"{name}: {res[name]}", flush=True)

    parts = {"recommend": 0.0, "append": 0.0, "rebuild": 0.0}

    def host_loop():
        lists = [[] for _ in range(U)]
        for j in range(STEPS):
            t0 = time.perf_counter()
            it, _ = store.recommend(slots, 1, exclude=lists if j else None)
            t1 = time.perf_counter()
            store.append(slots, (one_ptr, np.ascontiguousarray(it[:, 0])))
            t2 = time.perf_counter()
            for i in range(U):  # the rebuilt exclusion lists, growing by one entry per row
                lists[i].append(int(it[i, 0]))
            t3 = time.perf_counter()
            parts["recommend"] += (t1 - t0) * 1e3
            parts["append"] += (t2 - t1) * 1e3
            parts["rebuild"] += (t3 - t2) * 1e3
        return lists

    res["host_loop"] = timed(m, host_loop, reps=3, before=restart)
    n = 4.0  # the warm-up call and three repetitions
    res["host_loop"]["parts_ms"] = {k: v / n for k, v in parts.items()}
    print(f"host_loop: {res['host_loop']}", flush=True)
    if "--rollout" in argv:
        restart()
        want = np.array(host_loop())
        restart()
        r = store.rollout(slots, STEPS)
        assert np.array_equal(r.items, want), "the rollout is not the host loop"
        for name, kw in (("rollout_greedy", {}), ("rollout_greedy_log_prob", {"log_prob": True}),
                         ("rollout_sample", {"mode": "sample", "seed": 3}), ("rollout_greedy_final_state", {"final_state": True})):
            res[name] = timed(m, lambda: store.rollout(slots, STEPS, **kw))
            print(f"{name}: {res[name]}", flush=True)
    with open(_opt("--json"), "w") as f:
        json.dump(res, f)


def driver():
    parent = os.path.abspath(_opt("--parent-tree"))
    here = os.path.dirname(HERE)
    rounds = int(_opt("--rounds", "3"))
    out = _opt("--out", os.path.join(here, "profiles", "rollout_8192x1M_d128"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    runs = {"parent": [], "this": []}
    for r in range(rounds):
        for which, tree in (("parent", parent), ("this", here)):
            path = f"{out}.{which}{r}.tmp.json"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--json", path]
            if which == "this" and r == rounds - 1:
                cmd.append("--rollout")
            subprocess.run(cmd, check=True, timeout=900)
            runs[which].append(json.load(open(path)))
            os.remove(path)
    json.dump(runs, open(out + ".json", "w"), indent=1)
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    last = runs["this"][-1]
    lines = [f"# rollout: {U} sessions x {I} items, d = {D}, LSTM, steps = {STEPS}", "",
             "Written by `tools/time_rollout.py`; every figure is a median in milliseconds.  `rank` = kernel time of the scan side",
             "(SBR_K_RANK), `fwd` = kernel time of the state side (SBR_K_RECURRENT_FWD), `wall` = the call from Python.", "",
             "## The untouched calls and the host loop, parent against this tree", "",
             f"{rounds} alternating processes each; the median over the processes of each process's median.", "",
             "| call | parent rank | this rank | ratio | parent fwd | this fwd | parent wall | this wall |", "|---|---|---|---|---|---|---|---|"]
    for name in UNTOUCHED + ("host_loop",):
        p = {k: med([x[name][k] for x in runs["parent"]]) for k in ("rank_ms", "fwd_ms", "wall_ms")}
        t = {k: med([x[name][k] for x in runs["this"]]) for k in ("rank_ms", "fwd_ms", "wall_ms")}
        kp, kt = p["rank_ms"] + p["fwd_ms"], t["rank_ms"] + t["fwd_ms"]
        lines.append(f"| {name} | {p['rank_ms']:.3f} | {t['rank_ms']:.3f} | {kt / kp if kp else float('nan'):.4f} | {p['fwd_ms']:.3f} | "
                     f"{t['fwd_ms']:.3f} | {p['wall_ms']:.1f} | {t['wall_ms']:.1f} |")
    hp = {k: med([x["host_loop"]["parts_ms"][k] for x in runs["parent"]]) for k in ("recommend", "append", "rebuild")}
    lines += ["", f"The parent's host loop, wall time by part: recommend {hp['recommend']:.1f}, append {hp['append']:.1f}, "
              f"rebuild of the lists on the host {hp['rebuild']:.1f}.", ""]
    if "rollout_greedy" in last:
        exp = STEPS * (last["recommend_k1"]["rank_ms"] + last["append_one"]["fwd_ms"])
        lines += ["## The rollout, this tree, one process", "",
                  f"Expectation from the same process: {STEPS} x (recommend_reps(k = 1) {last['recommend_k1']['rank_ms']:.3f} + one-item append "
                  f"{last['append_one']['fwd_ms']:.3f}) = {exp:.2f} ms of kernels; greedy with the partition, whose own k = 1 scan is the pick: "
                  f"{STEPS} x (log_partition_reps {last['log_partition']['rank_ms']:.3f} + the append) = "
                  f"{STEPS * (last['log_partition']['rank_ms'] + last['append_one']['fwd_ms']):.2f}.", "",
                  "| call | rank | fwd | rank per step | fwd per step | wall |", "|---|---|---|---|---|---|"]
        for name in ("rollout_greedy", "rollout_greedy_log_prob", "rollout_sample", "rollout_greedy_final_state"):
            x = last[name]
            lines.append(f"| {name} | {x['rank_ms']:.3f} | {x['fwd_ms']:.3f} | {x['rank_ms'] / STEPS:.3f} | {x['fwd_ms'] / STEPS:.3f} | {x['wall_ms']:.1f} |")
        lines += ["", f"Wall time: rollout {last['rollout_greedy']['wall_ms']:.1f} against the host loop's "
                  f"{med([x['host_loop']['wall_ms'] for x in runs['parent']]):.1f} on the parent's library.", ""]
    open(out + ".md", "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
