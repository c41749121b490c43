"""Times recommend_sampled at catalogue scale: 8 192 users x 1M items, d = 128, k = 10 and 100, T = 0.25, 1 and 4, untrained model,
one process per measurement run.

    python tools/time_sampled.py --parent-tree DIR [--rounds 3] [--out profiles/sampled_8192x1M_d128]     (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child ...`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. recommend_reps, parent tree and this tree ALTERNATING, `--rounds` processes each: the unsampled instantiation must not have
     slowed (the project's noise floor is 3 %);
  2. recommend_sampled_reps of the same rows at every (k, T), in the same process as a recommend_reps measurement of this tree: the
     cost of the noise;
  3. the share of the scanned scores that reach the hash (stage 2) and the logarithms (stage 3) of topk_gemm_kernel's GumbelBias
     policy, from a HOST REPLAY of one workgroup — 128 users x one item range, tile by tile, with the kernel's staging and merge
     policy (a user's threshold moves only when a staging buffer of the workgroup overflows) — over numpy scores (f32 matmul: not
     the device's bits, the same distribution) and the contract's noise (tests/sampled_expect.py).  Nothing is counted on the device;
  4. the host route it replaces, on HOST_USERS users: predict over the whole catalogue per user, then numpy (Gumbel noise from
     numpy's generator, argpartition, sort).

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
KS = (10, 100)
TEMPS = (0.25, 1.0, 4.0)
REPS = 5
HOST_USERS = 128
REPLAY_RANGES = (0, 7, 15)  # item ranges of the 16 the scan splits 1M items into for 64 user tiles


def replay_shares(np, reps, E, b, ids, k, temp, seed, streams):
    """One workgroup's pass over the items `ids` (one range) for its 128 users: (scores scanned, scores hashed, noises evaluated)."""
    from sampled_expect import gumbel_of_r, hash_r, inv_temperature, row_keys

    inv_t = inv_temperature(temp)
    t = ((reps @ E.T + b[None, :]).astype(np.float32) * inv_t).astype(np.float32)
    k0, k1 = row_keys(seed, streams)
    r = hash_r(k0[:, None], k1[:, None], ids[None, :])
    table = gumbel_of_r((np.arange(1024, dtype=np.uint32) + np.uint32(1)) * np.uint32(1 << 13) - np.uint32(1))
    ub1 = t + table[1023]
    ub2 = t + table[r >> np.uint32(13)]
    key = t + gumbel_of_r(r)
    nu, n = t.shape
    lists = [np.zeros(0, np.float32) for _ in range(nu)]
    thr = np.full(nu, -np.inf, np.float32)
    staged = [[] for _ in range(nu)]
    scanned = hashed = logged = 0
    for c0 in range(0, n, 32):
        cols = slice(c0, min(c0 + 32, n))
        scanned += nu * (cols.stop - cols.start)
        p1 = ub1[:, cols] > thr[:, None]
        hashed += int(p1.sum())
        p2 = p1 & (ub2[:, cols] > thr[:, None])
        logged += int(p2.sum())
        pend = p2
        while True:
            pend = pend & (key[:, cols] > thr[:, None])
            over = False
            for u in np.flatnonzero(pend.any(axis=1)):
                idx = np.flatnonzero(pend[u])
                room = 32 - len(staged[u])
                staged[u].extend(key[u, cols][idx[:room]].tolist())
                pend[u, idx[:room]] = False
                over |= idx.size > room
            if not over:
                break
            for u in range(nu):  # merge_staged(TK_STAGE): every user of the workgroup whose staging is full
                if len(staged[u]) >= 32:
                    lists[u] = np.sort(np.concatenate([lists[u], np.array(staged[u], np.float32)]))[::-1][:k]
                    staged[u] = []
                    if lists[u].size == k:
                        thr[u] = lists[u][-1]
    return scanned, hashed, logged


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
    res = {"recommend": {}}
    for k in KS:
        res["recommend"][f"k{k}"] = timed(lambda: m.recommend_reps(reps, k))
        print(f"recommend k={k}: {res['recommend'][f'k{k}']}", flush=True)
    if "--sampled" in argv:
        res["sampled"], res["shares"], res["host_route"] = {}, {}, {}
        for k in KS:
            for temp in TEMPS:
                key = f"k{k}_T{temp}"
                res["sampled"][key] = timed(lambda: m.recommend_sampled_reps(reps, k, temperature=temp, seed=11))
                print(f"sampled {key}: {res['sampled'][key]}", flush=True)
            a = m.recommend_sampled_reps(reps[:256], k, temperature=1.0, seed=11)
            b = m.recommend_sampled_reps(reps[:256], k, temperature=1.0, seed=11)
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
        # 3. the host replay of the bounds: user tile 0 over three of the scan's 16 ranges of 62 528 items
        per = ((I + 15) // 16 + 31) // 32 * 32
        for k in KS:
            for temp in TEMPS:
                tot = [0, 0, 0]
                for g in REPLAY_RANGES:
                    ids = np.arange(g * per, min((g + 1) * per, I), dtype=np.uint32)
                    got = replay_shares(np, reps[:128], m.get_param_rows(Param.ITEM_EMBEDDING, ids), bias[ids], ids, k, temp, 11,
                                        np.arange(128, dtype=np.uint64))
                    tot = [x + y for x, y in zip(tot, got)]
                res["shares"][f"k{k}_T{temp}"] = {"scanned": tot[0], "hashed": tot[1], "noise": tot[2], "hashed_share": tot[1] / tot[0],
                                                   "noise_share": tot[2] / tot[0]}
                print(f"shares k={k} T={temp}: {res['shares'][f'k{k}_T{temp}']}", flush=True)
        # 4. the host route: predict of the catalogue per user, numpy noise and selection
        all_items = np.arange(I, dtype=np.uint32)
        rng = np.random.default_rng(0)
        for k in KS:
            t_pred = t_np = 0.0
            for u in range(HOST_USERS):
                t0 = time.perf_counter()
                s = m.predict(reps[u], all_items)
                t1 = time.perf_counter()
                keys = s + rng.gumbel(size=I).astype(np.float32)
                top = np.argpartition(-keys, k)[:k]
                top = top[np.argsort(-keys[top])]
                t2 = time.perf_counter()
                t_pred += t1 - t0
                t_np += t2 - t1
            res["host_route"][f"k{k}"] = {"users": HOST_USERS, "predict_ms": t_pred * 1e3, "numpy_ms": t_np * 1e3}
            dev = timed(lambda: m.recommend_sampled_reps(reps[:HOST_USERS], k, temperature=1.0, seed=11), reps=3)
            res["host_route"][f"k{k}"]["recommend_sampled"] = dev
            print(f"host route k={k}: {res['host_route'][f'k{k}']}", flush=True)
    with open(_opt("--out"), "w") as fh:
        json.dump(res, fh, indent=1)


def run_child(tree, out, sampled=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--out", out] + (["--sampled"] if sampled else [])
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=900)  # a child that fails or hangs ends the whole run
    return json.load(open(out))


def driver():
    this_tree = os.path.abspath(os.path.join(HERE, ".."))
    parent_tree = os.path.abspath(_opt("--parent-tree"))
    rounds = int(_opt("--rounds", "3"))
    out = _opt("--out", os.path.join(this_tree, "profiles", "sampled_8192x1M_d128"))
    tmp = out + ".child.json"
    res = {"users": U, "items": I, "dim": D, "reps": REPS, "rounds": rounds, "parent": [], "change": []}
    for r in range(rounds):  # alternating: parent, change, parent, change, ...
        res["parent"].append(run_child(parent_tree, tmp)["recommend"])
        last = run_child(this_tree, tmp, sampled=(r == rounds - 1))
        res["change"].append(last["recommend"])
    os.remove(tmp)
    res["sampled_run"] = last
    med = lambda runs, k, what: sorted(x[f"k{k}"][what] for x in runs)[len(runs) // 2]  # noqa: E731
    L = [f"# recommend_sampled at {U} users x {I} items, d = {D}", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} repetitions after a warm-up call; wall = the whole",
         "call from Python.  Untrained model, representations = rows of the item table.", "",
         "## 1. recommend_reps: parent commit against this build", "",
         f"{rounds} processes of each build, alternating (parent, this build, parent, ...); every process's median, then the median of those.", "",
         "| k | parent kernels ms (each process) | this build kernels ms (each process) | parent median | this build median | this / parent | parent wall ms | this build wall ms |",
         "|---|---|---|---|---|---|---|---|"]
    for k in KS:
        p, c = med(res["parent"], k, "kernels_ms"), med(res["change"], k, "kernels_ms")
        L.append(f"| {k} | " + ", ".join(f"{x[f'k{k}']['kernels_ms']:.2f}" for x in res["parent"]) + " | "
                 + ", ".join(f"{x[f'k{k}']['kernels_ms']:.2f}" for x in res["change"])
                 + f" | {p:.2f} | {c:.2f} | {c / p:.4f} | {med(res['parent'], k, 'wall_ms'):.1f} | {med(res['change'], k, 'wall_ms'):.1f} |")
    L += ["", "## 2. recommend_sampled_reps against recommend_reps of the same rows (same process, this build)", "",
          "Six launches against two: the keys prologue, the scan, the merge, the pairs, their plain scores, the padding.", "",
          "| k | T | recommend kernels ms | sampled kernels ms | sampled / recommend | recommend wall ms | sampled wall ms | scores hashed (replay) | noises evaluated (replay) |",
          "|---|---|---|---|---|---|---|---|---|"]
    for k in KS:
        a = last["recommend"][f"k{k}"]
        for temp in TEMPS:
            b, s = last["sampled"][f"k{k}_T{temp}"], last["shares"][f"k{k}_T{temp}"]
            L.append(f"| {k} | {temp} | {a['kernels_ms']:.2f} | {b['kernels_ms']:.2f} | {b['kernels_ms'] / a['kernels_ms']:.3f} | {a['wall_ms']:.1f} | "
                     f"{b['wall_ms']:.1f} | {s['hashed_share'] * 100:.2f} % | {s['noise_share'] * 100:.2f} % |")
    L += ["", "The two shares are a host replay of one workgroup (user tile 0) over three of the scan's 16 item ranges with the kernel's staging and",
          "merge policy, on numpy scores and the contract's noise: of the scores scanned, those that pass the first bound and are hashed, and those",
          "that pass the second bound too and have their noise evaluated.", "",
          f"## 3. the host route it replaces, on {HOST_USERS} users", "",
          "predict over the whole catalogue per user, then numpy: Gumbel noise from numpy's generator, argpartition, a sort of the k.", "",
          "| k | predict ms | numpy ms | host route ms | recommend_sampled_reps kernels ms | wall ms |", "|---|---|---|---|---|---|"]
    for k in KS:
        h = last["host_route"][f"k{k}"]
        L.append(f"| {k} | {h['predict_ms']:.0f} | {h['numpy_ms']:.0f} | {h['predict_ms'] + h['numpy_ms']:.0f} | {h['recommend_sampled']['kernels_ms']:.2f} | "
                 f"{h['recommend_sampled']['wall_ms']:.1f} |")
    L.append("")
    print("\n".join(L), flush=True)
    with open(out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    with open(out + ".md", "w") as fh:
        fh.write("\n".join(L))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
