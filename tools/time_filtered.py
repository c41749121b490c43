"""Times the tag filter of the top-k scan at catalogue scale: 8 192 users x 1M items, d = 128, k = 10 and 100, untrained model, one
process per measurement run.

    python tools/time_filtered.py --parent-tree DIR [--rounds 3] [--out profiles/filtered_8192x1M_d128]     (writes .json and .md)

DIR is a checkout of the parent commit with its library built (python -m sbr_rs_amd.build there).  The driver starts child
processes of this file (`--child ...`), each of which loads the package of ONE tree, and stops at the first child that fails:

  1. recommend_reps unfiltered, parent tree and this tree ALTERNATING, `--rounds` processes each: the unfiltered instantiation must
     not have slowed (the project's noise floor is 3 %);
  2. recommend_reps with all-pass masks (any_of = none_of = 0) in the same process as an unfiltered measurement of this tree:
     the filter's overhead;
  3. masks that pass about 50 %, 10 % and 1 % of the catalogue (one tag bit each, set with that probability);
  4. the exclusion-list equivalent of 3 — recommend_reps with every disallowed item in the user's list — on EXCL_USERS users beside
     the filtered call on the same users: at 8 192 users the lists are 8 192 x up to 990 000 ids x 4 bytes = 15-30 GiB on the host
     (and again on the device), so the full shape is not run.

Kernel time = the engine's device events around the launches of the SBR_K_RANK family, median of REPS repetitions after a warm-up
call (the exclusion-list calls of 4: one call each); wall time = the whole call from Python."""
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
REPS = 5
EXCL_USERS = 128
PASS = {"50%": (0, 0.5), "10%": (1, 0.1), "1%": (2, 0.01)}  # name -> (tag bit, probability that an item has it)


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

    last = [None]  # what the last timed call returned

    def timed(fn, reps=REPS, warm=True):
        if warm:
            fn()
        m.timing_enable(True)
        kern, wall = [], []
        for _ in range(reps):
            m.timing_read()
            t0 = time.perf_counter()
            last[0] = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(m.timing_read()["RANK"][0])
        m.timing_enable(False)
        return {"kernels_ms": float(np.median(kern)), "wall_ms": float(np.median(wall)), "kernels_all_ms": [float(x) for x in kern]}

    m = Model(hparams(I, T, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
    m.set_param(Param.ITEM_BIAS, (np.random.RandomState(1).randn(I) * 0.1).astype(np.float32))
    reps = m.get_param_rows(Param.ITEM_EMBEDDING, np.random.RandomState(9).randint(0, I, U).astype(np.uint32))
    res = {"unfiltered": {}}
    for k in KS:
        res["unfiltered"][f"k{k}"] = timed(lambda: m.recommend_reps(reps, k))
        print(f"unfiltered k={k}: {res['unfiltered'][f'k{k}']}", flush=True)
    if "--filtered" in argv:
        rs = np.random.RandomState(3)
        tags = np.zeros(I, np.uint32)
        for bit, p in PASS.values():
            tags |= (rs.rand(I) < p).astype(np.uint32) << np.uint32(bit)
        m.set_item_tags(tags)
        res["all_pass"], res["pass"], res["exclusion"] = {}, {}, {}
        for k in KS:
            res["all_pass"][f"k{k}"] = timed(lambda: m.recommend_reps(reps, k, any_of=0, none_of=0))
            print(f"all-pass k={k}: {res['all_pass'][f'k{k}']}", flush=True)
            plain = m.recommend_reps(reps[:512], k)
            same = m.recommend_reps(reps[:512], k, any_of=0, none_of=0)
            assert np.array_equal(plain[0], same[0]) and np.array_equal(plain[1].view(np.uint32), same[1].view(np.uint32))
        for name, (bit, _) in PASS.items():
            mask = 1 << bit
            outside = np.flatnonzero((tags & np.uint32(mask)) == 0).astype(np.uint32)
            frac = 1.0 - outside.size / I
            excl = [outside] * EXCL_USERS
            for k in KS:
                key = f"{name}_k{k}"
                res["pass"][key] = dict(timed(lambda: m.recommend_reps(reps, k, any_of=mask)), passing=frac)
                small = timed(lambda: m.recommend_reps(reps[:EXCL_USERS], k, any_of=mask), reps=3)
                got = last[0]
                # one call, not warmed: the host sorts and uploads 128 lists of up to 990 000 ids in every call
                lists = timed(lambda: m.recommend_reps(reps[:EXCL_USERS], k, exclude=excl), reps=1, warm=(name == "50%" and k == KS[0]))
                ref = last[0]
                res["exclusion"][key] = {"users": EXCL_USERS, "filtered": small, "lists": lists, "host_list_bytes": int(outside.size) * 4 * EXCL_USERS}
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
                print(f"pass {name} k={k}: {res['pass'][key]}  on {EXCL_USERS} users: filtered {small} lists {lists}", flush=True)
            del excl
    with open(_opt("--out"), "w") as fh:
        json.dump(res, fh, indent=1)


def run_child(tree, out, filtered=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--out", out] + (["--filtered"] if filtered else [])
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, timeout=900)  # a child that fails or hangs ends the whole run
    return json.load(open(out))


def driver():
    this_tree = os.path.abspath(os.path.join(HERE, ".."))
    parent_tree = os.path.abspath(_opt("--parent-tree"))
    rounds = int(_opt("--rounds", "3"))
    out = _opt("--out", os.path.join(this_tree, "profiles", "filtered_8192x1M_d128"))
    tmp = out + ".child.json"
    res = {"users": U, "items": I, "dim": D, "reps": REPS, "rounds": rounds, "parent": [], "change": []}
    for r in range(rounds):  # alternating: parent, change, parent, change, ...
        res["parent"].append(run_child(parent_tree, tmp)["unfiltered"])
        last = run_child(this_tree, tmp, filtered=(r == rounds - 1))
        res["change"].append(last["unfiltered"])
    os.remove(tmp)
    res["filtered_run"] = last
    med = lambda runs, k, what: sorted(x[f"k{k}"][what] for x in runs)[len(runs) // 2]  # noqa: E731
    L = [f"# The tag filter at {U} users x {I} items, d = {D}", "",
         f"Kernel time = device events around the SBR_K_RANK launches, median of {REPS} repetitions after a warm-up call; wall = the whole",
         "call from Python.  Untrained model, representations = rows of the item table.", "",
         "## 1. recommend_reps unfiltered: parent commit against this build", "",
         f"{rounds} processes of each build, alternating (parent, this build, parent, ...); every process's median, then the median of those.", "",
         "| k | parent kernels ms (each process) | this build kernels ms (each process) | parent median | this build median | this / parent | parent wall ms | this build wall ms |",
         "|---|---|---|---|---|---|---|---|"]
    for k in KS:
        p, c = med(res["parent"], k, "kernels_ms"), med(res["change"], k, "kernels_ms")
        L.append(f"| {k} | " + ", ".join(f"{x[f'k{k}']['kernels_ms']:.2f}" for x in res["parent"]) + " | "
                 + ", ".join(f"{x[f'k{k}']['kernels_ms']:.2f}" for x in res["change"])
                 + f" | {p:.2f} | {c:.2f} | {c / p:.4f} | {med(res['parent'], k, 'wall_ms'):.1f} | {med(res['change'], k, 'wall_ms'):.1f} |")
    L += ["", "## 2. all-pass masks against the unfiltered call (same process, this build)", "",
          "| k | unfiltered kernels ms | all-pass kernels ms | all-pass / unfiltered | unfiltered wall ms | all-pass wall ms |", "|---|---|---|---|---|---|"]
    for k in KS:
        a, b = last["unfiltered"][f"k{k}"], last["all_pass"][f"k{k}"]
        L.append(f"| {k} | {a['kernels_ms']:.2f} | {b['kernels_ms']:.2f} | {b['kernels_ms'] / a['kernels_ms']:.4f} | {a['wall_ms']:.1f} | {b['wall_ms']:.1f} |")
    L += ["", "## 3. filters that pass a part of the catalogue", "",
          "One mask for every user: any_of = one tag bit that about that share of the items carries.", "",
          "| passing | k | kernels ms | / unfiltered | wall ms |", "|---|---|---|---|---|"]
    for name in PASS:
        for k in KS:
            r = last["pass"][f"{name}_k{k}"]
            L.append(f"| {name} ({r['passing'] * 100:.2f} %) | {k} | {r['kernels_ms']:.2f} | {r['kernels_ms'] / last['unfiltered'][f'k{k}']['kernels_ms']:.3f} | {r['wall_ms']:.1f} |")
    L += ["", f"## 4. the exclusion-list equivalent, on {EXCL_USERS} users", "",
          f"recommend_reps with every disallowed item in each user's exclusion list, beside the filtered call on the same {EXCL_USERS} users",
          f"(one user tile).  The lists of {U} users are {U // EXCL_USERS} times the host bytes below — 15 GiB at 50 %, 30 GiB at 1 % — and are",
          "uploaded to the device as well, so the full shape is not run.", "",
          "| passing | k | filtered kernels ms | lists kernels ms | filtered wall ms | lists wall ms | host lists | host lists at 8 192 users |", "|---|---|---|---|---|---|---|---|"]
    for name in PASS:
        for k in KS:
            r = last["exclusion"][f"{name}_k{k}"]
            L.append(f"| {name} | {k} | {r['filtered']['kernels_ms']:.2f} | {r['lists']['kernels_ms']:.2f} | {r['filtered']['wall_ms']:.1f} | {r['lists']['wall_ms']:.1f} | "
                     f"{r['host_list_bytes'] / 2**20:.0f} MiB | {r['host_list_bytes'] * (U // EXCL_USERS) / 2**30:.1f} GiB |")
    L.append("")
    print("\n".join(L), flush=True)
    with open(out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    with open(out + ".md", "w") as fh:
        fh.write("\n".join(L))


if __name__ == "__main__":
    child() if "--child" in argv else driver()
