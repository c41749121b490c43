"""Times seen-item exclusion on the session store: U sessions x 1M items, dim 128, LSTM, 128 items appended to every session, a
seen-item memory of W = 128 items per slot.

    python tools/time_sessions_seen.py [sessions] [--out profiles/sessions_seen_8192x1M_d128] [--parent parent.json]

(a)  store.recommend(k) on a store WITH memory: the exclusion lists are made on the device from the rings.
(b)  store.recommend(k, exclude = the same items as host lists) on a plain store: what a caller does without the memory — the
     host sorts and de-duplicates the lists and uploads them with every call.  Timed twice: through the Python method (which also
     builds the CSR from the per-session sequences) and as the C call sbr_sessions_recommend on a CSR prepared beforehand, the
     library's own wall time.
(c)  store.recommend(k) on the plain store, nothing excluded.
append of one item to every session, on the store with memory and on the plain one.

A build without the memory (Model.sessions has no `remember`) runs (b), (c) and the plain append alone: run on the parent commit,
its --out .json can be given to a later run as --parent, which adds that table to the .md.

One process; a seeded untrained LSTM and synthetic histories.  A warm-up call of each, then REPS alternating repetitions; kernel
time = the engine's device events around the launches of the SBR_K_RANK family (top-k GEMM + merge, and the list-building kernel
where there is one) and of the SBR_K_RECURRENT_FWD family (session step + commit, and the ring writes); wall time = host clock
around the call (every call ends in a stream synchronise); medians, and the spread as min .. max.  Before timing, (a) and (b) must
agree bit for bit."""
import inspect
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

torch.zeros(1, device="cuda")  # PyTorch's HIP runtime first (tests/conftest.py)
from helpers import hparams  # noqa: E402
from sbr_rs_amd._abi import ModelKind  # noqa: E402
from sbr_rs_amd.engine import Model, _ptr, device_info  # noqa: E402


def option(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


out_base, parent_json = option("--out"), option("--parent")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in (out_base, parent_json)]
U, I, D, T, W = int(args[0]) if args else 8192, 1_000_000, 128, 128, 128
REPS, KS = 7, (10, 100)
HAVE_MEMORY = "remember" in inspect.signature(Model.sessions).parameters

m = Model(hparams(I, T, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
rs = np.random.RandomState(5)
items = rs.randint(0, I, U * T).astype(np.uint32)
ptr = np.arange(U + 1, dtype=np.uint64) * T
slots = np.arange(U, dtype=np.uint32)
one_ptr = np.arange(U + 1, dtype=np.uint64)
one = rs.randint(0, I, U).astype(np.uint32)
host_lists = items.reshape(U, T)  # the same items as host lists, one row per session

plain = m.sessions(U)
plain.append(slots, (ptr, items))
mem = None
if HAVE_MEMORY:
    mem = m.sessions(U, remember=W)
    mem.append(slots, (ptr, items))
    for k in KS:
        a, b = mem.recommend(slots, k), plain.recommend(slots, k, exclude=host_lists)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "memory and host lists disagree"
        c = plain.recommend(slots, k)
        assert not np.array_equal(a[0], c[0]), "the lists exclude something"


def c_call(st, k, out_items, out_scores):
    """sbr_sessions_recommend on the CSR prepared once: the library's share of (b)"""
    rc = st._L.sbr_sessions_recommend(st._h, _ptr(slots), U, k, _ptr(ptr), _ptr(items), 0, _ptr(out_items), _ptr(out_scores))
    assert rc == 0, rc


calls = {}
for k in KS:
    oi, os_ = np.zeros((U, k), np.uint32), np.zeros((U, k), np.float32)
    if mem is not None:
        calls[f"(a) recommend k={k}, store with memory"] = lambda k=k: mem.recommend(slots, k)
    calls[f"(b) recommend k={k}, plain store, exclude=host lists"] = lambda k=k: plain.recommend(slots, k, exclude=host_lists)
    calls[f"(b) the same as the C call on a prepared CSR, k={k}"] = lambda k=k, oi=oi, os_=os_: c_call(plain, k, oi, os_)
    calls[f"(c) recommend k={k}, plain store, nothing excluded"] = lambda k=k: plain.recommend(slots, k)
if mem is not None:
    calls["append 1 item each, store with memory"] = lambda: mem.append(slots, (one_ptr, one))
calls["append 1 item each, plain store"] = lambda: plain.append(slots, (one_ptr, one))

for fn in calls.values():  # warm-up (arena growth, first launches)
    fn()
m.timing_enable(True)
fwd = {name: [] for name in calls}
scan = {name: [] for name in calls}
wall = {name: [] for name in calls}
for _ in range(REPS):
    for name, fn in calls.items():
        m.timing_read()
        t0 = time.perf_counter()
        fn()
        wall[name].append((time.perf_counter() - t0) * 1e3)
        t = m.timing_read()
        fwd[name].append(t["RECURRENT_FWD"][0])
        scan[name].append(t["RANK"][0])
m.timing_enable(False)

name_dev, cus, hbm = device_info()
res = {"device": name_dev, "cus": cus, "sessions": U, "items": I, "dim": D, "appended": T, "seen_capacity": W if HAVE_MEMORY else 0,
       "reps": REPS, "calls": {}}
for name in calls:
    res["calls"][name] = {"recurrent_kernels_ms_median": float(np.median(fwd[name])), "scan_kernels_ms_median": float(np.median(scan[name])),
                          "wall_ms_median": float(np.median(wall[name])), "recurrent_kernels_ms_all": fwd[name],
                          "scan_kernels_ms_all": scan[name], "wall_ms_all": wall[name]}


def table(r):
    rows = ["| call | recurrent kernels ms | scan kernels ms (min .. max) | wall ms (min .. max) |", "|---|---|---|---|"]
    for name, c in r["calls"].items():
        rows.append(f"| {name} | {c['recurrent_kernels_ms_median']:.3f} | {c['scan_kernels_ms_median']:.3f} "
                    f"({min(c['scan_kernels_ms_all']):.3f} .. {max(c['scan_kernels_ms_all']):.3f}) | {c['wall_ms_median']:.2f} "
                    f"({min(c['wall_ms_all']):.2f} .. {max(c['wall_ms_all']):.2f}) |")
    return rows


lines = [f"# seen-item exclusion at {U} sessions x {I} items, d = {D}, LSTM, {T} items appended per session, W = {W}", "",
         f"Device: {name_dev}, {cus} CUs.  One process, a warm-up call of each, then {REPS} alternating repetitions; medians, and the",
         "spread of the repetitions as min .. max.  Kernel ms = device events around the launches of the scan family (top-k GEMM + merge,",
         "and session_seen_lists_kernel where the store has memory) and of the recurrent family (session step + commit, and",
         "session_seen_append_kernel where the store has memory); wall ms = host clock around the call, which ends in a stream",
         "synchronise and includes the host's list preparation, uploads and the copy of the results.", ""] + table(res)
if parent_json:
    with open(parent_json) as f:
        res["parent"] = json.load(f)
    lines += ["", "The same script at the parent commit (a build without the memory; a process of its own on the same device, run just",
              "before the one above):", ""] + table(res["parent"])
print("\n".join(lines), flush=True)
if out_base:
    with open(out_base + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(out_base + ".md", "w") as f:
        f.write("\n".join(lines) + "\n")
plain.close()
if mem is not None:
    mem.close()
