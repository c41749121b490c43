"""Times keeping a session store across a parameter change: U sessions x 1M items, dim 128, LSTM, a seen-item memory of W = 128 items
per slot, 128 items appended to every session.

    python tools/time_sessions_replay.py [sessions] [--out run.json] [--large slots]
    python tools/time_sessions_replay.py --report profiles/sessions_replay_8192x1M_d128.md --this a.json b.json c.json --parent p.json q.json r.json

(a)  replay: the parameters change (set_param, not timed), then store.replay() — the rings feed the step kernels on the device.
(b)  the host route, which needs nothing this call adds: lists = store.seen(all) before the change, then after it store.reset()
     and store.append(all, lists) — the rings go down to the host, are re-packed there and go up again.  Timed as the sum of the
     three calls.
(c)  model.user_representations of the same 128-item histories: the same arithmetic by the sequence-resident forward pass, for
     orientation.
A build without replay (Sessions has no `replay`) runs (b) and (c) alone: the script runs unchanged on the parent commit.
--large N adds one row: replay alone on a store of N slots whose memories were filled with set_seen.

One process; a seeded untrained LSTM and synthetic histories.  A warm-up of each, then REPS alternating repetitions.  Kernel time =
the engine's device events around the launches: RECURRENT_FWD brackets the session steps and commits (and the ring writes of an
append), SPARSE_SORT brackets replay's feed kernel; wall time = host clock around the calls, each of which ends in a stream
synchronise.  Before timing, (a) and (b) must leave the same bits.  --report takes the .json of several processes of this build and
of the parent's and writes the profile: medians of the process medians."""
import json
import os
import sys
import time

import numpy as np

REPS = 5
I, D, T, W = 1_000_000, 128, 128, 128


def option(name, many=False):
    if name not in sys.argv:
        return [] if many else None
    at = sys.argv.index(name) + 1
    if not many:
        return sys.argv[at]
    out = []
    while at < len(sys.argv) and not sys.argv[at].startswith("--"):
        out.append(sys.argv[at])
        at += 1
    return out


def route_bytes(U, chunks=1):
    """host <-> device bytes of either route, from the shapes (the item table and the states never move in either)"""
    replay = U * 8 + U * 8 + chunks * (T + 1) * 4  # cnt down; slot and count words and the step offsets up
    seen = U * 4 + U * 4 + U * W * 4               # slots up; counts and the padded lists down
    reset = 0
    append = U * 8 + 2 * U * T * 4 + U * 8         # slot and count words, the ids time-major and session-major, the starts
    return replay, seen + reset + append


def report():
    out = option("--report")
    runs = {"this build": [json.load(open(p)) for p in option("--this", many=True)],
            "parent commit": [json.load(open(p)) for p in option("--parent", many=True)]}
    first = runs["this build"][0]
    U = first["sessions"]

    def med(rs, call, key):
        vals = [r["calls"][call][key] for r in rs if call in r["calls"]]
        return (float(np.median(vals)), min(vals), max(vals), len(vals)) if vals else None

    lines = [f"# replay of a session store at {U} sessions x {I} items, d = {D}, LSTM, W = {W}, {T} items per session", "",
             f"Device: {first['device']}, {first['cus']} CUs.  `tools/time_sessions_replay.py`: per process a warm-up of each call, then {REPS}",
             "alternating repetitions and their median; below, the median of the process medians (min .. max of them), the processes of",
             "the two builds run alternately in one session on one device.  Kernel ms = device events around the launches (steps:",
             "session_lstm_step_kernel + session_commit_kernel, and session_seen_append_kernel in an append; feed:",
             "session_replay_feed_steps_kernel); wall ms = host clock around the calls, which end in a stream synchronise.  The",
             "parameter change itself (set_param) is outside every timed window.", "",
             "| build | call | feed kernel ms | step kernels ms | wall ms (min .. max) | processes |", "|---|---|---|---|---|---|"]
    wall = {}
    for build, rs in runs.items():
        if not rs:
            continue
        for call in rs[0]["calls"]:
            if call.startswith("large"):
                continue
            f, s, w = med(rs, call, "feed_ms"), med(rs, call, "steps_ms"), med(rs, call, "wall_ms")
            wall[(build, call)] = w[0]
            lines.append(f"| {build} | {call} | {f[0]:.3f} | {s[0]:.3f} | {w[0]:.2f} ({w[1]:.2f} .. {w[2]:.2f}) | {w[3]} |")
    rb, hb = route_bytes(U)
    a = wall.get(("this build", "(a) replay"))
    bp, bt = wall.get(("parent commit", "(b) host route: seen + reset + append")), wall.get(("this build", "(b) host route: seen + reset + append"))
    lines += [""]
    if a and bp:
        lines += [f"**Condition.** replay's wall time at this build, {a:.2f} ms, against the host route's wall time at the parent commit, {bp:.2f} ms:",
                  f"replay takes {a / bp:.3f} of it ({bp / a:.2f}x faster)" + (f"; against the host route at this build ({bt:.2f} ms): {a / bt:.3f}." if bt else "."),
                  "The condition of the change — replay below the parent's host route — " + ("holds." if a < bp else "DOES NOT hold."), ""]
    sa, sc = med(runs["this build"], "(a) replay", "steps_ms"), med(runs["this build"], "(c) user_representations of the same histories", "steps_ms")
    if a and sa and sc:
        lines += [f"Where replay's time goes: {sa[0]:.2f} of its {a:.2f} ms of wall time are the step kernels — {T} launches of session_lstm_step_kernel and",
                  f"one commit per chunk, {sa[0] / (T + 1) * 1e3:.0f} us each — and the feed kernel and the host's plan are within the rest.  The sequence-resident",
                  f"forward pass does the same arithmetic in {sc[0]:.2f} ms of kernels (row (c), whose wall time is the host's packing of the histories).", ""]
    lines += [f"**Bytes between host and device** (from the shapes; item table and states move in neither): replay {rb:,} B — the slots'",
              f"counts down (8 B per slot), slot and count words and the step offsets up; the host route {hb:,} B — the padded lists down,",
              f"the ids up twice (time-major for the steps, session-major for the ring writes): {hb / rb:.0f}x.", ""]
    parts = [(r["calls"][c], c) for r in runs["this build"] for c in r["calls"] if c.startswith("(b)")]
    if parts and "parts_ms" in parts[0][0]:
        p = {k: float(np.median([x[0]["parts_ms"][k] for x in parts])) for k in parts[0][0]["parts_ms"]}
        lines += ["The host route's wall time by call (this build, median over processes): " + ", ".join(f"{k} {v:.2f} ms" for k, v in p.items()) + ".", ""]
    large = [r["calls"][c] | {"name": c} for r in runs["this build"] for c in r["calls"] if c.startswith("large")]
    if large:
        lg = large[0]
        lines += [f"**One larger row** (one process, replay alone, memories filled with set_seen): {lg['name']}: {lg['chunks']} chunks,",
                  f"feed kernel {lg['feed_ms']:.3f} ms, step kernels {lg['steps_ms']:.3f} ms, wall {lg['wall_ms']:.2f} ms",
                  f"({min(lg['wall_ms_all']):.2f} .. {max(lg['wall_ms_all']):.2f}); {route_bytes(lg['slots'], lg['chunks'])[0]:,} B between host and device.", ""]
    with open(out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if "--report" in sys.argv:
    report()
    sys.exit(0)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

torch.zeros(1, device="cuda")  # PyTorch's HIP runtime first (tests/conftest.py)
from helpers import hparams  # noqa: E402
from sbr_rs_amd._abi import ModelKind, Param  # noqa: E402
from sbr_rs_amd.engine import Model, Sessions, device_info  # noqa: E402

out_path, large = option("--out"), option("--large")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in (out_path, large)]
U = int(args[0]) if args else 8192
HAVE_REPLAY = hasattr(Sessions, "replay")

m = Model(hparams(I, T, D, int(ModelKind.LSTM_NORMAL), 2, B=1024))
rs = np.random.RandomState(5)
items = rs.randint(0, I, U * T).astype(np.uint32)
ptr = np.arange(U + 1, dtype=np.uint64) * T
slots = np.arange(U, dtype=np.uint32)
bias = m.get_param(Param.ITEM_BIAS)


def change_parameters():
    m.set_param(Param.ITEM_BIAS, bias)  # the same values: the generation moves, the expected states do not


store = m.sessions(U, remember=W)
store.append(slots, (ptr, items))
want = store.state(slots)


def same_as_wanted():
    got = store.state(slots)
    return all(np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)) for a, b in zip(got[:2], want[:2])) \
        and np.array_equal(got[2], want[2])


parts = {"seen": [], "reset": [], "append": []}


def host_route(record=False):
    t0 = time.perf_counter()
    lists = store.seen(slots)
    t1 = time.perf_counter()
    change_parameters()
    t2 = time.perf_counter()
    store.reset()
    t3 = time.perf_counter()
    store.append(slots, lists)
    t4 = time.perf_counter()
    if record:
        parts["seen"].append((t1 - t0) * 1e3)
        parts["reset"].append((t3 - t2) * 1e3)
        parts["append"].append((t4 - t3) * 1e3)
    return (t1 - t0) + (t4 - t2)


def replay_route(st=None):
    change_parameters()
    t0 = time.perf_counter()
    (st or store).replay()
    return time.perf_counter() - t0


def forward_only():
    t0 = time.perf_counter()
    m.user_representations(ptr, items)
    return time.perf_counter() - t0


calls = {}
if HAVE_REPLAY:
    calls["(a) replay"] = replay_route
calls["(b) host route: seen + reset + append"] = host_route
calls["(c) user_representations of the same histories"] = forward_only
for name, fn in calls.items():  # warm-up (arena growth, first launches), and the routes must agree
    fn()
    if not name.startswith("(c)"):
        assert same_as_wanted(), name

m.timing_enable(True)
res = {"device": device_info()[0], "cus": device_info()[1], "sessions": U, "items": I, "dim": D, "appended": T, "seen_capacity": W,
       "reps": REPS, "replay": HAVE_REPLAY, "calls": {}}
rec = {name: {"feed": [], "steps": [], "wall": []} for name in calls}
for _ in range(REPS):
    for name, fn in calls.items():
        m.timing_read()
        w = fn(True) if fn is host_route else fn()
        t = m.timing_read()
        rec[name]["wall"].append(w * 1e3)
        rec[name]["feed"].append(t["SPARSE_SORT"][0])
        rec[name]["steps"].append(t["RECURRENT_FWD"][0])
for name, r in rec.items():
    res["calls"][name] = {"feed_ms": float(np.median(r["feed"])), "steps_ms": float(np.median(r["steps"])), "wall_ms": float(np.median(r["wall"])),
                          "wall_ms_all": r["wall"], "feed_ms_all": r["feed"], "steps_ms_all": r["steps"]}
res["calls"]["(b) host route: seen + reset + append"]["parts_ms"] = {k: float(np.median(v)) for k, v in parts.items()}
store.close()

if large and HAVE_REPLAY:
    N = int(large)
    big = m.sessions(N, remember=W)
    for a in range(0, N, 65536):
        b = min(a + 65536, N)
        big.set_seen(np.arange(a, b, dtype=np.uint32), (np.arange(b - a + 1, dtype=np.uint64) * T, rs.randint(0, I, (b - a) * T).astype(np.uint32)))
    replay_route(big)
    r = {"feed": [], "steps": [], "wall": [], "chunks": 0}
    for _ in range(REPS):
        m.timing_read()
        w = replay_route(big)
        t = m.timing_read()
        r["wall"].append(w * 1e3)
        r["feed"].append(t["SPARSE_SORT"][0])
        r["steps"].append(t["RECURRENT_FWD"][0])
        r["chunks"] = int(t["SPARSE_SORT"][1])
    assert big.lengths([0, N - 1]).tolist() == [T, T]
    res["calls"][f"large: replay of {N} slots"] = {"slots": N, "chunks": r["chunks"], "feed_ms": float(np.median(r["feed"])),
                                                    "steps_ms": float(np.median(r["steps"])), "wall_ms": float(np.median(r["wall"])),
                                                    "wall_ms_all": r["wall"]}
    big.close()
m.timing_enable(False)

for name, c in res["calls"].items():
    print(f"{name}: feed {c['feed_ms']:.3f} ms, steps {c['steps_ms']:.3f} ms, wall {c['wall_ms']:.2f} ms", flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
