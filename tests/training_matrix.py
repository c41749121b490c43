"""The training side as a matrix, as tests/serving_matrix.py is for the serving side: every training kernel the built library
holds (the ROSTER) and the CELLS — one configuration of a fit each: model kind, loss, stored width, optimiser, devices and form
of the step, the environment hooks that force a form, and a named shape — that tests/test_training_matrix_gpu.py runs against
the CPU oracle bit for bit, each naming the kernels it launches.  tests/test_training_matrix_cpu.py holds the two against each
other: every roster entry is claimed by a cell at an exact width, and no cell claims a name the library does not hold.

The roster is derived, not written down: the `__global__` kernels defined in the five training sources (templated or not; their
names only), as the library's symbol table instantiates them, in tools/rocpd_stats.py's spelling — so the kernel trace of the
GPU module (profiles/training_matrix_kernels.md) compares with the roster as text.

`claims(...)` restates the launchers' choices — launch_recurrent_forward / _backward, launch_score, launch_ewma_sequences,
launch_dense_gradient, launch_seg_reduce with its three Emit policies, launch_small_back (sbr_kernels.hip), the wave launchers
(sbr_wave.hip), sort_and_list / radix_sort / launch_merge_sort / launch_pair_sort (sbr_sort.hip), the owner launchers through
DISPATCH_NQ, the step runs and the stream scorer (sbr_steps.hip) and the report kernels (sbr_report.hip) — with step_schedule's
conditions (sbr_engine.hip) in front of them.  A claim is a promise that the cell launches the kernel; a cell may launch more.

This module imports no device code."""
from __future__ import annotations

import collections
import os
import re

import serving_matrix as sm
from serving_matrix import COUPLED, EWMA, NORMAL, PADDED, WIDTHS, evidence, library_kernels, short, stored_width  # noqa: F401

SOURCES = ("sbr_kernels.hip", "sbr_steps.hip", "sbr_sort.hip", "sbr_wave.hip", "sbr_report.hip")
EVIDENCE = os.path.join(sm.ROOT, "profiles", "training_matrix_kernels.md")
LOSS_BPR, LOSS_HINGE, LOSS_WARP = 0, 1, 2  # tests/helpers.py's
ADAGRAD, ADAM = 0, 1
NG = {NORMAL: 4, COUPLED: 3, EWMA: 0}

# the launchers' constants (sbr_kernels.hip, sbr_sort.hip, sbr_numerics.h, sbr_steps.hip)
SEG_INLINE_MAX_KEYS = 4096   # up to this many keys the sparse reduction is one launch; the one-launch sort's limit is the same
DW_CHUNK_ROWS = 1024         # split-K chunk of the dense gradient
EWMA_CHUNK_SEQS = 256        # sequences per dalpha chunk
OVERLAP_MIN_ROWS = 1366      # step_schedule: from this many rows on the sort and the dense gradient run on streams of their own
SCORE_SINGLE_U = 4
SMALL_TAIL_TAIL256_ROWS, SMALL_TAIL_MAX_ROWS, LSTM_STEPS_MAX_ROWS = 64, 255, 48
MAX_T = 1024                 # longest max_sequence_length the sequence-resident kernels take
BWD256_MIN_TILES = 320


# ------------------------------------------------------------------------------------------------
# the roster
# ------------------------------------------------------------------------------------------------
def training_kernels() -> set:
    """the names of the __global__ kernels the five training sources define"""
    names = set()
    for src in SOURCES:
        text = open(os.path.join(sm.CSRC, src)).read()
        names.update(re.findall(r"^__global__[^\n]*?\bvoid (\w+)\(", text, re.M))
    return names


def _is_test_hook(name: str) -> bool:
    return name.startswith("selftest_") or name == "stream_delay_kernel" or "SrcRows" in name


def library_training_kernels(lib: str = sm.LIB) -> list:
    kernels = training_kernels()
    return sorted(n for n in library_kernels(lib) if n.split("<", 1)[0] in kernels)


def excluded(lib: str = sm.LIB) -> dict:
    """Test hooks, which have tests of their own and no place in a fit: name -> the reason."""
    why = {"selftest_": "numeric self-test kernel (tests/test_numerics_gpu.py, tests/test_guarded_scratch_gpu.py)",
           "stream_delay": "the stream-delay hook of tests/test_stream_joins_gpu.py",
           "SrcRows": "the self-test sort's key source (sbr_selftest_sort: tests/test_numerics_gpu.py, both tile sizes and the one-launch form)"}
    return {n: next(v for k, v in why.items() if k in n) for n in library_training_kernels(lib) if _is_test_hook(n)}


EXCLUDED = excluded() if os.path.exists(sm.LIB) else {}


def roster(lib: str = sm.LIB) -> list:
    """the training kernels in the library, instantiation by instantiation, without the test hooks; sorted"""
    return [n for n in library_training_kernels(lib) if not _is_test_hook(n)]


# An instantiation the library holds that no public call reaches: name -> the reason.  Expected to stay empty.
UNREACHABLE: dict = {}


# ------------------------------------------------------------------------------------------------
# the shapes: the smallest at which these kernels can still go wrong
# ------------------------------------------------------------------------------------------------
# B sequences per device and step; lens: "ragged" = U{2..T} (a sequence of two items has no row to train on: both sides leave it out),
# "long" = T, every seventh 3 and a few of 2 (about 9.7 rows per sequence: a step of 200 sequences is past OVERLAP_MIN_ROWS and 4 096
# keys), "perstep" = three sequences of T = 1 030 beside three short ones, "one_long" = 70..T beside a 2 and a 3.  Every shape with
# B > 1 gives two full steps and a ragged third of five sequences (per device: the group's split may end a step earlier).
Shape = collections.namedtuple("Shape", "B T lens many_keys chunks")
SHAPES = {
    "rt1": Shape(37, 12, "ragged", False, False),      # three 16-sequence tiles, the last of 5
    "rt2": Shape(70, 12, "ragged", False, False),      # three 32-sequence tiles, the last of 6
    "rt4": Shape(131, 12, "ragged", False, False),     # three 64-sequence tiles, the last of 3
    "perstep": Shape(3, 1030, "perstep", None, None),  # max_sequence_length past SBR_MAX_T: the per-step launches
    "chunks": Shape(200, 12, "long", True, True),      # two 1 024-row chunks of the dense gradient, the second ragged
    "chunks256": Shape(116, 12, "long", False, True),  # the same at the d = 256 LSTM's price in the oracle
    "wide": Shape(300, 12, "ragged", True, False),     # two dalpha chunks of 256 sequences, the second of 44
    "few": Shape(6, 12, "ragged", False, False),       # a small step on every device of a group
    "one": Shape(1, 12, "ragged", False, False),       # the reference's own schedule: one subsequence per step, at most 11 rows
    "one_long": Shape(1, 100, "one_long", False, False),  # ... of 69..99 rows: the 1 024-thread tail
}
ITEMS = 203  # Zipf; 203 % world != 0 for worlds 3, 8 and 9

SINGLE, OWNER, GRADIENT, PARTITIONED = "single", "owner", "gradient", "partitioned"  # sbr_fit_step; SimulatedRanks' two exchanges; group_create
FUSED, REFERENCE, SESSIONS = "fit", "reference", "sessions"  # a whole fit under set_step_fusion(level); reference order; sessions' audience
Cell = collections.namedtuple("Cell", "label kind loss dim opt world mode env shape claims")


def cell_id(c: Cell) -> str:
    return c.label


# ------------------------------------------------------------------------------------------------
# what a cell launches
# ------------------------------------------------------------------------------------------------
def _nq(world: int) -> int:
    return 4 if world <= 4 else 8 if world <= 8 else 16  # DISPATCH_NQ


def _recurrent(kind, D, env, shape):
    """launch_recurrent_forward / launch_recurrent_backward (and the wave launchers in front of them) for an LSTM"""
    ng, sh = NG[kind], SHAPES[shape]
    if D <= 32 and env.get("SBR_WAVE", "1") != "0":  # unset: up to SBR_WAVE_MAX_SEQ sequences per step
        return [f"lstm_fwd_wave_kernel<{D}, {ng}>", f"lstm_bwd_wave_kernel<{D}, {ng}>"]
    rt = int(env.get("SBR_SEQ_RT", "1"))  # unset: 16-sequence tiles below SBR_SEQ_RT1_MAX_TILES tiles
    rt = rt if rt < 4 or 64 <= D <= 128 else 2
    stepwise = sh.T - 1 > MAX_T
    out = [f"lstm_fwd_step_kernel<{D}, {ng}>" if stepwise or D == 256 else f"lstm_fwd_seq_kernel<{D}, {ng}, {rt}, 1>"]
    resident = D <= 128 or (sh.B + 31) // 32 >= int(env.get("SBR_BWD256_MIN_TILES", BWD256_MIN_TILES))
    if resident and not stepwise:
        return out + [f"lstm_bwd_seq_kernel<{D}, {ng}, {2 if D == 256 else rt}>"]
    return out + [f"lstm_bwd_cell_kernel<{D}, {ng}>", f"lstm_bwd_gemm_kernel<{D}, {ng}>"]


def _dense(kind, D, env, shape, world):
    """launch_dense_gradient and the dense update behind it"""
    ng, sh = NG[kind], SHAPES[shape]
    if not ng:
        one = sh.B <= EWMA_CHUNK_SEQS
        return (["ewma_dab_final_kernel"] if one else ["ewma_dab_chunk_kernel", "ewma_dense_final_kernel"]) + ["dense_apply_kernel"]
    if D <= 32 and env.get("SBR_DW_BLOCK", "1") != "0":  # unset: up to SBR_DW_BLOCK_MAX_CHUNKS chunks
        out = [f"lstm_dw_block_kernel<{D}, {ng}>"]
    else:
        full = (2 * D) % 128 == 0 and (ng * D) % 128 == 0
        out = [f"lstm_dw_full_kernel<{D}, {ng}>" if full else f"lstm_dw_kernel<{D}, {ng}>"]
    if sh.chunks:  # one device: the debug fetch of the first step reduces the partials, the second step's update folds the sum in
        out.append("dense_reduce_local_kernel")
    return out + ["dense_apply_kernel", "repack_lstm_kernel"]


def _score(kind, loss, D, env):
    """launch_score / launch_ewma_sequences without a tail"""
    nt = "true" if env.get("SBR_STREAM", "1") == "1" else "false"  # unset: streaming while the step's h rows are small
    if loss == LOSS_WARP:
        u = int(env.get("SBR_SCORE_U", "2"))  # unset: two rows per lane group below 700 000 rows
        out = [f"score_kernel<{D}, {u}, {'true' if u == 1 else 'false'}, {nt}>"]
        return out + ([f"ewma_forward_kernel<{D}>", f"ewma_backward_kernel<{D}>"] if kind == EWMA else [])
    return [f"ewma_seq_kernel<{D}, false>"] if kind == EWMA else [f"score_single_kernel<{D}, {SCORE_SINGLE_U}, {nt}>"]


def _tiles(src, env, keys_pass=False):
    """radix_sort's launches over one key source; keys_pass: more than one digit, the later passes read the key array"""
    n = 64 if env.get("SBR_SORT_ITEMS") == "64" else 8  # unset: 512-key tiles up to 2^18 keys
    out = [f"radix_hist_kernel<{src}, {n}>", "radix_binscan_kernel", f"radix_scatter_kernel<{src}, {n}>"]
    return out + ([f"radix_hist_kernel<SrcKeys, {n}>", f"radix_scatter_kernel<SrcKeys, {n}>"] if keys_pass else [])


def _sort(loss, env, shape):
    """launch_own_sort: the negatives of a single-negative loss are known before the forward pass (SrcEarly)"""
    src = "SrcBlock" if loss == LOSS_WARP else "SrcEarly"
    if not SHAPES[shape].many_keys and env.get("SBR_SORT_SMALL") != "0":
        return [f"small_sort_kernel<{src}>"]
    n = 64 if env.get("SBR_SORT_ITEMS") == "64" else 8
    return _tiles(src, env) + [f"head_tiles_kernel<false, {n}>", "head_scan_kernel", f"head_tiles_kernel<true, {n}>"]


def _sparse(D, mode, world, env, shape):
    """launch_seg_reduce under the mode's Emit policy, and the owners' side of the exchange"""
    emit = {SINGLE: "EmitApply", OWNER: "EmitChunk", GRADIENT: "EmitChunk", PARTITIONED: "EmitList"}[mode]
    many = SHAPES[shape].many_keys
    out = [f"seg_short_kernel<{D}, {emit}, {'false' if many else 'true'}>"]
    if many:
        out += ["seg_units_kernel", f"seg_chunk_kernel<{D}>", f"seg_finish_kernel<{D}, {emit}>"]
        if mode == SINGLE:  # sbr_fit_step past OVERLAP_MIN_ROWS lists the long segments beside BPTT (the cell's second step)
            out.append("seg_long_list_kernel")
    if mode == OWNER:
        out += ["clear_chunk_flags_kernel", f"owner_update_kernel<{D}, {_nq(world)}>", "accumulate_loss_kernel"]
    elif mode == GRADIENT:
        out += ["clear_chunk_flags_kernel", f"owner_reduce_kernel<{D}, {_nq(world)}>", f"table_apply_kernel<{D}>", "accumulate_loss_kernel"]
    elif mode == PARTITIONED:
        out += ["owner_bounds_kernel", "merge_plan_kernel", f"owner_list_apply_kernel<{D}, {_nq(world)}>"] + _tiles("SrcMerge", env, keys_pass=True)
    return out


def _report(shape, mode):
    """launch_block_header; past OVERLAP_MIN_ROWS the lagged figure is two launches of its own"""
    out = ["block_header_kernel"]
    return out + (["seq_loss_kernel", "lagged_chain_kernel"] if SHAPES[shape].many_keys and mode == SINGLE else [])


def _one_sequence(kind, loss, D, opt, level, shape):
    """one subsequence per step at d <= 32 under sbr_model_set_step_fusion(level): sbr_fit_steps' choice, then step_schedule's"""
    single = loss != LOSS_WARP
    rows_fit_run = shape == "one"  # at most 11 rows: inside SBR_EWMA_STEPS_MAX_ROWS and SBR_LSTM_STEPS_MAX_ROWS
    if level >= 2 and opt == ADAGRAD and single and rows_fit_run:
        if kind == EWMA:
            return [f"ewma_steps_kernel<{D}>"]
        if kind == NORMAL and D == 32:
            return ["lstm_steps_kernel", "repack_lstm_kernel"]
    if level == 0:
        return []
    tail = f"score_tail_kernel<{D}, {256 if shape == 'one' else 1024}>"
    if kind == EWMA:
        return [f"ewma_seq_kernel<{D}, true>" if single else tail, f"small_back_kernel<{D}>"]
    return [f"lstm_fwd_wave_kernel<{D}, {NG[kind]}>", tail, f"lstm_bwd_wave_kernel<{D}, {NG[kind]}>", f"small_back_kernel<{D}>"]


def claims(kind, loss, dim, opt, world, mode, env, shape) -> tuple:
    D, env = stored_width(dim), dict(env)
    if mode == SESSIONS:  # launch_pair_sort: by the low halves, then by the high ones; each a single digit at these sizes
        return tuple(_tiles("SrcSwapped", env))
    if mode == REFERENCE:
        return (f"score_refstream_kernel<{D}>",)
    if mode == FUSED:
        level = int(env["step_fusion"])
        return tuple(_one_sequence(kind, loss, D, opt, level, shape)) or tuple(_score(kind, loss, D, env))
    if shape == "perstep":  # which of the two steps holds how many of the long sequences is the shuffle's choice: the recurrent side only
        return tuple(_score(kind, loss, D, env) + _recurrent(kind, D, env, shape) + _dense(kind, D, env, "rt1", world)[:1])
    out = _score(kind, loss, D, env) + _sort(loss, env, shape) + _sparse(D, mode, world, env, shape) + _report(shape, mode)
    if NG[kind]:
        out += _recurrent(kind, D, env, shape)
    if mode == SINGLE:
        out += _dense(kind, D, env, shape, world) + [f"materialize_dh_kernel<{D}>"]
    return tuple(dict.fromkeys(out))


# ------------------------------------------------------------------------------------------------
# the cells
# ------------------------------------------------------------------------------------------------
_KIND = {NORMAL: "normal", COUPLED: "coupled", EWMA: "ewma"}
_LOSS = {LOSS_BPR: "bpr", LOSS_HINGE: "hinge", LOSS_WARP: "warp"}


def _cell(label, kind, loss, dim, shape, env=(), mode=SINGLE, world=1, opt=ADAGRAD):
    env = tuple(sorted(dict(env).items()))
    name = "-".join([label, _KIND[kind], _LOSS[loss], f"d{dim}"] + (["adam"] if opt == ADAM else []) + ([f"w{world}"] if world > 1 else []))
    return Cell(name, kind, loss, dim, opt, world, mode, env, shape, claims(kind, loss, dim, opt, world, mode, env, shape))


# the single-negative losses and both cache policies over an LSTM width's sequence-resident cells: (kind, tile form) -> (loss, SBR_STREAM)
_SINGLE_NEGATIVE = {(NORMAL, 1): (LOSS_HINGE, "0"), (NORMAL, 2): (LOSS_BPR, "1"), (COUPLED, 1): (LOSS_BPR, "0"), (COUPLED, 2): (LOSS_HINGE, "1"),
                    (NORMAL, 4): (LOSS_WARP, "1"), (COUPLED, 4): (LOSS_WARP, "0")}


def _recurrent_cells():
    out = []
    for D in (16, 32, 64, 128):
        for kind in (NORMAL, COUPLED):
            for rt in (1, 2, 4):  # at d = 16 / 32 the 64-sequence request is served by the 32-sequence form: the cell stays, as the RT 2 form's second shape
                loss, stream = _SINGLE_NEGATIVE[kind, rt]
                env = {"SBR_SEQ_RT": str(rt), "SBR_STREAM": stream, "SBR_WAVE": "0", "SBR_DW_BLOCK": "0"}
                out.append(_cell(f"seq-rt{rt}", kind, loss, D, f"rt{rt}", env))
            # max_sequence_length 1 030: forward, cell and GEMM launches per time step
            out.append(_cell("perstep", kind, LOSS_WARP if kind == NORMAL else LOSS_HINGE, D, "perstep", {"SBR_WAVE": "0"}))
    for i, kind in enumerate((NORMAL, COUPLED)):  # d = 256: forward per step always; BPTT resident (32-sequence tiles) and per step
        for j, (form, tiles) in enumerate((("resident", "1"), ("stepwise", "1000000"))):
            loss, stream = ((LOSS_HINGE, "0"), (LOSS_BPR, "1"), (LOSS_BPR, "0"), (LOSS_HINGE, "1"))[2 * i + j]
            out.append(_cell(f"bptt256-{form}", kind, loss, 256, "rt2", {"SBR_BWD256_MIN_TILES": tiles, "SBR_STREAM": stream}))
    for D in (16, 32):  # the wave form, and the dense gradient's block form beside the tile kernel
        for kind, loss in ((NORMAL, LOSS_WARP), (COUPLED, LOSS_BPR)):
            out.append(_cell("wave", kind, loss, D, "rt1", {"SBR_WAVE": "1", "SBR_DW_BLOCK": "1"}))
            out.append(_cell("dwblock", kind, loss, D, "chunks", {"SBR_WAVE": "1", "SBR_DW_BLOCK": "1"}))
    for D in WIDTHS:  # lstm_dw_kernel / lstm_dw_full_kernel as the width selects them, over two chunks
        for kind, loss in ((NORMAL, LOSS_HINGE), (COUPLED, LOSS_WARP)):
            out.append(_cell("dwchunks", kind, loss, D, "chunks256" if D == 256 else "chunks", {"SBR_WAVE": "0", "SBR_DW_BLOCK": "0", "SBR_SEQ_RT": "2"}))
    return out


def _scoring_cells():
    out = []
    for D in WIDTHS:
        for u in ("1", "2"):
            for stream in ("0", "1"):  # EWMA + WARP: ewma_forward_kernel, the score kernel's four forms, ewma_backward_kernel
                out.append(_cell(f"warp-u{u}-nt{stream}", EWMA, LOSS_WARP, D, "rt2", {"SBR_SCORE_U": u, "SBR_STREAM": stream}))
        out.append(_cell("reference", (EWMA, NORMAL, COUPLED)[WIDTHS.index(D) % 3], (LOSS_WARP, LOSS_HINGE, LOSS_BPR)[WIDTHS.index(D) % 3], D, "one",
                         mode=REFERENCE))
    out.append(_cell("dalpha-chunks", EWMA, LOSS_WARP, 64, "wide"))
    for D in (16, 32):  # one subsequence per step
        for level in (2, 1, 0):
            fusion = {"step_fusion": str(level)}
            out.append(_cell(f"one-f{level}", EWMA, LOSS_HINGE, D, "one", fusion, FUSED))
            out.append(_cell(f"one-f{level}", NORMAL, LOSS_BPR, D, "one", fusion, FUSED))
            out.append(_cell(f"one-f{level}", COUPLED, LOSS_WARP, D, "one", fusion, FUSED))
        out.append(_cell("one-long-f1", NORMAL, LOSS_WARP, D, "one_long", {"step_fusion": "1"}, FUSED))
        out.append(_cell("one-long-f2", EWMA, LOSS_WARP, D, "one_long", {"step_fusion": "2"}, FUSED))
        out.append(_cell("one-f2", EWMA, LOSS_BPR, D, "one", {"step_fusion": "2"}, FUSED, opt=ADAM))  # Adam: no step run, the fused launches
    return out


def _sparse_cells():
    out = []
    for D in WIDTHS:  # the item side does not depend on the model kind: EWMA + hinge keeps the oracle's time down
        out.append(_cell("apply", EWMA, LOSS_HINGE, D, "rt2"))
        out.append(_cell("apply-many", EWMA, LOSS_HINGE, D, "chunks"))
        for world in (3, 8, 9):
            for mode in (OWNER, GRADIENT, PARTITIONED):
                out.append(_cell(mode, EWMA, LOSS_HINGE, D, "few", mode=mode, world=world))
        for mode in (OWNER, PARTITIONED):
            out.append(_cell(f"{mode}-many", EWMA, LOSS_HINGE, D, "chunks", mode=mode, world=3))
    out.append(_cell("gradient-many", EWMA, LOSS_HINGE, 64, "chunks", mode=GRADIENT, world=3))
    return out


def _ordering_cells():
    out = []
    for n in ("8", "64"):  # the tiled passes on small inputs, for each key source
        tiled = {"SBR_SORT_SMALL": "0", "SBR_SORT_ITEMS": n}
        out.append(_cell(f"sort-tiles{n}", EWMA, LOSS_WARP, 32, "rt2", tiled))
        out.append(_cell(f"sort-tiles{n}", EWMA, LOSS_HINGE, 32, "rt2", tiled))
        out.append(_cell(f"sort-tiles{n}", EWMA, LOSS_HINGE, 32, "few", {"SBR_SORT_ITEMS": n}, PARTITIONED, world=3))
        out.append(_cell(f"pair-sort-tiles{n}", EWMA, LOSS_HINGE, 32, "one", {"SBR_SORT_ITEMS": n}, SESSIONS))
    out.append(_cell("sort-many", EWMA, LOSS_WARP, 16, "chunks"))
    return out


def _adam_cells():
    """the optimiser is a run-time branch of the update kernels: one cell per Emit policy and per dense path"""
    out = [_cell("apply-many", EWMA, LOSS_HINGE, 128, "chunks", opt=ADAM),
           _cell("owner", EWMA, LOSS_WARP, 32, "few", mode=OWNER, world=3, opt=ADAM),
           _cell("partitioned", EWMA, LOSS_BPR, 64, "few", mode=PARTITIONED, world=3, opt=ADAM),
           _cell("dwchunks", NORMAL, LOSS_BPR, 64, "chunks", {"SBR_SEQ_RT": "2"}, opt=ADAM),  # the reduce-apply launch
           _cell("dwblock", COUPLED, LOSS_HINGE, 32, "rt1", {"SBR_WAVE": "1", "SBR_DW_BLOCK": "1"}, opt=ADAM),
           _cell("one-f1", COUPLED, LOSS_HINGE, 16, "one", {"step_fusion": "1"}, FUSED, opt=ADAM)]  # small_back_kernel's update
    return out


def _padded_cells():
    """a padded dim's last columns are zeros the oracle never sees: one cell per recurrent form and per sparse form"""
    seq = lambda rt: {"SBR_SEQ_RT": str(rt), "SBR_WAVE": "0", "SBR_DW_BLOCK": "0"}  # noqa: E731
    return [_cell("seq-rt1", NORMAL, LOSS_WARP, PADDED[16], "rt1", seq(1)), _cell("seq-rt2", COUPLED, LOSS_HINGE, PADDED[64], "rt2", seq(2)),
            _cell("seq-rt4", NORMAL, LOSS_BPR, PADDED[128], "rt4", seq(4)), _cell("wave", COUPLED, LOSS_WARP, PADDED[32], "rt1", {"SBR_WAVE": "1"}),
            _cell("bptt256-resident", NORMAL, LOSS_WARP, PADDED[256], "rt2", {"SBR_BWD256_MIN_TILES": "1"}),
            _cell("perstep", COUPLED, LOSS_WARP, PADDED[64], "perstep"),
            _cell("apply", EWMA, LOSS_HINGE, PADDED[128], "rt2"), _cell("apply-many", EWMA, LOSS_WARP, PADDED[32], "chunks"),
            _cell("owner", EWMA, LOSS_HINGE, PADDED[16], "few", mode=OWNER, world=3),
            _cell("gradient", EWMA, LOSS_WARP, PADDED[64], "few", mode=GRADIENT, world=8),
            _cell("partitioned", EWMA, LOSS_HINGE, PADDED[256], "few", mode=PARTITIONED, world=9)]


CELLS = _recurrent_cells() + _scoring_cells() + _sparse_cells() + _ordering_cells() + _adam_cells() + _padded_cells()


def claimed(cells=None) -> set:
    """the names claimed at an exact width (a padded cell does not stand for its instantiation: serving_matrix.claimed)"""
    return {name for c in (CELLS if cells is None else cells) if c.dim in WIDTHS for name in c.claims}


def unclaimed(cells=None, lib: str = sm.LIB) -> list:
    """the roster entries no cell claims and UNREACHABLE does not explain"""
    have = claimed(cells) | set(UNREACHABLE)
    return [n for n in roster(lib) if n not in have]
