"""The serving side as a matrix: every templated serving kernel instantiation the built library holds (the ROSTER), and the CELLS —
public calls with concrete arguments — that tests/test_serving_matrix_gpu.py runs against the CPU oracle, each naming the
instantiations it launches.  tests/test_serving_matrix_cpu.py holds the two against each other: every roster entry is claimed by
a cell, and no cell claims a name the library does not hold.

The roster is derived, not written down.  The serving kernel templates are the `template <...> __global__` definitions of
sbr_catalogue.hip and sbr_sessions.hip (their names only); their instantiations are the demangled host stubs of libsbr_hip.so
(`sbr::__device_stub__NAME<ARGS>(...)` in the symbol table, which a build without a GPU produces).  A name is written the way
tools/rocpd_stats.py shortens a trace's kernel names — `topk_gemm_kernel<64, QueryBias, NoFilter>` — so a kernel trace of the
GPU module (profiles/serving_matrix_kernels.md) compares with the roster as text.

This module imports no device code."""
from __future__ import annotations

import collections
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sbr_rs_amd", "csrc")
LIB = os.path.join(ROOT, "sbr_rs_amd", "libsbr_hip.so")
SOURCES = ("sbr_catalogue.hip", "sbr_sessions.hip")
EVIDENCE = os.path.join(ROOT, "profiles", "serving_matrix_kernels.md")

WIDTHS = (16, 32, 64, 128, 256)                      # the stored widths; a cell's embedding_dim is the width itself,
PADDED = {16: 9, 32: 24, 64: 48, 128: 100, 256: 200}  # or the width's padded dim: the last columns are zeros the oracle never sees
NORMAL, COUPLED, EWMA = "LSTM_NORMAL", "LSTM_COUPLED", "EWMA"  # sbr_rs_amd._abi.ModelKind's names
KINDS = (NORMAL, COUPLED, EWMA)

# the shape of every cell (the issue's: the smallest at which these kernels can go wrong)
ITEMS, ROWS, K, GROUPS = 229, 130, 10, 3  # item ranges of 96, 96 and 37: several tiles per range, a ragged last tile, a short range
TIES = ((31, 32), (95, 96))               # identical rows and biases: a pair across a 32-item tile edge, a pair across a range edge


def stored_width(dim: int) -> int:
    return next(w for w in WIDTHS if dim <= w)


# ------------------------------------------------------------------------------------------------
# the roster
# ------------------------------------------------------------------------------------------------
def serving_templates() -> set:
    """the names of the templated __global__ kernels of the two serving sources"""
    names = set()
    for src in SOURCES:
        text = open(os.path.join(CSRC, src)).read()
        names.update(re.findall(r"^template <[^>\n]*>\n__global__[^\n]*?\bvoid (\w+)\(", text, re.M))
    return names


def short(name: str) -> str:
    """tools/rocpd_stats.py's spelling of a demangled kernel name"""
    name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", ""))
    return name.replace("void ", "").replace("sbr::", "").replace("__device_stub__", "").strip()


def library_kernels(lib: str = LIB) -> set:
    """every kernel the library holds a host stub of, in short()'s spelling"""
    out = subprocess.run(["nm", "-C", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return {short(m.group(1)) for m in re.finditer(r"^\S+ \w (.*__device_stub__.*)$", out, re.M)}


def roster(lib: str = LIB) -> list:
    """the instantiations of the serving templates in the library, sorted"""
    templates = serving_templates()
    return sorted(n for n in library_kernels(lib) if "<" in n and n.split("<", 1)[0] in templates)


# An instantiation the library holds that no public call reaches: name -> the reason.  Expected to stay empty.
UNREACHABLE: dict = {}


# ------------------------------------------------------------------------------------------------
# the cells
# ------------------------------------------------------------------------------------------------
Cell = collections.namedtuple("Cell", "call kind dim filtered claims")


def cell_id(c: Cell) -> str:
    return f"{c.call}-{c.kind}-d{c.dim}" + ("-tags" if c.filtered else "")


def _step(kind: str, D: int) -> list:
    """the session cell step of a model kind: what append, replay, rollout and beam_search advance a state with"""
    if kind == EWMA:
        return [f"session_ewma_step_kernel<{D}>"]
    return [f"session_lstm_step_kernel<{D}, {4 if kind == NORMAL else 3}>"]


def _claims(call: str, kind: str, D: int, F: str) -> list:
    """what `call` launches at stored width D under filter F, as topk_scan, above_scan, launch_top_select and partition_sum
    dispatch it (sbr_catalogue.hip) and as launch_session_append and its neighbours do (sbr_sessions.hip)"""
    topk = lambda score, f=F: f"topk_gemm_kernel<{D}, {score}, {f}>"  # noqa: E731
    above = lambda score, f=F: [f"above_gemm_kernel<{D}, {score}, {f}, false>", f"above_gemm_kernel<{D}, {score}, {f}, true>"]  # noqa: E731
    TM = 16 if D <= 128 else 8
    return {
        # one catalogue scan per score policy
        "recommend": lambda: [topk("BiasAdd")],
        "similar_cosine": lambda: [f"item_rnorm_kernel<{D}>", f"similar_query_kernel<{D}>", topk("ScaleMul")],
        "similar_dot": lambda: [f"item_rnorm_kernel<{D}>", f"similar_query_kernel<{D}>", topk("ScaleMul")],
        "audience": lambda: [f"subset_gather_kernel<{D}>", topk("QueryBias")],
        "sampled": lambda: [topk("GumbelBias"), f"candidate_score_kernel<{D}>"],
        "set_sampled": lambda: [f"subset_gather_kernel<{D}>", topk("GumbelMapped"), f"candidate_score_kernel<{D}>"],
        # the sum, threshold and budget scans
        "log_partition": lambda: [topk("BiasAdd"), f"partition_gemm_kernel<{D}, {F}>", f"partition_finish_kernel<{D}>"],
        "above": lambda: above("BiasAdd"),
        "audience_above": lambda: [f"subset_gather_kernel<{D}>"] + above("QueryBias"),
        "top": lambda: [f"select_gemm_kernel<{D}, BiasAdd, {F}>"] + above("BiasAdd"),
        "audience_top": lambda: [f"subset_gather_kernel<{D}>", f"select_gemm_kernel<{D}, QueryBias, {F}>"] + above("QueryBias"),
        # a selection behind recommend's pool, and the small kernels
        "capped": lambda: [topk("BiasAdd")],
        "diverse": lambda: [topk("BiasAdd"), f"diverse_select_kernel<{D}>"],
        "candidates": lambda: [f"candidate_score_kernel<{D}>", f"predict_kernel<{D}>"],
        "among": lambda: [f"subset_gather_kernel<{D}>", topk("BiasAdd")],
        "rank_targets": lambda: [f"rank_targets_{part}_kernel<{D}, {TM}>" for part in ("prepare", "gemm", "finish")],
        # everything with a recurrent cell in it
        "append": lambda: _step(kind, D) + ([] if kind == EWMA else [f"session_commit_kernel<{D}>"]),
        "replay": lambda: _step(kind, D) + ([] if kind == EWMA else [f"session_commit_kernel<{D}>"]) + [
            "session_seen_lists_kernel<64>", "audience_seen_match_kernel<false>", "audience_seen_match_kernel<true>"],
        "seen_wide": lambda: _step(kind, D) + ["session_seen_lists_kernel<256>", topk("BiasAdd")],
        "rollout": lambda: _step(kind, D) + [topk("BiasAdd"), topk("GumbelBias"), f"partition_gemm_kernel<{D}, {F}>",
                                            f"partition_finish_kernel<{D}>", f"candidate_score_kernel<{D}>"],
        "set_rollout": lambda: _step(kind, D) + [f"subset_gather_kernel<{D}>", topk("BiasAdd"), topk("GumbelMapped"),
                                                f"partition_gemm_kernel<{D}, {F}>", f"candidate_score_kernel<{D}>"],
        "beam": lambda: _step(kind, D) + [topk("BiasAdd"), f"partition_gemm_kernel<{D}, {F}>"],
        "set_beam": lambda: _step(kind, D) + [f"subset_gather_kernel<{D}>", topk("BiasAdd"), f"partition_gemm_kernel<{D}, {F}>"],
        "sequences": lambda: [f"rank_test_score_kernel<{D}>", f"rank_gemm_kernel<{D}>", f"rank_history_kernel<{D}>", f"rank_prefix_kernel<{D}>",
                              topk("BiasAdd"), f"partition_gemm_kernel<{D}, {F}>", f"partition_prefix_kernel<{D}>"],
    }[call]()


# the catalogue calls, and whether the call takes tag masks (audience has no filter: that pair of policies does not exist)
CATALOGUE_CALLS = (("recommend", True), ("similar_cosine", True), ("similar_dot", True), ("audience", False), ("sampled", True),
                   ("set_sampled", True), ("log_partition", True), ("above", True), ("audience_above", False), ("top", True),
                   ("audience_top", False), ("capped", True), ("diverse", False), ("candidates", False), ("among", False),
                   ("rank_targets", False))
RECURRENT_CALLS = ("append", "replay", "rollout", "set_rollout", "beam", "set_beam", "sequences")
# at a padded dim: one call of each kernel family (top-k, threshold, budget, sum, rank and the small kernels; the cell step)
PADDED_CATALOGUE_CALLS = ("recommend", "similar_cosine", "audience", "sampled", "set_sampled", "log_partition", "above", "top", "diverse",
                          "candidates", "rank_targets")
PADDED_RECURRENT_CALLS = ("append", "rollout", "sequences")


def _cell(call, kind, dim, filtered=False):
    return Cell(call, kind, dim, filtered, tuple(_claims(call, kind, stored_width(dim), "TagFilter" if filtered else "NoFilter")))


def _cells():
    out = []
    for w in WIDTHS:
        for call, takes_masks in CATALOGUE_CALLS:  # the item side does not depend on the model kind: one EWMA model per width
            out += [_cell(call, EWMA, w, f) for f in ((False, True) if takes_masks else (False,))]
        for kind in KINDS:
            out += [_cell(call, kind, w) for call in RECURRENT_CALLS]
    for i, w in enumerate(WIDTHS):
        out += [_cell(call, EWMA, PADDED[w]) for call in PADDED_CATALOGUE_CALLS]
        out += [_cell(call, KINDS[i % 3], PADDED[w]) for call in PADDED_RECURRENT_CALLS]
    out.append(_cell("seen_wide", EWMA, 16))  # a memory of 100 items: the wide form of the seen-list merge, which no width selects
    return out


CELLS = _cells()


def claimed(cells=None) -> set:
    """the names claimed at an exact width: a padded dim's last columns are zeros, under which a mis-indexed last k-slice multiplies
    zeros, so a padded cell does not stand for its instantiation"""
    return {name for c in (CELLS if cells is None else cells) if c.dim in WIDTHS for name in c.claims}


def unclaimed(cells=None, lib: str = LIB) -> list:
    """the roster entries no cell claims and UNREACHABLE does not explain"""
    have = claimed(cells) | set(UNREACHABLE)
    return [n for n in roster(lib) if n not in have]


# ------------------------------------------------------------------------------------------------
# the evidence: the kernel names of one traced run of the GPU module
# ------------------------------------------------------------------------------------------------
def evidence(path: str = EVIDENCE) -> dict:
    """{kernel name: launches} of the committed list (tools/rocpd_stats.py's table: | `name` | calls | ...)"""
    out = {}
    for line in open(path):
        m = re.match(r"\| `([^`]+)` \| (\d+) \|", line)
        if m:
            out[m.group(1)] = out.get(m.group(1), 0) + int(m.group(2))
    return out
