"""The cases of tests/test_rank_eligible_gpu.py as a table that needs no device, in tests/serving_matrix.py's manner: every case
names the instantiations of the rank_eligible_* kernel templates (sbr_rs_amd/csrc/sbr_rank_eligible.h) it launches, and
tests/test_rank_eligible_cpu.py holds the table against the built library's symbol table — every instantiation is named by a case
at an exact width, and no case names one the library lacks.

This module imports no device code."""
from __future__ import annotations

import collections

import serving_matrix as sm

TEMPLATES = ("rank_eligible_prepare_kernel", "rank_eligible_gemm_kernel", "rank_eligible_finish_kernel")
KINDS = sm.KINDS

Case = collections.namedtuple("Case", "kind dim claims")


def tmax(width: int) -> int:
    """targets per scan row at a stored width (rank_targets_tmax)"""
    return 16 if width <= 128 else 8


def claims(dim: int) -> tuple:
    """what a case at `dim` launches: the filtered bodies run all three templates (a set or a store alone: prepare and finish around
    rank_targets_gemm_kernel, which the serving matrix's roster holds)"""
    D = sm.stored_width(dim)
    return tuple(f"{t}<{D}, {tmax(D)}>" for t in TEMPLATES)


def case_id(c: Case) -> str:
    return f"{c.kind}-d{c.dim}"


# one model kind per width, rotating; every width once exactly and once at its padded dim
CASES = [Case(KINDS[i % 3], w, claims(w)) for i, w in enumerate(sm.WIDTHS)] + \
        [Case(KINDS[(i + 1) % 3], sm.PADDED[w], claims(sm.PADDED[w])) for i, w in enumerate(sm.WIDTHS)]
# the store bodies: all three kinds, at one exact width and one padded dim
STORE_CASES = [Case(k, d, claims(d)) for k in KINDS for d in (16, 100)]


def library_instantiations(lib: str = sm.LIB) -> set:
    """the instantiations of the three templates the library holds, in serving_matrix.short()'s spelling"""
    return {n for n in sm.library_kernels(lib) if "<" in n and n.split("<", 1)[0] in TEMPLATES}


def claimed() -> set:
    """the names claimed at an exact width (a padded case does not stand for its instantiation: serving_matrix.claimed)"""
    return {n for c in CASES + STORE_CASES if c.dim in sm.WIDTHS for n in c.claims}


def named() -> set:
    return {n for c in CASES + STORE_CASES for n in c.claims}
