"""No device: the training matrix is complete.  Every training kernel in the built library (training_matrix's roster, read off
libsbr_hip.so's symbol table) is claimed by a cell of tests/test_training_matrix_gpu.py at an exact width, no cell claims a name the
library does not hold, and the committed kernel list of one traced run of that module shows every roster entry launched."""
import os
import re

import pytest

import serving_matrix as sm
import training_matrix as tm

OWNER_256_16 = "owner_update_kernel<256, 16>"


@pytest.fixture(scope="module")
def roster():
    assert os.path.exists(sm.LIB), "the library is built by __graft_entry__.build()"
    return tm.roster()


def _by_kernel(roster):
    out = {}
    for n in roster:
        out.setdefault(n.split("<", 1)[0], []).append(n)
    return out


def _widths(names):
    return {int(re.match(r"\w+<(\d+)", n).group(1)) for n in names}


def test_the_roster_is_read_off_the_library(roster):
    """every training kernel of the five sources is in the library, the D-templated families have all five widths or exactly the
    widths their launcher can select, and the families' sizes are the launchers' tables"""
    kernels = tm.training_kernels()
    assert {"lstm_fwd_seq_kernel", "lstm_bwd_seq_kernel", "score_kernel", "seg_short_kernel", "owner_list_apply_kernel", "lstm_steps_kernel",
            "small_sort_kernel", "lstm_dw_block_kernel", "block_header_kernel", "stream_delay_kernel"} <= kernels
    by = _by_kernel(roster)
    assert set(by) == {k for k in kernels if not tm._is_test_hook(k)}, "a kernel without an instantiation, or one outside the sources"
    five = set(sm.WIDTHS)
    selectable = {  # the launcher's own condition on the width
        "lstm_fwd_seq_kernel": {16, 32, 64, 128}, "lstm_fwd_wave_kernel": {16, 32}, "lstm_bwd_wave_kernel": {16, 32}, "lstm_dw_block_kernel": {16, 32},
        "lstm_dw_kernel": {16, 32, 64}, "lstm_dw_full_kernel": {64, 128, 256}, "score_tail_kernel": {16, 32}, "small_back_kernel": {16, 32},
        "ewma_steps_kernel": {16, 32}}
    for k, names in by.items():
        if re.match(r"\w+<\d+[,>]", names[0]):
            assert _widths(names) == selectable.get(k, five), k
    count = {k: len(v) for k, v in by.items()}
    # forward: four widths x two gate counts x three tile forms less the 64-sequence form at d = 16 / 32, which launch_recurrent_forward
    # does not instantiate; backward: the same and d = 256's 32-sequence form
    assert count["lstm_fwd_seq_kernel"] == 4 * 2 * 3 - 4 and count["lstm_bwd_seq_kernel"] == 4 * 2 * 3 - 4 + 2
    assert not [n for n in by["lstm_fwd_seq_kernel"] if re.match(r"\w+<(16|32), \d, 4,", n)]
    assert count["lstm_fwd_step_kernel"] == count["lstm_bwd_cell_kernel"] == count["lstm_bwd_gemm_kernel"] == 5 * 2
    assert count["lstm_dw_kernel"] + count["lstm_dw_full_kernel"] == 5 * 2
    assert count["score_kernel"] == 5 * 2 * 2 and count["score_single_kernel"] == 5 * 2 and count["score_tail_kernel"] == 2 * 2
    assert count["seg_short_kernel"] == 5 * 3 * 2 and count["seg_finish_kernel"] == 5 * 3 and count["seg_chunk_kernel"] == 5
    assert count["owner_reduce_kernel"] == count["owner_update_kernel"] == count["owner_list_apply_kernel"] == 5 * 3
    assert count["ewma_seq_kernel"] == 5 + 2 and count["score_refstream_kernel"] == 5
    # five key sources (SrcRows is the self-test's) x two tile sizes; the one-launch sort reads a step's own keys only
    assert count["radix_hist_kernel"] == count["radix_scatter_kernel"] == 5 * 2 and count["small_sort_kernel"] == 2 and count["head_tiles_kernel"] == 4
    assert len(roster) == len(set(roster)) >= 300


def test_the_excluded_kernels_are_the_test_hooks():
    hooks = {n for n in tm.library_training_kernels() if n.startswith("selftest_") or n == "stream_delay_kernel" or "<SrcRows" in n}
    assert set(tm.EXCLUDED) == hooks and all(tm.EXCLUDED.values())
    assert {"selftest_math_kernel", "selftest_store_kernel", "stream_delay_kernel", "small_sort_kernel<SrcRows>"} <= hooks
    assert not set(tm.EXCLUDED) & set(tm.roster())


def test_every_instantiation_is_claimed_by_a_cell(roster):
    left = tm.unclaimed()
    assert not left, f"{len(left)} instantiations no cell launches: {left}"
    assert not tm.UNREACHABLE, "an unreachable instantiation is reported in the pull request that lists it"
    assert not set(tm.UNREACHABLE) - set(roster), "UNREACHABLE names something the library does not hold"


def test_no_cell_claims_a_name_the_library_does_not_hold(roster):
    have = set(roster)
    wrong = {c.label: [n for n in c.claims if n not in have] for c in tm.CELLS}
    wrong = {k: v for k, v in wrong.items() if v}
    assert not wrong, wrong
    ids = [c.label for c in tm.CELLS]
    assert len(ids) == len(set(ids)) and all(c.claims for c in tm.CELLS)


def test_removing_a_cell_names_what_is_left_unclaimed(roster):
    """without the owner-update cell of nine devices at width 256 its 16-device instantiation is reported by name"""
    cells = [c for c in tm.CELLS if not (c.mode == tm.OWNER and c.world == 9 and c.dim == 256)]
    assert len(cells) == len(tm.CELLS) - 1
    left = tm.unclaimed(cells)
    assert left == [OWNER_256_16]
    assert f"{len(left)} instantiations no cell launches: {left}" == f"1 instantiations no cell launches: ['{OWNER_256_16}']"


def test_an_instantiation_without_a_cell_is_reported(roster):
    """a launcher that gains an instantiation gains a roster entry: a roster with one more name than the cells claim fails the check"""
    extra = "lstm_bwd_seq_kernel<256, 4, 4>"
    have = tm.claimed() | set(tm.UNREACHABLE)
    assert [n for n in roster + [extra] if n not in have] == [extra]


def test_the_cells_cover_the_axes():
    exact = [c for c in tm.CELLS if c.dim in sm.WIDTHS]
    env = lambda c: dict(c.env)  # noqa: E731
    for D in (16, 32, 64, 128):  # both LSTM kinds x the three tile requests, and the per-step launches
        for kind in (tm.NORMAL, tm.COUPLED):
            assert {env(c).get("SBR_SEQ_RT") for c in exact if c.kind == kind and c.dim == D and c.label.startswith("seq-")} == {"1", "2", "4"}
            assert any(c.shape == "perstep" and c.kind == kind and c.dim == D for c in exact)
    assert {(c.kind, env(c)["SBR_BWD256_MIN_TILES"]) for c in exact if c.dim == 256 and "SBR_BWD256_MIN_TILES" in env(c)} == {
        (k, t) for k in (tm.NORMAL, tm.COUPLED) for t in ("1", "1000000")}
    for D in sm.WIDTHS:  # WARP's four forms; every exchange for 4, 8 and 16 owners; both sides of 4 096 keys for every Emit policy
        assert {(env(c).get("SBR_SCORE_U"), env(c).get("SBR_STREAM")) for c in exact if c.dim == D and c.label.startswith("warp-")} == {
            (u, s) for u in ("1", "2") for s in ("0", "1")}
        assert {(c.mode, c.world) for c in exact if c.dim == D and c.world > 1 and c.shape == "few"} >= {
            (m, w) for m in (tm.OWNER, tm.GRADIENT, tm.PARTITIONED) for w in (3, 8, 9)}
        assert {c.mode for c in exact if c.dim == D and tm.SHAPES[c.shape].many_keys} >= {tm.SINGLE, tm.OWNER, tm.PARTITIONED}
        assert any(c.mode == tm.REFERENCE and c.dim == D for c in exact)
    assert all(tm.ITEMS % c.world for c in tm.CELLS if c.world > 1)
    assert {c.opt for c in tm.CELLS} == {tm.ADAGRAD, tm.ADAM}
    assert {c.mode for c in tm.CELLS if c.opt == tm.ADAM} >= {tm.SINGLE, tm.OWNER, tm.PARTITIONED, tm.FUSED}
    padded = [c for c in tm.CELLS if c.dim not in sm.WIDTHS]
    assert {c.dim for c in padded} == set(sm.PADDED.values()) and {c.mode for c in padded} == {tm.SINGLE, tm.OWNER, tm.GRADIENT, tm.PARTITIONED}


def test_the_traced_run_launched_every_instantiation(roster):
    """profiles/training_matrix_kernels.md: the kernel names and launch counts of ONE rocprofv3 --kernel-trace run of the GPU module,
    reduced by tools/rocpd_stats.py.  Evidence of that run, not a measurement: counts only, at least one per roster entry, and nothing
    that is neither a training kernel, a test hook nor a serving kernel (the pair sort's cells run a sessions call), the runtime's copy
    and fill kernels and PyTorch's (tests/simulated_ranks.py copies with tensors) aside."""
    assert open(tm.EVIDENCE).readline().startswith("Evidence from one run"), "the file says what it is in its first line"
    seen = tm.evidence(tm.EVIDENCE)
    missing = [n for n in roster if seen.get(n, 0) < 1]
    assert not missing, f"{len(missing)} roster entries the traced run never launched: {missing}"
    known = set(roster) | set(tm.EXCLUDED) | sm.library_kernels()
    stray = [n for n in seen if n not in known and not n.startswith(("__amd_rocclr_", "at::native::"))]
    assert not stray, stray
