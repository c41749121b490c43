"""No device: the serving matrix is complete.  Every templated serving kernel instantiation in the built library (serving_matrix's
roster, read off libsbr_hip.so's symbol table) is claimed by a cell of tests/test_serving_matrix_gpu.py, no cell claims a name the
library does not hold, and the committed kernel list of one traced run of that module shows every roster entry launched."""
import os

import pytest

import serving_matrix as sm

QUERYBIAS_64 = "topk_gemm_kernel<64, QueryBias, NoFilter>"


@pytest.fixture(scope="module")
def roster():
    assert os.path.exists(sm.LIB), "the library is built by __graft_entry__.build()"
    return sm.roster()


def test_the_roster_is_read_off_the_library(roster):
    """every serving template has instantiations, every width appears, and the families the dispatch code names are all there"""
    templates = sm.serving_templates()
    assert {"topk_gemm_kernel", "above_gemm_kernel", "select_gemm_kernel", "partition_gemm_kernel", "rank_gemm_kernel", "rank_targets_gemm_kernel",
            "diverse_select_kernel", "subset_gather_kernel", "partition_prefix_kernel", "session_lstm_step_kernel", "session_commit_kernel",
            "session_ewma_step_kernel", "session_seen_lists_kernel", "audience_seen_match_kernel"} <= templates
    by_template = {t: [n for n in roster if n.split("<", 1)[0] == t] for t in templates}
    assert all(by_template.values()), [t for t, v in by_template.items() if not v]
    for t, names in by_template.items():
        if names[0].split("<", 1)[1][:2].isdigit() and t != "session_seen_lists_kernel":  # D-templated (not the merge's list size)
            assert {int(n.split("<", 1)[1].split(",")[0].rstrip(">")) for n in names} == set(sm.WIDTHS), t
    # topk_scan's pairs: four policies with and without a filter, QueryBias without; above_scan's and launch_top_select's three
    assert len(by_template["topk_gemm_kernel"]) == 5 * 9 and len(by_template["above_gemm_kernel"]) == 5 * 3 * 2
    assert len(by_template["select_gemm_kernel"]) == 5 * 3 and len(by_template["partition_gemm_kernel"]) == 5 * 2
    assert QUERYBIAS_64 in roster and not any("QueryBias, TagFilter" in n for n in roster)
    assert len(roster) == len(set(roster)) >= 190


def test_every_instantiation_is_claimed_by_a_cell(roster):
    left = sm.unclaimed()
    assert not left, f"{len(left)} instantiations no cell launches: {left}"
    assert not sm.UNREACHABLE, "an unreachable instantiation is reported in the pull request that lists it"
    assert not set(sm.UNREACHABLE) - set(roster), "UNREACHABLE names something the library does not hold"


def test_no_cell_claims_a_name_the_library_does_not_hold(roster):
    have = set(roster)
    wrong = {sm.cell_id(c): [n for n in c.claims if n not in have] for c in sm.CELLS}
    wrong = {k: v for k, v in wrong.items() if v}
    assert not wrong, wrong
    ids = [sm.cell_id(c) for c in sm.CELLS]
    assert len(ids) == len(set(ids)) and all(c.claims for c in sm.CELLS)


def test_removing_a_cell_names_what_is_left_unclaimed(roster):
    """without the audience cell at width 64 its QueryBias instantiation is reported by name; the check has teeth"""
    cells = [c for c in sm.CELLS if not (c.call == "audience" and c.dim == 64)]
    assert len(cells) == len(sm.CELLS) - 1
    assert sm.unclaimed(cells) == [QUERYBIAS_64]


def test_the_cells_cover_the_axes():
    """all five exact widths and one padded dim each; every kind at every width for the recurrent calls; a filtered twin wherever
    the call takes masks"""
    for call, takes_masks in sm.CATALOGUE_CALLS:
        for w in sm.WIDTHS:
            got = {c.filtered for c in sm.CELLS if c.call == call and c.dim == w}
            assert got == ({False, True} if takes_masks else {False}), (call, w)
    for call in sm.RECURRENT_CALLS:
        assert {(c.kind, c.dim) for c in sm.CELLS if c.call == call and c.dim in sm.WIDTHS} == {(k, w) for k in sm.KINDS for w in sm.WIDTHS}, call
    for w, dim in sm.PADDED.items():
        assert sm.stored_width(dim) == w and dim < w
        assert {c.call for c in sm.CELLS if c.dim == dim} == set(sm.PADDED_CATALOGUE_CALLS) | set(sm.PADDED_RECURRENT_CALLS)


def test_the_traced_run_launched_every_instantiation(roster):
    """profiles/serving_matrix_kernels.md: the kernel names and launch counts of ONE rocprofv3 --kernel-trace run of the GPU module,
    reduced by tools/rocpd_stats.py.  Evidence of that run, not a measurement: counts only, at least one per roster entry."""
    assert open(sm.EVIDENCE).readline().startswith("Evidence from one run"), "the file says what it is in its first line"
    seen = sm.evidence()
    missing = [n for n in roster if seen.get(n, 0) < 1]
    assert not missing, f"{len(missing)} roster entries the traced run never launched: {missing}"
