"""CPU: rank_targets under a serving policy (ELIGIBLE RANKS, include/sbr_hip.h).  The two entries are declared, exported and bound;
the numpy expectation (rank_eligible_expect) answers its own small cases; ranking_metrics' "miss" / "skip" arithmetic and
eligible_targets hold on hand-made inputs; and the roster: the instantiations of the three rank_eligible_* kernel templates in the
built library are exactly those the GPU module's cases name (tests/rank_eligible_cases.py)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import rank_eligible_cases as rc
import serving_matrix as sm
from rank_eligible_expect import eligible_ranks, expect_rows, forbidden_items, mask_list
from rank_expect import ranks_expectation
from sbr_rs_amd import _abi, _lib, evaluation
from sbr_rs_amd._abi import Status

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("sbr_rank_targets_rows", "sbr_item_set_rank_targets")


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------------
def test_the_two_entries_are_declared_exported_and_bound():
    L = _lib_loaded()
    header = open(os.path.join(HERE, "..", "include", "sbr_hip.h")).read()
    tail = "const struct sbr_scan_rows* rows, uint64_t num_rows, const uint64_t* target_ptr,\n"
    assert f"sbr_status sbr_rank_targets_rows(sbr_model* m, {tail}" in header
    assert f"sbr_status sbr_item_set_rank_targets(sbr_item_set* set, {tail}" in header
    assert "ELIGIBLE RANKS" in header
    for name in NAMES:
        fn = getattr(L, name)
        assert name in _lib.DECLARED_SYMBOLS and fn.restype is C.c_int and len(fn.argtypes) == 6, name
    assert _abi.ABI_VERSION == 13 and L.sbr_abi_version() == 13 and "#define SBR_ABI_VERSION 13u" in header  # additions only


def test_the_entries_refuse_without_a_model_a_set_or_rows():
    L = _lib_loaded()
    out = np.full(4, 7, np.uint32)
    ptr = np.zeros(2, np.uint64)
    d = _abi.SbrScanRows()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.sbr_rank_targets_rows(None, C.byref(d), 1, vp(ptr), vp(out), vp(out)) == Status.INVALID_ARGUMENT
    assert L.sbr_item_set_rank_targets(None, C.byref(d), 1, vp(ptr), vp(out), vp(out)) == Status.INVALID_ARGUMENT
    assert L.sbr_item_set_rank_targets(None, None, 1, vp(ptr), vp(out), vp(out)) == Status.INVALID_ARGUMENT
    assert np.all(out == 7)


def test_python_surface():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine

    for fn in (engine.Model.rank_targets, engine.Model.rank_targets_reps, engine.ItemSet.rank_targets, engine.ItemSet.rank_targets_reps):
        p = inspect.signature(fn).parameters
        assert p["any_of"].default is None and p["none_of"].default is None, fn
    for fn in (engine.Sessions.rank_targets, engine.ItemSetSessions.rank_targets):
        assert list(inspect.signature(fn).parameters) == ["self", "slots", "targets", "exclude", "any_of", "none_of", "include_seen"], fn
        assert inspect.signature(fn).parameters["include_seen"].default is False
    assert list(inspect.signature(engine.ItemSet.rank_targets).parameters) == list(inspect.signature(engine.Model.rank_targets).parameters)
    for fn in (evaluation.rank_targets, sbr.lstm.ImplicitLSTMModel.rank_targets):
        p = inspect.signature(fn).parameters
        assert all(p[k].default is None for k in ("any_of", "none_of", "item_set")), fn
    p = inspect.signature(evaluation.ranking_metrics).parameters
    assert p["ineligible"].default == "miss" and all(p[k].default is None for k in ("any_of", "none_of", "item_set"))
    # the plain calls go where they went: no masks, no descriptor
    src = inspect.getsource(engine.Model.rank_targets_reps)
    assert "sbr_rank_targets_reps" in src and "sbr_rank_targets_rows" in src


# ------------------------------------------------------------------------------------------------
# the expectation's own cases
# ------------------------------------------------------------------------------------------------
SCORES = np.array([0.5, 2.0, 2.0, -1.0, 3.0, 0.0, 2.0, 1.0], np.float32)
TAGS = np.array([1, 2, 3, 0, 4, 1, 2, 8], np.uint32)


def test_expectation_a_forbidden_target_has_rank_num_items():
    assert forbidden_items(TAGS, 0, 4) == {4} and forbidden_items(TAGS, 1, 0) == {1, 3, 4, 6, 7} and forbidden_items(TAGS, 0, 0) == set()
    assert eligible_ranks(SCORES, [4, 1], (), TAGS, 0, 4).tolist() == [8, 3]  # item 4 forbidden: rank 8; items 1, 2, 6 tie at the top now
    assert eligible_ranks(SCORES, [0], (), TAGS, 1, 0).tolist() == [2] and eligible_ranks(SCORES, [7], (), TAGS, 1, 0).tolist() == [8]
    assert eligible_ranks(SCORES, [0, 5], (), TAGS, 1 << 20, 0).tolist() == [8, 8]  # a mask that allows nothing


def test_expectation_a_target_outside_the_set_has_the_catalogues_num_items():
    S = [0, 1, 5, 7]
    assert mask_list(8, (), members=S) == {2, 3, 4, 6}
    assert eligible_ranks(SCORES, [4, 1, 7, 0, 5], members=S).tolist() == [8, 1, 2, 3, 4]
    assert eligible_ranks(SCORES, [1], [1, 1, 7], members=S).tolist() == [8]  # listed, repeats or not


def test_expectation_ties_count_against_the_target_and_duplicates_agree():
    assert eligible_ranks(SCORES, [1, 2, 6, 1]).tolist() == [4, 4, 4, 4]
    assert eligible_ranks(SCORES, [1], [2]).tolist() == [3] and eligible_ranks(SCORES, [1], [2], TAGS, 0, 2).tolist() == [8]
    # a listed item that is also forbidden leaves the count once
    assert eligible_ranks(SCORES, [7], [4, 4], TAGS, 0, 4).tolist() == [4]


def test_expectation_zero_masks_without_a_set_is_the_plain_statement():
    rs = np.random.RandomState(3)
    scores = rs.randn(5, 40).astype(np.float32)
    targets = [rs.randint(0, 40, n) for n in (0, 1, 3, 7, 2)]
    lists = [rs.randint(0, 40, n) for n in (4, 0, 9, 1, 40)]
    tags = rs.randint(0, 16, 40).astype(np.uint32)
    zero = np.zeros(5, np.uint32)
    want = np.concatenate([ranks_expectation(scores[u], np.unique(lists[u]), targets[u]) for u in range(5)])
    assert np.array_equal(expect_rows(scores, targets, lists, tags, zero, zero), want)
    assert np.array_equal(expect_rows(scores, targets, lists, members=np.arange(40)), want)
    assert expect_rows(scores, [[]] * 5).size == 0


# ------------------------------------------------------------------------------------------------
# ranking_metrics' "miss" / "skip" and eligible_targets
# ------------------------------------------------------------------------------------------------
def test_miss_and_skip_on_hand_made_ranks():
    ranks = [np.array([1, 50, 3]), np.array([50]), np.array([2, 4]), np.array([], np.int64)]
    eligible = [np.array([True, False, True]), np.array([False]), np.array([True, True]), np.array([], bool)]
    rows, skipped = evaluation.apply_ineligible(ranks, eligible, "miss")
    assert skipped == 0 and [r.tolist() for r in rows] == [[1, 50, 3], [50], [2, 4], []]
    miss = evaluation.ranking_metrics_from_ranks(rows, ks=(2,))
    assert miss["num_users_ranked"] == 3 and miss["hit_rate"][2] == pytest.approx(2 / 3) and miss["recall"][2] == pytest.approx((1 / 3 + 0 + 1 / 2) / 3)
    assert miss["mrr"] == pytest.approx((1 + 1 / 50 + 1 / 2) / 3)
    rows, skipped = evaluation.apply_ineligible(ranks, eligible, "skip")
    assert skipped == 2 and [r.tolist() for r in rows] == [[1, 3], [], [2, 4], []]
    skip = evaluation.ranking_metrics_from_ranks(rows, ks=(2,))
    assert skip["num_users_ranked"] == 2 and skip["users"].tolist() == [0, 2]  # the user left without targets is not ranked
    assert skip["hit_rate"][2] == 1.0 and skip["recall"][2] == pytest.approx((1 / 2 + 1 / 2) / 2) and skip["mrr"] == pytest.approx((1 + 1 / 2) / 2)
    assert skip["mean_rank"] == pytest.approx((2 + 3) / 2)
    with pytest.raises(ValueError):
        evaluation.apply_ineligible(ranks, eligible, "drop")
    with pytest.raises(ValueError):
        evaluation.apply_ineligible(ranks, eligible[:2], "skip")
    with pytest.raises(ValueError):
        evaluation.ranking_metrics(None, None, ineligible="drop")


class _Tags:
    def __init__(self, tags):
        self._tags = tags

    def item_tags(self):
        return self._tags


class _Set:
    def __init__(self, items):
        self.items = np.asarray(items, np.uint32)


def test_eligible_targets_against_the_sets():
    rs = np.random.RandomState(11)
    n = 60
    tags = rs.randint(0, 16, n).astype(np.uint32)
    tags[5] = 0
    hist = [rs.randint(0, n, k) for k in (0, 3, 10, 25)]
    targets = [rs.randint(0, n, k) for k in (4, 0, 12, 30)]
    any_of = np.array([0, 3, 8, 5], np.uint32)
    none_of = np.array([4, 0, 1, 2], np.uint32)
    S = np.array(sorted(rs.choice(n, 35, replace=False)), np.uint32)
    model = _Tags(tags)
    for members in (None, S):
        for mask_history in (True, False):
            got = evaluation.eligible_targets(model, hist, targets, mask_history=mask_history, any_of=any_of, none_of=none_of,
                                              item_set=None if members is None else _Set(members))
            for u in range(4):
                m = mask_list(n, hist[u] if mask_history else (), tags, any_of[u], none_of[u], members)
                assert got[u].dtype == bool and got[u].tolist() == [int(t) not in m for t in targets[u]], (u, mask_history)
    # scalars apply to every user; no masks needs no tags
    got = evaluation.eligible_targets(model, hist, targets, any_of=3)
    assert got[2].tolist() == [int(t) not in mask_list(n, hist[2], tags, 3, 0) for t in targets[2]]
    assert all(g.all() for g in evaluation.eligible_targets(object(), hist, targets, mask_history=False))
    # the ranks agree: a target is in M exactly when its expected rank is num_items (scores without ties at the bottom)
    scores = rs.randn(4, n).astype(np.float32)
    want = [eligible_ranks(scores[u], targets[u], hist[u], tags, any_of[u], none_of[u], S) for u in range(4)]
    got = evaluation.eligible_targets(model, hist, targets, any_of=any_of, none_of=none_of, item_set=_Set(S))
    for u in range(4):
        assert ((want[u] == n) == ~got[u]).all()


# ------------------------------------------------------------------------------------------------
# the roster
# ------------------------------------------------------------------------------------------------
def test_roster_every_instantiation_is_named_by_a_case_and_no_case_names_a_missing_one():
    _lib_loaded()
    have = rc.library_instantiations()
    assert len(have) == 3 * len(sm.WIDTHS), sorted(have)  # the three templates at the five stored widths
    assert have - rc.claimed() == set(), "instantiations no case at an exact width names"
    assert rc.named() - have == set(), "cases name instantiations the library lacks"
    assert not any(n.split("<", 1)[0] in rc.TEMPLATES for n in sm.roster()), "the serving matrix's roster is what it was"
    assert all(t not in sm.serving_templates() for t in rc.TEMPLATES)
