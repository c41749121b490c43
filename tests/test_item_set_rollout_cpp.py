"""Rollout and beam search within an item set through the C++ host layer (sbr::ItemSet::OnSessions::rollout / beam_search and the
histories forms sbr::ItemSet::rollout / beam_search in include/sbr.hpp, tests/cpp/item_set_rollout_tests.cpp): for one LSTM and one
EWMA model the program asserts that the OnSessions methods return what the C entry points return, that this equals the store's own
call with the set's complement appended to every exclusion list, and that the histories forms are their defining sequence of calls."""
import os
import subprocess

import pytest

from sbr_rs_amd import build as hip_build


def test_cpp_program_builds_without_a_device():
    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_item_set_rollout_tests(verbose=False))


@pytest.mark.gpu
def test_cpp_item_set_rollout_and_beam_search_match_the_entry_points_and_the_complement_route():
    binary = hip_build.build_item_set_rollout_tests(verbose=False)
    p = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    for name in ("lstm normal d=48", "ewma d=20"):
        assert f"{name}: sessions=40 set=103 rollout and beam_search within the set ok" in p.stdout, p.stdout
