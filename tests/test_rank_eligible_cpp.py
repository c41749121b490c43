"""GPU: the C++ host layer's rank_targets under a serving policy (include/sbr.hpp, tests/cpp/rank_eligible_tests.cpp): the model's
overload with a TagFilter, ItemSet::rank_targets, Sessions::rank_targets and ItemSet::on(store).rank_targets return the ranks of
the C call the contract names, and ranking_metrics under a policy skips exactly the targets the policy can never show.  The
program checks itself; a small synthetic model, no data set."""
import subprocess

import pytest

from sbr_rs_amd import build as hip_build


@pytest.mark.gpu
def test_cpp_eligible_ranks_match_the_c_calls():
    hip_build.build(verbose=False)
    binary = hip_build.build_rank_eligible_tests(verbose=False)
    p = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "skipped=" in p.stdout
