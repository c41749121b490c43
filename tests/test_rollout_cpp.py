"""GPU: the rollout calls through the C++ host layer (sbr::Sessions::rollout and ImplicitSequenceModel::rollout in include/sbr.hpp,
tests/cpp/rollout_tests.cpp): they return what the C entry point returns, the greedy rows are the host loop's, the store is left
as it was, and the model-level convenience is its defining sequence of calls, for an LSTM of each variant and EWMA.  The program
asserts; the harness checks that it ran all three models."""
import os
import subprocess

import pytest

from sbr_rs_amd import build as hip_build


def test_cpp_program_builds_without_a_device():
    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_rollout_tests(verbose=False))


@pytest.mark.gpu
def test_cpp_rollout_matches_the_entry_point_and_the_host_loop():
    binary = hip_build.build_rollout_tests(verbose=False)
    p = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    for name in ("lstm normal d=48", "lstm coupled d=128", "ewma d=20"):
        assert f"{name}: sessions=40 steps=6 rollout ok" in p.stdout, p.stdout
