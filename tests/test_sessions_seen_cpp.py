"""GPU: the seen-item memory through the C++ host layer (sbr::Sessions with a seen_capacity in include/sbr.hpp,
tests/cpp/sessions_seen_tests.cpp): a store that remembers its slots' items answers recommend as the model answers the histories,
bit for bit, however they were appended, and state + seen restore a slot exactly into another store, for an LSTM of each variant
and EWMA.  The program asserts; the harness checks that it ran all three models."""
import os
import subprocess

import pytest

from sbr_rs_amd import build as hip_build


def test_cpp_program_builds_without_a_device():
    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_sessions_seen_tests(verbose=False))


@pytest.mark.gpu
def test_cpp_seen_memory_matches_the_histories():
    binary = hip_build.build_sessions_seen_tests(verbose=False)
    p = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    for name in ("lstm normal d=48", "lstm coupled d=128", "ewma d=20"):
        assert f"{name}: sessions=40" in p.stdout and "seen ok" in p.stdout, p.stdout
