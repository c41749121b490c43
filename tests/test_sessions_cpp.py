"""GPU: the C++ host layer's session store (sbr::Sessions in include/sbr.hpp, tests/cpp/sessions_tests.cpp): three ways of
appending 70 histories give the bits of user_representations, and recommend / score_candidates on the store equal the calls on
the histories, for an LSTM of each variant and EWMA.  The program asserts; the harness checks that it ran all three models."""
import os
import subprocess

import pytest

from sbr_rs_amd import build as hip_build


def test_cpp_program_builds_without_a_device():
    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_sessions_tests(verbose=False))


@pytest.mark.gpu
def test_cpp_sessions_match_the_histories():
    binary = hip_build.build_sessions_tests(verbose=False)
    p = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    for name in ("lstm normal d=48", "lstm coupled d=128", "ewma d=20"):
        assert f"{name}: sessions=70" in p.stdout, p.stdout
