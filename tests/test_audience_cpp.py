"""GPU: the audience scan through the C++ host layer (Sessions::audience, ImplicitSequenceModel::audience_reps / audience in
include/sbr.hpp, tests/cpp/audience_tests.cpp): every facade call gives the rows of the C call it wraps, bit for bit, for an LSTM
and EWMA.  The program asserts; the harness checks that it ran both models."""
import subprocess

import pytest

from sbr_rs_amd import build as hip_build


@pytest.mark.gpu
def test_cpp_audience_matches_the_c_calls():
    binary = hip_build.build_audience_tests(verbose=False)
    p = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    for name in ("lstm normal d=48", "ewma d=20"):
        assert f"{name}: sessions=70 queries=40 audience ok" in p.stdout, p.stdout
