"""GPU: replay of a session store through the C++ host layer (sbr::Sessions::replay in include/sbr.hpp,
tests/cpp/sessions_replay_tests.cpp): after every parameter block of the model changes, a stale store with seen-item memory is
replayed on the device and holds, bit for bit, what a new store holds after append of the remembered items, for an LSTM of each
variant and EWMA.  The program asserts; the harness checks that it ran all three models."""
import os
import subprocess

import pytest

from sbr_rs_amd import build as hip_build


def test_cpp_program_builds_without_a_device():
    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_sessions_replay_tests(verbose=False))


@pytest.mark.gpu
def test_cpp_replay_matches_append_on_a_fresh_store():
    binary = hip_build.build_sessions_replay_tests(verbose=False)
    p = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    for name in ("lstm normal d=48", "lstm coupled d=128", "ewma d=20"):
        assert f"{name}: slots=70 replayed=6 replay ok" in p.stdout, p.stdout
