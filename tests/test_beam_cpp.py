"""GPU: the beam-search calls through the C++ host layer (sbr::Sessions::beam_search and ImplicitSequenceModel::beam_search in
include/sbr.hpp, tests/cpp/beam_tests.cpp): the program asserts that they return what the C entry point returns, that the store is
left as it was and that the model-level convenience is its defining sequence of calls; it then writes its model's parameters, its
histories, lists and result, and the Python binding must return the same bits for the same model and arguments."""
import os
import subprocess

import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams
from sbr_rs_amd import build as hip_build
from sbr_rs_amd._abi import ModelKind, Param


def test_cpp_program_builds_without_a_device():
    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_beam_tests(verbose=False))


@pytest.mark.gpu
def test_cpp_beam_search_matches_the_entry_point_and_python(tmp_path):
    from sbr_rs_amd.engine import Model

    binary = hip_build.build_beam_tests(verbose=False)
    p = subprocess.run([binary, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "lstm normal d=48: sessions=40 width=4 steps=5 beam_search ok" in p.stdout, p.stdout

    def load(name, dtype):
        return np.fromfile(os.path.join(tmp_path, name), dtype=dtype)

    g = Model(hparams(300, 8, 48, int(ModelKind.LSTM_NORMAL), LOSS_HINGE, B=8))
    for which, name in ((Param.ITEM_EMBEDDING, "E.f32"), (Param.ITEM_BIAS, "b.f32"), (Param.LSTM_W, "W.f32"), (Param.LSTM_B, "B.f32")):
        g.set_param(which, load(name, np.float32))
    hp, hi = load("hist_ptr.u64", np.uint64), load("hist_items.u32", np.uint32)
    ep, ei = load("excl_ptr.u64", np.uint64), load("excl_items.u32", np.uint32)
    n = hp.size - 1
    st = g.sessions(n + 2)
    slots = np.arange(n, dtype=np.uint32)
    st.append(slots, [hi[hp[u]:hp[u + 1]] for u in range(n)])
    r = st.beam_search(slots, 5, width=4, temperature=0.75, exclude=[ei[ep[u]:ep[u + 1]] for u in range(n)], partitions=True)
    st.close()
    shape = (n, 4, 5)
    assert np.array_equal(r.items, load("items.u32", np.uint32).reshape(shape))
    for f, name in (("scores", "scores.f32"), ("step_log_probs", "step_lp.f32"), ("shift", "shift.f32")):
        assert np.array_equal(getattr(r, f).view(np.uint32), load(name, np.uint32).reshape(shape)), f
    assert np.array_equal(r.log_probs.view(np.uint32), load("cum.f32", np.uint32).reshape(n, 4))
    assert np.array_equal(r.mass, load("mass.u64", np.uint64).reshape(shape))
    assert np.array_equal(r.lengths, load("lengths.u32", np.uint32)) and np.array_equal(r.beams, load("beams.u32", np.uint32))
