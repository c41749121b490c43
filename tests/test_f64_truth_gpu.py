"""The engine's training step against the float64 model of DESIGN.md §2 (tests/f64_model.py), on the GPU.

The same case table and the same comparison as tests/test_f64_truth.py, with `engine.Model` in the oracle's place: the
kernels are held to float64 directly and not through the oracle, which this file does not import.  Every kernel-form switch
selects a different kernel for the same mathematics, so each form is compared too.
"""
import pytest

from f64_cases import CASE_BY_NAME, CASES, run_case
from helpers import OPT_ADAGRAD
from sbr_rs_amd.engine import Model

pytestmark = pytest.mark.gpu


class EngineDriver:
    @staticmethod
    def make(hp):
        return Model(hp)

    @staticmethod
    def opt_steps(model):
        return model.counters()[1]

    @staticmethod
    def step_local(plan, mb):
        plan.step_local(mb)

    @staticmethod
    def step_apply(plan, mb):
        plan.step_apply(mb)

    @staticmethod
    def step(plan, mb):
        plan.steps(mb, 1)


def _run(case_name, **kw):
    rep = run_case(CASE_BY_NAME[case_name], EngineDriver, **kw)
    print("\n".join(rep.lines()))
    assert not rep.failures, "\n".join(rep.failures)
    return rep


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_engine_step_matches_float64(case):
    _run(case.name)


@pytest.mark.parametrize("wave", ["0", "1"])
@pytest.mark.parametrize("case", ["normal-hinge-16", "coupled-warp-24", "normal-hinge-32-single", "normal-bpr-1"])
def test_wave_and_tile_forms(monkeypatch, case, wave):
    """d <= 32, small steps: one wave per sequence on the vector ALU (SBR_WAVE = 1) or the MFMA tile kernels (0)."""
    monkeypatch.setenv("SBR_WAVE", wave)
    _run(case)


@pytest.mark.parametrize("rt", ["1", "2", "4"])
@pytest.mark.parametrize("case", ["normal-hinge-128-large", "coupled-bpr-64-equal"])
def test_sequence_tile_sizes(monkeypatch, case, rt):
    """The sequence-resident kernels on 16-, 32- and 64-sequence tiles (SBR_SEQ_RT)."""
    monkeypatch.setenv("SBR_SEQ_RT", rt)
    _run(case)


@pytest.mark.parametrize("min_tiles", ["1", "1000000"])
@pytest.mark.parametrize("case", ["coupled-warp-256"])
def test_d256_bptt_forms(monkeypatch, case, min_tiles):
    """d = 256 BPTT: the sequence-resident kernel or the per-step launches (SBR_BWD256_MIN_TILES)."""
    monkeypatch.setenv("SBR_BWD256_MIN_TILES", min_tiles)
    _run(case)


@pytest.mark.parametrize("u", ["1", "2"])
@pytest.mark.parametrize("case", ["ewma-warp-64", "normal-warp-64", "coupled-warp-256"])
def test_warp_score_rows_per_group(monkeypatch, case, u):
    monkeypatch.setenv("SBR_SCORE_U", u)
    _run(case)


@pytest.mark.parametrize("stream", ["0", "1"])
@pytest.mark.parametrize("case", ["ewma-warp-64", "normal-hinge-128-large", "ewma-hinge-256"])
def test_streaming_and_cached_gathers(monkeypatch, case, stream):
    monkeypatch.setenv("SBR_STREAM", stream)
    _run(case)


@pytest.mark.parametrize("fusion", [0, 1, 2])
@pytest.mark.parametrize("case", ["ewma-hinge-32-single", "normal-hinge-32-single", "ewma-bpr-16-single"])
def test_one_sequence_step_launches(case, fusion):
    """One sequence per step at d <= 32 through the plan's own step: separate launches (0), fused launches (1), runs of
    steps in one launch where the shape allows (2: EWMA and LSTM Normal with Adagrad; the Adam case takes the fused ones)."""
    rep = _run(case, whole_step=True, setup=lambda m: m.set_step_fusion(fusion))
    one_launch = fusion == 2 and CASE_BY_NAME[case].opt == OPT_ADAGRAD
    assert rep.one_launch_steps == (3 if one_launch else 0)   # the form asked for is the form that ran
