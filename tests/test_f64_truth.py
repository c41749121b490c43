"""The oracle's training step against the float64 model of DESIGN.md §2 (tests/f64_model.py), on the CPU.

Every GPU parity test holds the engine to the oracle bit for bit; this file (and tests/test_f64_truth_gpu.py for the engine
itself) holds the oracle to a reference that shares none of its code: torch float64 autograd for the graph, numpy float64
for the optimiser.  The mutant tests show that the comparison can fail: each plants one plausible misreading of the
contract in the float64 model and must be caught, with a gap of at least 10x over the bound.
"""
import numpy as np
import pytest

import f64_model as F
from f64_cases import CASE_BY_NAME, CASES, run_case
from oracle.oracle import OracleModel


class OracleDriver:
    @staticmethod
    def make(hp):
        return OracleModel(hp)

    @staticmethod
    def opt_steps(model):
        return model.optimizer_steps()

    @staticmethod
    def step_local(plan, mb):
        plan._block = plan.step_local(mb)

    @staticmethod
    def step_apply(plan, mb):
        plan.step_apply(plan._block)

    @staticmethod
    def step(plan, mb):
        plan.step(mb)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_step_matches_float64(oracle_lib, case):
    rep = run_case(case, OracleDriver)
    print("\n".join(rep.lines()))
    assert not rep.failures, "\n".join(rep.failures)


def test_whole_step_entry_point_matches_float64(oracle_lib):
    """The same comparison through `step` (both halves in one call), the form the GPU file uses for the fused launches."""
    rep = run_case(CASE_BY_NAME["ewma-bpr-16-single"], OracleDriver, whole_step=True)
    assert not rep.failures, "\n".join(rep.failures)


# mutant -> the case that must catch it (against the unmutated oracle)
MUTANT_CASE = {
    "bias_touched_by_inputs": "coupled-bpr-16",
    "l2_needs_data_gradient": "normal-hinge-16",
    "mean_over_sequences": "coupled-warp-24",
    "update_per_occurrence": "coupled-bpr-64-equal",
    "no_input_row_path": "ewma-bpr-16",
    "hinge_without_one": "ewma-hinge-16",
    "ewma_first_step_scaled": "ewma-warp-64",
    "coupled_f_from_i": "coupled-hinge-100",
    "adam_decays_untouched_rows": "coupled-bpr-16",
    "adam_bias_step_off_by_one": "ewma-bpr-200",
}


def test_every_mutation_has_a_case():
    assert set(MUTANT_CASE) == set(F.MUTATIONS)


@pytest.mark.parametrize("mutation", F.MUTATIONS)
def test_mutant_is_caught(oracle_lib, mutation):
    rep = run_case(CASE_BY_NAME[MUTANT_CASE[mutation]], OracleDriver, mutation=mutation)
    print(f"{mutation}: worst e / bound = {rep.worst_ratio():.3g}; {len(rep.failures)} failed checks")
    assert rep.failures, f"{mutation} passes: the case table has a gap"
    assert rep.worst_ratio() >= 10.0, f"{mutation}: e exceeds the bound by {rep.worst_ratio():.3g}x only"
