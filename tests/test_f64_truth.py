"""The oracle's training step against the float64 model of DESIGN.md §2 (tests/f64_model.py), on the CPU.

Every GPU parity test holds the engine to the oracle bit for bit; this file (and tests/test_f64_truth_gpu.py for the engine
itself) holds the oracle to a reference that shares none of its code: torch float64 autograd for the graph, numpy float64
for the optimiser.  The mutant tests show that the comparison can fail: each plants one plausible misreading of the
contract in the float64 model and must be caught, with a gap of at least 10x over the bound.  The second half does the same
for the world-N group step and the staleness-one pipeline of DESIGN.md §8, which are the identity at one device.
"""
import numpy as np
import pytest

import f64_model as F
from f64_cases import (CASE_BY_NAME, CASES, WORLD_CASE_BY_NAME, WORLD_CASES, run_case, run_partition_check, run_world_case,
                       world_hparams)
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


# ---------------------------------------------------------------- world N -----------------------------------------------------
class OracleWorld:
    """What run_world_case drives: `replicas` (the models whose state is seeded and read), the local halves of every device,
    their debug blocks, and the exchange + update.  Here: ONE oracle model that emulates the N devices, its step through the
    protocol halves in the order DESIGN.md §8 states (the oracle's one-call step_apply is the one-device form).  Synchronous:
    exchange = scatter + apply.  Pipeline: run_world_case calls scatter(k), step_local(k + 1), apply(k)."""
    keeps_dhidden = True

    def __init__(self, case, ptr, items):
        self.n = case.world
        self.model = OracleModel(world_hparams(case))
        self.replicas = [self.model]
        self.plan = self.model.fit_begin(ptr, items)

    def epoch_prepare(self):
        return self.plan.epoch_prepare()

    def rows(self, mb, q):
        return self.plan.minibatch_rows(mb, device=q)

    def step_local(self, mb):
        for q in range(self.n):
            self.plan.compute_local(mb, q)

    def debug_fetch(self, q, which, rows):
        return self.plan.debug_fetch(which, rows, device=q)

    def scatter(self, mb):
        self._send = [self.plan.scatter(q, self.n) for q in range(self.n)]
        self._dense = np.concatenate([self.plan.export_dense(q) for q in range(self.n)])

    def apply(self, mb):
        c = self.plan.chunk_bytes()
        own = [self.plan.owner_reduce(np.concatenate([s[p * c:(p + 1) * c] for s in self._send])) for p in range(self.n)]
        self.plan.apply_table(np.concatenate(own), self._dense)

    def exchange(self, mb):
        self.scatter(mb)
        self.apply(mb)

    def gather_state(self):
        pass

    @staticmethod
    def opt_steps(model):
        return model.optimizer_steps()

    def end(self):
        return self.plan.end()[0]

    def close(self):
        self.plan.close()


@pytest.mark.parametrize("case", WORLD_CASES, ids=[c.name for c in WORLD_CASES])
def test_oracle_world_step_matches_float64(oracle_lib, case):
    rep = run_world_case(case, OracleWorld)
    print("\n".join(rep.lines()))
    print(f"{case.name}: worst e / bound " + ", ".join(f"{c} {max((en[3] / en[6] for en in rep.entries if en[2] == c), default=0):.3g}"
                                                       for c in ("forward", "rowgrad", "dense", "param")))
    assert not rep.failures, "\n".join(rep.failures)


class OracleWorldWholeStep(OracleWorld):
    """The update through the oracle's own group step (what its `fit` calls): it runs the local halves again, on unchanged
    parameters, and then the same exchange."""

    def exchange(self, mb):
        self.plan.step(mb)


@pytest.mark.parametrize("case", ["w2-normal-hinge-16", "w4-coupled-bpr-24-adam", "w9-ewma-warp-32"])
def test_oracle_world_whole_step_entry_point_matches_float64(oracle_lib, case):
    rep = run_world_case(WORLD_CASE_BY_NAME[case], OracleWorldWholeStep)
    assert not rep.failures, "\n".join(rep.failures)


@pytest.mark.parametrize("case", WORLD_CASES, ids=[c.name for c in WORLD_CASES])
def test_oracle_partitions_drop_the_remainder(oracle_lib, case):
    rep = run_partition_check(case, OracleWorld)
    assert not rep.failures, "\n".join(rep.failures)


# world mutant -> the case that must catch it (against the unmutated oracle)
WORLD_MUTANT_CASE = {
    "mean_over_devices": "w3-ewma-warp-64",
    "update_per_device": "w2-normal-hinge-16",
    "accumulator_of_per_device_squares": "w8-normal-warp-128",
    "l2_per_device": "w9-ewma-warp-32",
    "adam_t_counts_devices": "w4-coupled-bpr-24-adam",
    "remainder_kept": "w3-ewma-warp-64",
    "pipeline_fresh_gradient": "pipe-w2-normal-warp-64",
    "pipeline_stale_by_two": "pipe-w3-ewma-hinge-32",
}


def test_every_world_mutation_has_a_case():
    assert set(WORLD_MUTANT_CASE) == set(F.WORLD_MUTATIONS)


@pytest.mark.parametrize("mutation", F.WORLD_MUTATIONS)
def test_world_mutant_is_caught(oracle_lib, mutation):
    case = WORLD_CASE_BY_NAME[WORLD_MUTANT_CASE[mutation]]
    run = run_partition_check if mutation == "remainder_kept" else run_world_case
    rep = run(case, OracleWorld, mutation=mutation)
    print(f"{mutation}: worst e / bound = {rep.worst_ratio():.3g}; {len(rep.failures)} failed checks")
    assert rep.failures, f"{mutation} passes: the world case table has a gap"
    assert rep.worst_ratio() >= 10.0, f"{mutation}: e exceeds the bound by {rep.worst_ratio():.3g}x only"
