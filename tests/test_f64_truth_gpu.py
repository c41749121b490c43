"""The engine's training step against the float64 model of DESIGN.md §2 (tests/f64_model.py), on the GPU.

The same case table and the same comparison as tests/test_f64_truth.py, with `engine.Model` in the oracle's place: the
kernels are held to float64 directly and not through the oracle, which this file does not import.  Every kernel-form switch
selects a different kernel for the same mathematics, so each form is compared too.  The world-N cases go through
every production form of the group step: the C-ABI halves of one process per GPU in both exchanges, the single-process group
(replicated in both exchanges, partitioned), and the staleness-one pipeline through the halves.
"""
import pytest

from f64_cases import (CASE_BY_NAME, CASES, WORLD_CASE_BY_NAME, WORLD_CASES, run_case, run_partition_check, run_world_case,
                       world_hparams)
from helpers import OPT_ADAGRAD
from sbr_rs_amd.engine import GroupPlan, Model, group_create
from simulated_ranks import SimulatedRanks

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


# ---------------------------------------------------------------- world N -----------------------------------------------------
SYNC_WORLD = [c.name for c in WORLD_CASES if not c.pipeline]
PIPE_WORLD = [c.name for c in WORLD_CASES if c.pipeline]


class RanksWorld:
    """run_world_case's driver over one model and plan per rank and tests/simulated_ranks.py (the C-ABI halves of the one-
    process-per-GPU protocol, tensor copies for the collectives).  exchange: the Synchronous step's form.  The pipeline: per
    rank step_scatter(k) and step_dense, then step_local(k + 1) on every rank, then the gradient exchange of step k."""
    keeps_dhidden = True

    def __init__(self, case, ptr, items, exchange="owner"):
        self.n, self.form = case.world, exchange
        self.replicas = [Model(world_hparams(case, q)) for q in range(self.n)]
        self.plans = [m.fit_begin(ptr, items) for m in self.replicas]
        self.ranks = SimulatedRanks(self.replicas, self.plans)

    def epoch_prepare(self):
        nmb = {p.epoch_prepare() for p in self.plans}
        assert len(nmb) == 1
        return nmb.pop()

    def rows(self, mb, q):
        return self.plans[q].minibatch_rows(mb)

    def step_local(self, mb):
        for p in self.plans:
            p.step_local(mb)

    def debug_fetch(self, q, which, rows):
        return self.plans[q].debug_fetch(which, rows)

    def exchange(self, mb):
        self.ranks.exchange(mb, self.form)

    def scatter(self, mb):
        for q in range(self.n):
            self.plans[q].step_scatter(mb, self.ranks.send[q].data_ptr())
            self.plans[q].step_dense(self.ranks.dense[q].data_ptr())
            self.replicas[q].synchronize()

    def apply(self, mb):
        self.ranks.exchange(mb, "gradient", scatter=False)

    def gather_state(self):
        self.ranks.finish()

    @staticmethod
    def opt_steps(model):
        return model.counters()[1]

    def end(self):
        losses = [p.end()[0] for p in self.plans]
        assert all(v == losses[0] for v in losses)
        return losses[0]

    def close(self):
        for p in self.plans:
            p.close()


class GroupWorld:
    """run_world_case's driver over the single-process group: step_local, the members' debug blocks, then step."""
    keeps_dhidden = True

    def __init__(self, case, ptr, items, partition=False, gradient=False, host_threads=None):
        self.n = case.world
        self.replicas = group_create(world_hparams(case), self.n, partition_item_table=partition)
        assert all(m.is_partitioned() == partition for m in self.replicas)
        self.gp = GroupPlan(self.replicas, ptr, items, host_threads=host_threads)
        if not partition:
            self.gp.set_exchange(gradient)
        self.threads = None

    def epoch_prepare(self):
        return self.gp.epoch_prepare()

    def rows(self, mb, q):
        return self.gp.member(q).minibatch_rows(mb)

    def step_local(self, mb):
        self.gp.step_local(mb)
        self.gp.synchronize()

    def debug_fetch(self, q, which, rows):
        return self.gp.member(q).debug_fetch(which, rows)

    def exchange(self, mb):
        self.gp.step(mb)
        self.gp.synchronize()

    def gather_state(self):
        self.gp.gather_optimizer_state()

    @staticmethod
    def opt_steps(model):
        return model.counters()[1]

    def end(self):
        self.threads = self.gp.stats()[2]
        return self.gp.end()

    def close(self):
        self.gp.close()


def _run_world(case_name, driver, **kw):
    made = []

    def make(case, ptr, items):
        made.append(driver(case, ptr, items, **kw))
        return made[0]

    rep = run_world_case(WORLD_CASE_BY_NAME[case_name], make)
    print("\n".join(rep.lines()))
    print(f"{case_name}: worst e / bound " + ", ".join(f"{c} {max((en[3] / en[6] for en in rep.entries if en[2] == c), default=0):.3g}"
                                                       for c in ("forward", "rowgrad", "dense", "param")))
    assert not rep.failures, "\n".join(rep.failures)
    return made[0]


@pytest.mark.parametrize("exchange", ["owner", "gradient"])
@pytest.mark.parametrize("case", SYNC_WORLD)
def test_world_step_through_the_rank_halves(case, exchange):
    """scatter -> owner_update -> in-place all-gather of the parameter slices -> dense blocks ("owner"; the optimiser state is
    gathered after every step and the owner updates go on from it), or scatter -> owner_reduce -> apply_table ("gradient")."""
    _run_world(case, RanksWorld, exchange=exchange)


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("case", SYNC_WORLD)
def test_world_step_through_the_group_plan(case, gradient):
    """The single-process group over replicated models, owner-applied and with the gradient all-gather."""
    _run_world(case, GroupWorld, gradient=gradient)


@pytest.mark.parametrize("threads", [True, False])
def test_world_step_group_plan_host_threads(threads):
    drv = _run_world("w4-coupled-bpr-24-adam", GroupWorld, host_threads=threads)
    assert drv.threads == (4 if threads else 1)   # the form asked for is the form that ran


@pytest.mark.parametrize("case", ["w2-normal-hinge-16", "w3-ewma-warp-64", "w9-ewma-warp-32"])
def test_world_step_over_a_partitioned_table(case):
    """The item table stored once: every owner merges the devices' gradient lists over its rows (2, 3 and more than 8 owners)."""
    _run_world(case, GroupWorld, partition=True)


@pytest.mark.parametrize("case", PIPE_WORLD)
def test_world_pipeline_through_the_rank_halves(case):
    _run_world(case, RanksWorld)


@pytest.mark.parametrize("driver,kw,case", [(RanksWorld, {}, "w3-ewma-warp-64"), (GroupWorld, {}, "w8-normal-warp-128"),
                                           (GroupWorld, {"partition": True}, "w9-ewma-warp-32")],
                         ids=["ranks-w3", "group-w8", "partitioned-w9"])
def test_partitions_drop_the_remainder(driver, kw, case):
    rep = run_partition_check(WORLD_CASE_BY_NAME[case], lambda c, ptr, items: driver(c, ptr, items, **kw))
    assert not rep.failures, "\n".join(rep.failures)
