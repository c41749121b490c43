"""The cross-stream joins of the training step, tested by making one stream LATE at a time.

A training step is spread over three or four streams per model (main, side, sorter, copier; sbr_fit_step_local /
sbr_fit_step_apply) and one exchange stream per member of a group (xs), tied together by events.  A missing or misplaced wait
changes no bit unless the timing happens to go the wrong way, and at the suite's shapes it almost never does.  The test hook
SBR_TEST_STREAM_DELAY (include/sbr_hip.h) queues a bounded delay kernel behind every cross-stream wait the engine
issues on a named stream and at the head of a call's first work on it: a consumer that really waits for the late stream is
unaffected, one that does not reads stale data and loses bit-parity with the oracle.  test_a_missing_join_is_visible is the
evidence that the method sees a missing join at all.

Every run is compared with the CPU oracle bit for bit (parameters, optimiser state, the lagged loss figure, the hidden states and
the dense gradient between the two halves of a step, MRR ranks, predictions, top-10 recommendations; the returned loss is an
order-free f64 sum on the engine's side and is held to rel 1e-6 as everywhere in the suite).  The switch-invariance cases are
compared with the same expectation, which the default run (no delay, no switch) is compared with as well: equal to the oracle's
bits is equal to the default run's bits.

The shape (tests/stream_join_cases.py) is the smallest at which the whole schedule engages; test_shape_engages_the_whole_schedule
asserts that from the indices.  The MIXED data set ends every epoch with a step that stays on the main stream, so that what one step
leaves for the next (the events the main stream has not joined) crosses a change of form in both directions.

Limits.  The group cases run world 2 on ONE GPU: two models' eight or more streams over the process's four hardware queues may
still share a queue, and a queue serialises what it carries whatever the events say, so a pass there bounds less than the
one-device cases do (three or four streams on four queues).  World 2 keeps the stream count lowest.  No multi-GPU run backs the
group cases.

Found by this file: with a partitioned table and replica 1's main stream late, mrr_score on replica 0 right behind the last
sbr_group_step ranked against rows that owner 1 had not updated yet (test_group_late_stream_changes_no_bit[partitioned-main@1-*]):
the rows of a partitioned table are written on their owners' streams, and a reader on another replica's stream joined nothing.
Readers of the table now wait for the other owners' `applied` events (join_table_owners, sbr_engine.hip).

The delay (DELAY_US).  Step times measured on an MI355X with overlap off and every family bracketed (the sum over the families of
sbr_model_timing_read, per step; profiles/stream_delay_shapes.md):

    normal-warp-32 0.48 ms   coupled-hinge-16 0.19 ms   ewma-bpr-32 0.20 ms   ewma-warp-16 0.18 ms
    normal-warp-256 0.57 ms   normal-hinge-32-adam 0.20 ms

The largest is 0.57 ms; four times that is 2.3 ms; DELAY_US = 3 000, under the engine's clamp of 5 000.  A late stream is then
late by more than everything that could hide it.  test_undelayed_step_times prints the figures again.
"""
import os

import numpy as np
import pytest

import stream_join_cases as S
from helpers import PAR_ASYNC, PAR_SYNC
from sbr_rs_amd._abi import Debug
from sbr_rs_amd.engine import STREAM_ROLES, GroupPlan, Model, group_create, selftest_stream_delay

pytestmark = pytest.mark.gpu

DELAY_US = 3000
STEPS = S.EPOCHS * S.STEPS_PER_EPOCH
VAR = "SBR_TEST_STREAM_DELAY"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    if a.dtype == np.float32:
        bad = np.flatnonzero(bits(a).ravel() != bits(b).ravel())
        if bad.size:
            i = bad[0]
            raise AssertionError(f"{what}: {bad.size}/{a.size} differ; first at {i}: gpu={a.ravel()[i]!r} oracle={b.ravel()[i]!r}")
    else:
        assert np.array_equal(a, b), what


def delay_spec(roles):
    return ",".join(f"{r}={DELAY_US}" for r in roles)


def check_evaluation(model, ex, what):
    """mrr_score, predict and recommend, called right behind the last step: no synchronize in between."""
    tptr, tit = S.eval_data()
    mrr, ranks = model.mrr_score(tptr, tit)
    hist = tit[int(tptr[0]): int(tptr[1])]
    pred = model.predict(model.user_representation(hist), np.arange(S.ITEMS, dtype=np.uint32))
    ri, rs = model.recommend(tptr, tit, S.TOP_K)
    assert_same_bits(ranks, ex.ranks, f"{what}: mrr ranks")
    assert mrr == ex.mrr, what
    assert_same_bits(pred, ex.predict, f"{what}: predict")
    assert_same_bits(ri, ex.rec_items, f"{what}: recommend items")
    assert_same_bits(rs, ex.rec_scores, f"{what}: recommend scores")


def check_model(model, case, ex, loss, lagged, what):
    for p in S.params_of(case):
        assert_same_bits(model.get_param(p), ex.params[p], f"{what}: {p.name}")
    assert loss == pytest.approx(ex.loss, rel=1e-6), what
    assert_same_bits(np.array([lagged], np.float32), np.array([ex.lagged], np.float32), f"{what}: lagged loss figure")


def check_counters(counts, delayed, what, data=S.UNIFORM):
    """The hook acted: at least one delay per step on every delayed role (the copier works once per epoch; a step that stays on
    the main stream queues nothing on side and sorter), none elsewhere."""
    for role in STREAM_ROLES:
        if role in delayed:
            least = S.EPOCHS if role == "copier" else data.overlapped_steps if role in ("side", "sorter") else data.steps
            assert counts[role] >= least, f"{what}: {role} was delayed {counts[role]} times, expected at least {least}"
        else:
            assert counts[role] == 0, f"{what}: {role} was delayed though not named"


def run_single(name, drive, setup=None, before_read=None, timing=None, data=S.UNIFORM):
    """One model through the three epochs of `data`, `drive` = "step" (sbr_fit_step), "halves" (step_local | debug fetch of the
    dense gradient and the hidden states | step_apply), "fit" or "step+steps" (sbr_fit_step for the steps that engage the side
    streams, sbr_fit_steps for the others); then the evaluation calls and every parameter against the oracle.
    timing: the families expected to report launches (the steps' timing is read before the evaluation calls)."""
    case, ex = S.CASE_BY_NAME[name], S.oracle_single(name, data)
    ptr, it = S.train_data(1, data)
    what = f"{name} on {data.name} via {drive} [{os.environ.get(VAR, 'no delay')}]"
    m = Model(case.hp())
    if setup:
        setup(m)
    try:
        if drive == "fit":
            loss = m.fit(ptr, it)
            lagged = m.last_fit_lagged_loss()
            check_evaluation(m, ex, what)
        else:
            plan = m.fit_begin(ptr, it)
            k = 0
            for e in range(S.EPOCHS):
                nmb = plan.epoch_prepare()
                assert nmb == len(data.rows)
                if e + 1 < S.EPOCHS:
                    plan.epoch_prefetch()
                for mb in range(nmb):
                    if drive == "step" or (drive == "step+steps" and ex.rows[k] > S.OVERLAP_ABOVE_ROWS):
                        plan.step(mb)
                    elif drive == "step+steps":
                        plan.steps(mb, 1)
                    else:
                        plan.step_local(mb)
                        assert_same_bits(plan.debug_fetch(Debug.DENSE_GRAD, ex.rows[k]), ex.dense[k], f"{what}: step {k} dense gradient")
                        assert_same_bits(plan.debug_fetch(Debug.HIDDEN, ex.rows[k]), ex.hidden[k], f"{what}: step {k} hidden states")
                        plan.step_apply(mb)
                    k += 1
            if timing is not None:
                got = {f for f, (ms, n) in m.timing_read().items() if n > 0}
                assert got == set(timing), f"{what}: families with launches {sorted(got)}, expected {sorted(timing)}"
            if before_read:
                before_read()
            check_evaluation(m, ex, what)
            lagged = plan.end_lagged()
            loss = plan.end()[0]
            plan.close()
        check_model(m, case, ex, loss, lagged, what)
        return m.test_delays_queued()
    finally:
        m.close()


# ---------------------------------------------------------------- the method ---------------------------------------------------
def test_a_missing_join_is_visible():
    """A float that is 1.0; a stream late by DELAY_US sets it to 2.0 and records an event; a second stream copies it.  With the
    wait for the event the copy is 2.0; without it the copy runs while the first stream is still held back: 1.0.  (Only a plain
    float is read early.)"""
    assert selftest_stream_delay(DELAY_US, True) == 2.0
    assert selftest_stream_delay(DELAY_US, False) == 1.0


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_shape_engages_the_whole_schedule(name):
    S.check_shape(name)


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_undelayed_step_times(name):
    """Prints the case's step time with overlap off, the sum over the kernel families (what DELAY_US is chosen from: at least
    four times the largest; see the module's docstring), and holds the run to the oracle."""
    case = S.CASE_BY_NAME[name]
    ex = S.oracle_single(name)
    ptr, it = S.train_data()
    m = Model(case.hp())
    try:
        m.set_overlap(False)
        m.timing_enable(True)
        plan = m.fit_begin(ptr, it)
        for e in range(S.EPOCHS):
            for mb in range(plan.epoch_prepare()):
                plan.step(mb)
        t = m.timing_read()
        total = sum(ms for ms, n in t.values())
        print(f"\n{name}: {total / STEPS:.3f} ms per step with overlap off ("
              + ", ".join(f"{f} {ms / STEPS:.3f}" for f, (ms, n) in t.items() if n) + f"); DELAY_US = {DELAY_US}")
        lagged, loss = plan.end_lagged(), plan.end()[0]
        plan.close()
        check_model(m, case, ex, loss, lagged, f"{name} overlap off, timed")
    finally:
        m.close()


# ---------------------------------------------------------------- one device ---------------------------------------------------
ROLE_SETS = [("main",), ("side",), ("sorter",), ("copier",), ("side", "sorter", "copier")]


@pytest.mark.parametrize("drive", ["step", "halves", "fit"])
@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_default_run_equals_the_oracle(name, drive):
    counts = run_single(name, drive)
    check_counters(counts, (), f"{name} {drive}")


@pytest.mark.parametrize("roles", ROLE_SETS, ids=["+".join(r) for r in ROLE_SETS])
@pytest.mark.parametrize("drive", ["step", "halves", "fit"])
@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_late_stream_changes_no_bit(monkeypatch, name, drive, roles):
    monkeypatch.setenv(VAR, delay_spec(roles))
    counts = run_single(name, drive)
    check_counters(counts, roles, f"{name} {drive} {roles}")


# ------------------------------------------------- one device, steps of two forms ----------------------------------------------
# What a step leaves for the next one — which events the main stream has not joined — crosses a change of the step's form here:
# every epoch of the MIXED data is two steps on all the streams and one that stays on the main stream (S.check_mixed_shape).
MIXED_ROLE_SETS = [(), ("main",), ("sorter",), ("side", "sorter", "copier")]


@pytest.mark.parametrize("name", S.MIXED_CASES)
def test_mixed_epoch_changes_the_form_of_the_step(name):
    S.check_mixed_shape(name)


@pytest.mark.parametrize("roles", MIXED_ROLE_SETS, ids=["+".join(r) or "undelayed" for r in MIXED_ROLE_SETS])
@pytest.mark.parametrize("drive", ["step", "halves", "fit"])
@pytest.mark.parametrize("name", S.MIXED_CASES)
def test_mixed_epoch_late_stream_changes_no_bit(monkeypatch, name, drive, roles):
    if roles:
        monkeypatch.setenv(VAR, delay_spec(roles))
    counts = run_single(name, drive, data=S.MIXED)
    check_counters(counts, roles, f"{name} mixed {drive} {roles}", S.MIXED)


@pytest.mark.parametrize("role", ["sorter", "main"])
@pytest.mark.parametrize("name", S.MIXED_CASES)
def test_steps_behind_a_large_step_late_stream_changes_no_bit(monkeypatch, name, role):
    """sbr_fit_steps on a plan whose last step ran on all the streams: it joins whatever that step left.  (The one-launch runs of
    sbr_fit_steps need a plan of one sequence per step, whose steps never engage the side streams: the short step goes through
    sbr_fit_steps' step-by-step form.)"""
    monkeypatch.setenv(VAR, delay_spec((role,)))
    counts = run_single(name, "step+steps", data=S.MIXED)
    check_counters(counts, (role,), f"{name} mixed step+steps {role}", S.MIXED)


# ---------------------------------------------------------------- world 2 ------------------------------------------------------
# form: (case, partitioned table, gradient exchange, parallelism)
FORMS = {
    "owner-applied": ("normal-warp-32", False, False, PAR_SYNC),
    "gradient": ("ewma-warp-16", False, True, PAR_SYNC),
    "partitioned": ("coupled-hinge-16", True, False, PAR_SYNC),
    "pipeline": ("normal-warp-32", False, True, PAR_ASYNC),   # staleness one: the only user of xs
}
WORLD = 2
GROUP_ROLES = ["main@0", "main@1", "xs@0", "xs@1", "sorter@1"]
# only the staleness-one pipeline has an exchange stream
GROUP_DELAYS = [(form, role) for form in FORMS for role in GROUP_ROLES if form == "pipeline" or not role.startswith("xs")]


def run_group(form, threads, data=S.UNIFORM):
    name, partition, gradient, par = FORMS[form]
    case, ex = S.CASE_BY_NAME[name], S.oracle_world(name, WORLD, par, data)
    ptr, it = S.train_data(WORLD, data)
    what = f"{form} ({name}) on {data.name}, host threads {threads} [{os.environ.get(VAR, 'no delay')}]"
    models = group_create(case.hp(world=WORLD, par=par), WORLD, partition_item_table=partition)
    gp = GroupPlan(models, ptr, it, host_threads=threads)
    try:
        if not partition and par == PAR_SYNC:
            gp.set_exchange(gradient)
        for e in range(S.EPOCHS):
            nmb = gp.epoch_prepare(prefetch_next=e + 1 < S.EPOCHS)
            assert nmb == len(data.rows)
            for mb in range(nmb):
                assert gp.member(0).minibatch_rows(mb) == data.rows[mb]
                gp.step(mb)
        for q in range(WORLD):
            check_evaluation(models[q], ex, f"{what} replica {q}")
        assert gp.stats()[2] == (WORLD if threads else 1)
        loss = gp.end()
        for q in range(WORLD):
            check_model(models[q], case, ex, loss, models[q].last_fit_lagged_loss(), f"{what} replica {q}")
        return [m.test_delays_queued() for m in models]
    finally:
        gp.close()
        for m in models:
            m.close()


@pytest.mark.parametrize("threads", [False, True], ids=["one-host-thread", "host-threads"])
@pytest.mark.parametrize("form", list(FORMS))
def test_group_default_run_equals_the_oracle(form, threads):
    for q, counts in enumerate(run_group(form, threads)):
        check_counters(counts, (), f"{form} replica {q}")


@pytest.mark.parametrize("threads", [False, True], ids=["one-host-thread", "host-threads"])
@pytest.mark.parametrize("form,role", GROUP_DELAYS)
def test_group_late_stream_changes_no_bit(monkeypatch, form, role, threads):
    r, dev = role.split("@")
    monkeypatch.setenv(VAR, f"{role}={DELAY_US}")
    counts = run_group(form, threads)
    for q in range(WORLD):
        check_counters(counts[q], (r,) if q == int(dev) else (), f"{form} {role} replica {q}")


@pytest.mark.parametrize("role", ["main@0", "sorter@1"])
@pytest.mark.parametrize("form", ["gradient", "partitioned"])
def test_group_mixed_epoch_late_stream_changes_no_bit(monkeypatch, form, role):
    r, dev = role.split("@")
    monkeypatch.setenv(VAR, f"{role}={DELAY_US}")
    counts = run_group(form, False, S.MIXED)
    for q in range(WORLD):
        check_counters(counts[q], (r,) if q == int(dev) else (), f"{form} mixed {role} replica {q}", S.MIXED)


# ---------------------------------------------------------------- switches -----------------------------------------------------
def families_of(case):
    used = {"SCORE", "DENSE_GRAD", "DENSE_UPDATE", "SPARSE_UPDATE", "SPARSE_SORT"}
    return used if case.ewma_fused else used | {"RECURRENT_FWD", "RECURRENT_BWD"}


@pytest.mark.parametrize("drive", ["step", "fit"])
@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_overlap_off_changes_no_bit(name, drive):
    run_single(name, drive, setup=lambda m: m.set_overlap(False))


@pytest.mark.parametrize("select", ["all", "score", "none"])
@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_timing_changes_no_bit(name, select):
    """Timing on, with every family, with SCORE alone (the mode bench.py's headline runs in) and with none selected: the same
    bits, and launches reported for exactly the selected families the shape uses."""
    case = S.CASE_BY_NAME[name]
    chosen = {"all": None, "score": ["SCORE"], "none": []}[select]
    expect = families_of(case) if chosen is None else set(chosen)

    def setup(m):
        m.timing_enable(True)
        m.timing_select(chosen)

    run_single(name, "step", setup=setup, timing=expect)


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_caller_stream_changes_no_bit(name):
    """sbr_model_set_stream to a torch side stream; the caller synchronises that stream before it reads."""
    import torch

    stream = torch.cuda.Stream()
    run_single(name, "step", setup=lambda m: m.set_stream(stream.cuda_stream), before_read=stream.synchronize)
    stream.synchronize()


def test_timing_takes_one_sequence_steps_off_the_one_launch_path():
    """One sequence per step, step fusion 2: sbr_fit_steps runs whole runs of steps in one launch — unless timing is on, when every
    step is launched by itself.  Same bits either way; the timed run reports its launches, the one-launch run none."""
    case = S.ONE_SEQ_CASE
    ptr, it = S.one_sequence_data()
    params, loss_o, lagged_o = S.oracle_one_sequence()
    for timed in (False, True):
        m = Model(case.hp(epochs=S.ONE_SEQ_EPOCHS, batch=1, items=S.ONE_SEQ_ITEMS))
        try:
            m.set_step_fusion(2)
            m.timing_enable(timed)
            plan = m.fit_begin(ptr, it)
            for e in range(S.ONE_SEQ_EPOCHS):
                plan.steps(0, plan.epoch_prepare())
            launches = {f: n for f, (ms, n) in m.timing_read().items() if n}
            one_launch_steps = plan.phase_clocks()[5]
            lagged, loss = plan.end_lagged(), plan.end()[0]
            plan.close()
            what = f"one sequence per step, timing {timed}"
            for p in S.params_of(case):
                assert_same_bits(m.get_param(p), params[p], f"{what}: {p.name}")
            assert loss == pytest.approx(loss_o, rel=1e-6)
            assert_same_bits(np.array([lagged], np.float32), np.array([lagged_o], np.float32), f"{what}: lagged loss figure")
            if timed:
                assert launches.get("SCORE", 0) > 0 and one_launch_steps == 0, (launches, one_launch_steps)
            else:
                assert not launches and one_launch_steps > 0, (launches, one_launch_steps)
        finally:
            m.close()
