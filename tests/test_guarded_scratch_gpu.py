"""GPU: every call family with GUARD BANDS around its scratch memory (SBR_TEST_GUARD, include/sbr_hip.h) — the
write-side twin of tests/test_poisoned_scratch_gpu.py.  The scratch cache and the serving arena pack buffers back to back, rounded
to 256 bytes, a cache hit up to twice the request: a store one row, one tile or one vector past the end of its buffer faults
nowhere and usually changes no result bit at the shapes a test uses.  Here every block and every arena take is followed by 256 KiB
of a fixed byte, starting at the first byte past the REQUESTED size (and one band lies in front); the bands are compared when the
block is given back, at the next carve, and by the report the `guard` fixture reads after each test body.

G = 256 KiB is twice the largest block one workgroup stores in one step — 64 sequences x 4 x 128 gate floats in the
sequence-resident LSTM forward, 32 rows x 4 x 256 floats at d = 256, both 128 KiB — so an overrun by a whole tile lands in the band.

The module fixture `guard_is_live` proves through sbr_selftest_guard that ONE changed byte is seen and placed exactly — device
block, pinned block, arena take, and a block past the cache's 64 MiB; just past the end and just before the start; on the first and
on the re-used allocation — and that with the hook unset a report has checked nothing: a build without the hook fails there, not
vacuously.

Every body keeps its family's own comparison — equality with the oracle or the family's *_expect module; the bodies are those of
tests/test_poisoned_scratch_gpu.py, of the newer modules' poisoned-scratch tests (their poison switched off: "0") and of the
families' boundary-shape tests — and the fixture adds `violations == 0 and checked > 0` on top.  Nothing is compared with an
unguarded run.  What the method does not show: reads past a buffer, a stride that jumps the whole band, a store into another live
buffer's payload, the virtual-memory ranges of partitioned tables, and the caller's output arrays.

The groups of a GPU run: -k selftest, -k sort, -k serving, -k boundary, -k sessions, -k rollout, -k newer, -k training, -k both."""
import numpy as np
import pytest

import test_beam_gpu
import test_catalogue_gpu
import test_item_set_gpu
import test_item_set_rollout_gpu
import test_numerics_gpu
import test_poisoned_scratch_gpu as poisoned
import test_recommend_gpu
import test_rollout_gpu
import test_sequence_partition_gpu
import test_sequence_ranks_gpu
import test_sessions_gpu
import test_sessions_replay_gpu as replay
import test_sessions_seen_gpu
from helpers import LOSS_BPR, LOSS_HINGE, LOSS_WARP, hparams
from recommend_expect import topk_expectation
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import GUARD_ARENA_TAKE, GUARD_BIG_BLOCK, GUARD_DEVICE_BLOCK, GUARD_PINNED_BLOCK
from sbr_rs_amd.engine import Model, guard_report, selftest_guard
from test_poisoned_scratch_gpu import CASES, COUPLED, EWMA, NORMAL, case_ids
from test_sampled_gpu import _model, _oracle_of, _random_params, _rep_scores

pytestmark = pytest.mark.gpu

HOOK, POISON_HOOK, GROUPS_HOOK = "SBR_TEST_GUARD", "SBR_TEST_POISON", "SBR_CATALOGUE_GROUPS"
GUARD_KIB = 256
G = GUARD_KIB << 10
SELFTEST_BYTES = 4096 + 100  # what sbr_selftest_guard asks for: no multiple of 256, so 156 bytes of rounding join the band behind
PAD = 4352 - SELFTEST_BYTES
# where -> (the place its report names, blocks, takes, guard bytes compared)
SELFTEST = {GUARD_DEVICE_BLOCK: (GUARD_DEVICE_BLOCK, 1, 0, 2 * G + PAD), GUARD_PINNED_BLOCK: (GUARD_PINNED_BLOCK, 1, 0, 2 * G + PAD),
            GUARD_BIG_BLOCK: (GUARD_DEVICE_BLOCK, 1, 0, 2 * G + PAD), GUARD_ARENA_TAKE: (GUARD_ARENA_TAKE, 0, 3, 4 * G + 3 * PAD)}


# ------------------------------------------------------------------------------------------------
# the hook
# ------------------------------------------------------------------------------------------------
def _selftest_reports(mp, kib):
    """{(where, side): (first report, report of the re-used allocation)} under SBR_TEST_GUARD=kib (None: unset)"""
    if kib is None:
        mp.delenv(HOOK, raising=False)
    else:
        mp.setenv(HOOK, str(kib))
    g = Model(hparams(50, 8, 16, int(EWMA), LOSS_HINGE))
    out = {(where, side): selftest_guard(g, where, side) for where in SELFTEST for side in (1, -1)}
    g.close()
    return out


def _assert_selftest_exact(reports):
    for (where, side), pair in reports.items():
        place, blocks, takes, nbytes = SELFTEST[where]
        requested = SELFTEST_BYTES + ((64 << 20) if where == GUARD_BIG_BLOCK else 0)
        ordinal = 1 if (where == GUARD_ARENA_TAKE and side > 0) else 0  # the middle take of three; a block is the first since the report
        for which, r in zip(("first", "re-used"), pair):
            what = f"where={where} side={side} {which} allocation: {r}"
            assert (r.blocks, r.takes, r.bytes) == (blocks, takes, nbytes), what
            assert r.violations == 1 and r.first() == (place, ordinal, requested, side, 1), what


@pytest.fixture(scope="module")
def guard_is_live():
    """One byte is seen, and placed exactly, in all four kinds of allocation, on both sides, first and re-used; with the hook unset
    nothing is guarded, nothing checked and the selftest writes nothing: the tests below run between live bands or not at all."""
    with pytest.MonkeyPatch.context() as mp:
        _assert_selftest_exact(_selftest_reports(mp, GUARD_KIB))
        guard_report()  # drained
        for key, pair in _selftest_reports(mp, None).items():
            for r in pair:
                assert (r.blocks, r.takes, r.bytes, r.violations) == (0, 0, 0, 0), f"hook unset, {key}: {r}"
        g = Model(hparams(50, 8, 16, int(EWMA), LOSS_HINGE))
        g.recommend_reps(np.zeros((3, 16), np.float32), 5)
        r = guard_report(g)
        g.close()
        assert (r.checked, r.bytes, r.violations) == (0, 0, 0), f"hook unset: {r}"
        for bad in ("0", "", "abc", "-4", "256k"):  # malformed is off
            mp.setenv(HOOK, bad)
            r = selftest_guard(None, GUARD_DEVICE_BLOCK, 1)[0]
            assert (r.checked, r.bytes) == (0, 0), f"{HOOK}={bad!r}: {r}"
    return True


@pytest.fixture
def guard(request, monkeypatch, guard_is_live):
    monkeypatch.setenv(HOOK, str(GUARD_KIB))
    monkeypatch.setenv(GROUPS_HOOK, "3")
    guard_report()  # drained: what follows is this test's
    yield GUARD_KIB
    r = guard_report()
    print(f"guard report: {request.node.name}: {r}")
    assert r.violations == 0, f"a store outside its buffer: {r}"
    assert r.checked > 0 and r.bytes > 0, f"nothing was checked: {r}"


def test_selftest_one_byte_is_seen_and_placed(guard):
    """The fixture's proof as a test of its own, and at a second band size (4 KiB): the byte's place does not depend on it."""
    with pytest.MonkeyPatch.context() as mp:
        _assert_selftest_exact(_selftest_reports(mp, GUARD_KIB))
        for (where, side), pair in _selftest_reports(mp, 4).items():
            for r in pair:
                assert r.violations == 1 and r.first()[0] == SELFTEST[where][0] and r.first()[3:] == (side, 1), f"{where} {side}: {r}"


def test_selftest_a_violation_is_reported_once_then_drained(guard):
    """The selftest's findings stay out of the process-wide counters (a report right after it is clean), the counters are read and
    reset, and a guarded model's arena shows up as takes."""
    selftest_guard(None, GUARD_DEVICE_BLOCK, 1)
    g = Model(hparams(50, 8, 16, int(EWMA), LOSS_HINGE))
    g.recommend_reps(np.zeros((3, 16), np.float32), 5)
    r = guard_report(g)
    assert r.violations == 0 and r.blocks > 0 and r.takes > 0, str(r)
    r2 = guard_report()
    assert r2.takes == 0 and r2.violations == 0, str(r2)
    g.close()


@pytest.mark.parametrize("kind", [EWMA, NORMAL, COUPLED], ids=case_ids)
@pytest.mark.parametrize("d", [24, 100])
def test_selftest_model_creation_matches_the_oracle(guard, kind, d):
    poisoned.test_selftest_model_creation_matches_the_oracle(None, kind, d)


# ------------------------------------------------------------------------------------------------
# sort: per-(digit, tile) counters, ping-pong keys, the head list
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small,items", [("0", None), ("0", "64")])
@pytest.mark.parametrize("n,row_bits,dist", [(4096, 6, "uniform"), (4097, 6, "uniform"), (4096, 11, "zipf"), (4097, 11, "zipf"), (100_000, 11, "zipf")])
def test_sort_between_guards(guard, monkeypatch, n, row_bits, dist, small, items):
    test_numerics_gpu.test_key_ordering_is_a_stable_sort_by_row(_lib.load(), monkeypatch, n, row_bits, dist, small, items)


# ------------------------------------------------------------------------------------------------
# serving: the bodies of the poisoned module on its core case (1 000 items x 130 rows, d = 16 and 100 -> 128)
# ------------------------------------------------------------------------------------------------
SERVING = ["recommend", "mrr_score_and_rank_targets", "candidates", "filtered", "recommend_sampled", "log_partition", "recommend_capped", "audience"]


@pytest.mark.parametrize("family", SERVING)
@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_family(guard, family, kind, d):
    getattr(poisoned, "test_serving_" + family)(None, kind, d)


@pytest.mark.parametrize("family", ["above", "top"])
@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_family_with_small_fill_ranges(guard, monkeypatch, family, kind, d):
    getattr(poisoned, "test_serving_" + family)(None, monkeypatch, kind, d)


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("kind,d", [(EWMA, 16), (EWMA, 100)], ids=case_ids)
def test_serving_similar_items(guard, kind, d, metric):
    poisoned.test_serving_similar_items(None, kind, d, metric)


@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 100)], ids=case_ids)
def test_serving_recommend_diverse(guard, kind, d):
    poisoned.test_serving_recommend_diverse(None, kind, d)


def test_serving_interleaved_calls_on_one_model(guard, monkeypatch):
    """52 calls of every family on ONE model: the arena is carved under another layout, with its bands elsewhere, by every call."""
    poisoned.test_serving_interleaved_calls_on_one_model(monkeypatch, True, None)


@pytest.mark.parametrize("kind,d", CASES, ids=case_ids)
def test_serving_list_lengths(guard, kind, d):
    """k = 1, 5 and 33 on the core case (10 and 1 024 >= items are test_serving_family[recommend]'s)."""
    c = poisoned._case(kind, d)
    g = c.model()
    for k in (1, 5, 33):
        poisoned._same_rows(g.recommend_reps(c.reps, k, exclude=c.excl), c.topk(c.excl, k), f"k={k}")
    g.close()


# ------------------------------------------------------------------------------------------------
# boundary shapes of the scans: the families' own tests under the guard
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("items", [1, 31, 32, 33])
def test_boundary_items_per_scan(guard, monkeypatch, items):
    """the last 32-item tile, per-range lists shorter than k, ranges cut to the number of tiles"""
    test_catalogue_gpu.test_recommend_tiny_catalogues(monkeypatch, items)


@pytest.mark.parametrize("rows", [1, 127, 128, 129])
def test_boundary_scan_rows(guard, monkeypatch, rows):
    """the 128-row workgroup tile (130 rows: the core case)"""
    test_catalogue_gpu.test_recommend_user_tile_edges(monkeypatch, rows)


def test_boundary_second_launch_writes_behind_the_first(guard, monkeypatch):
    """8 192 + 40 rows over 64 items, k = 5: two launches, the second writing at out + 8 192 k; EWMA, d = 16, every row against
    the oracle's scores."""
    monkeypatch.setenv(GROUPS_HOOK, "1")
    rows, items, d, k = 8192 + 40, 64, 16, 5
    E, bias = _random_params(items, d, 64)
    g = _model(items, 8, d, EWMA, E, bias)
    reps = (np.random.RandomState(65).randn(rows, d) * 0.5).astype(np.float32)
    scores = _rep_scores(_oracle_of(g), items, reps)
    want = [topk_expectation(scores[u], (), k) for u in range(rows)]
    poisoned._same_rows(g.recommend_reps(reps, k), (np.array([w[0] for w in want], np.uint32), np.array([w[1] for w in want], np.float32)))
    g.close()


@pytest.mark.parametrize("kind", [EWMA, COUPLED], ids=case_ids)
def test_boundary_stored_width_256(guard, kind):
    """the d = 256 thread maps and vector stores of the forward pass and the scan (16 and 128: the core cases)"""
    test_recommend_gpu.test_recommend_matches_oracle(kind, 256, 3000)


# ------------------------------------------------------------------------------------------------
# sessions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(NORMAL, 32), (EWMA, 20)], ids=case_ids)
def test_sessions_between_guards(guard, kind, d):
    poisoned.test_sessions_on_poisoned_stores(None, kind, d)


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("kind,d", [(NORMAL, 32), (EWMA, 20)], ids=case_ids)
def test_sessions_one_and_thirty_three(guard, kind, d, n):
    test_sessions_gpu.test_one_and_thirty_three_sessions(kind, d, n)


@pytest.mark.parametrize("w", [1, 5])
@pytest.mark.parametrize("kind", [NORMAL, EWMA], ids=case_ids)
def test_sessions_seen_ring_wraps(guard, kind, w):
    test_sessions_seen_gpu.test_ring_keeps_the_last_w_in_order_with_repeats(kind, w)


@pytest.mark.parametrize("cap,w", [(1, 1), (33, 5)])
@pytest.mark.parametrize("kind,d", [(NORMAL, 32), (EWMA, 16)], ids=case_ids)
def test_sessions_replay_in_chunks_of_two(guard, monkeypatch, kind, d, cap, w):
    """Stores of capacity 1 and 33 (one slot; a full 32-row tile and one row), a seen ring of 1 and 5 that has wrapped, replayed in
    chunks of 2 sessions after a parameter change: equal to a fresh store that is told each slot's memory."""
    slots = np.arange(cap, dtype=np.uint32)
    rs = np.random.RandomState(cap + w)
    told = [rs.randint(0, replay.ITEMS, (3 * i) % 8 if cap > 1 else 7).astype(np.uint32) for i in range(cap)]
    m = replay.new_model(kind, d)
    st = m.sessions(cap, remember=w)
    st.append(slots, told)
    before = st.seen(slots)
    replay.randomize(m, kind, d, seed=79)
    monkeypatch.setenv(replay.HOOK, "2")
    assert st.replay() == sum(1 for t in told if len(t))
    fresh = replay.fresh_after(m, before, cap=cap, w=w)
    replay.assert_same_store(st, fresh, slots, kind != EWMA, "chunks of 2 vs fresh")
    replay.assert_lists_equal(st.seen(slots), before)
    m.close()


# ------------------------------------------------------------------------------------------------
# rollout and beam search: parity rows, rec_* records, backtrack
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 17])
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 100)], ids=case_ids)
def test_rollout_steps_in_chunks_of_two(guard, monkeypatch, kind, d, steps):
    monkeypatch.setenv("SBR_ROLLOUT_CHUNK", "2")
    test_rollout_gpu.test_greedy_is_the_contract_over_the_oracle(kind, d, steps)


@pytest.mark.parametrize("w", [1, 3, 8])
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 100)], ids=case_ids)
def test_rollout_beam_widths_in_chunks_of_two(guard, monkeypatch, kind, d, w):
    monkeypatch.setenv("SBR_BEAM_CHUNK", "2")
    test_beam_gpu.test_beams_are_the_contract_over_the_oracle(kind, d, w)


@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 16)], ids=case_ids)
def test_rollout_and_beam_inside_an_item_set_of_33(guard, monkeypatch, kind, d):
    monkeypatch.setenv("SBR_ROLLOUT_CHUNK", "2")
    monkeypatch.setenv("SBR_BEAM_CHUNK", "2")
    test_item_set_rollout_gpu.test_rollout_is_the_complement_route(kind, d, "33", 3, monkeypatch)
    test_item_set_rollout_gpu.test_beam_search_is_the_complement_route(kind, d, "33", 3, monkeypatch)


# ------------------------------------------------------------------------------------------------
# the newer families: the one test each of them runs on poisoned scratch, its poison switched off
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [test_sequence_ranks_gpu.SHAPES[1], test_sequence_ranks_gpu.SHAPES[3]], ids=["LSTM", "EWMA"])
def test_newer_sequence_ranks(guard, monkeypatch, shape):
    test_sequence_ranks_gpu.test_sequence_ranks_on_poisoned_scratch(monkeypatch, "0", shape)


@pytest.mark.parametrize("shape", [test_sequence_partition_gpu.SHAPES[1], test_sequence_partition_gpu.SHAPES[3]], ids=["LSTM", "EWMA"])
def test_newer_sequence_partition(guard, monkeypatch, shape):
    test_sequence_partition_gpu.test_sequence_partition_on_poisoned_scratch(monkeypatch, "0", shape)


def test_newer_item_set(guard, monkeypatch):
    test_item_set_gpu.test_on_poisoned_scratch(monkeypatch, 0)


@pytest.mark.parametrize("remember", [0, 5])
@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 16), (NORMAL, 100)], ids=case_ids)
def test_newer_rollout(guard, monkeypatch, kind, d, remember):
    test_rollout_gpu.test_on_poisoned_scratch(kind, d, remember, 0, monkeypatch)


@pytest.mark.parametrize("kind,d", [(NORMAL, 16), (EWMA, 16), (COUPLED, 100)], ids=case_ids)
def test_newer_beam(guard, monkeypatch, kind, d):
    test_beam_gpu.test_on_poisoned_scratch(kind, d, 0, monkeypatch)


def test_newer_item_set_rollout(guard, monkeypatch):
    test_item_set_rollout_gpu.test_on_poisoned_scratch(0, monkeypatch)


# ------------------------------------------------------------------------------------------------
# training: whole fits against the oracle
# ------------------------------------------------------------------------------------------------
def test_training_ewma_hinge_d32(guard):
    poisoned._fit(EWMA, LOSS_HINGE, 32)


def test_training_lstm_warp_d64(guard):
    poisoned._fit(NORMAL, LOSS_WARP, 64, calls=2)


@pytest.mark.parametrize("wide", [False, True], ids=["buffer", "wide"])
def test_training_coupled_bpr_d128(guard, monkeypatch, wide):
    poisoned.test_training_coupled_bpr_d128(None, monkeypatch, wide)


@pytest.mark.parametrize("kind,loss", [(NORMAL, LOSS_WARP), (EWMA, LOSS_BPR)], ids=case_ids)
def test_training_padded_width_d24(guard, kind, loss):
    poisoned._fit(kind, loss, 24)


@pytest.mark.parametrize("min_tiles", ["1", "1000000"])
def test_training_d256_both_bptt_forms(guard, monkeypatch, min_tiles):
    poisoned.test_training_d256_both_bptt_forms(None, monkeypatch, min_tiles)


def test_training_adam(guard):
    poisoned.test_training_adam(None)


def test_training_hot_rows_take_the_chunked_reduction(guard):
    """a hot row with more than 256 entries: the chunked row reduce"""
    poisoned.test_training_hot_rows_take_the_chunked_reduction(None)


@pytest.mark.parametrize("exchange", ["owner", "gradient"])
def test_training_two_ranks_on_one_gpu(guard, exchange):
    """203 items on two ranks: chunk buffers of ceil(I / N) rows with I odd"""
    poisoned.test_training_two_ranks_on_one_gpu(None, exchange)


def _histories_of_rows(rows_per_sequence, items, seed):
    """one history per entry: rows + 1 items (a sequence of n items packs n - 1 rows)"""
    rs = np.random.RandomState(seed)
    lens = np.asarray(rows_per_sequence, np.uint64) + 1
    ptr = np.zeros(len(lens) + 1, np.uint64)
    ptr[1:] = np.cumsum(lens)
    return ptr, rs.randint(0, items, int(ptr[-1])).astype(np.uint32)


def _step_rows(kind, loss, d, T, B, data):
    """the rows of every step of the first epoch (a throwaway model: opening a plan draws from the model's generator)"""
    g = Model(hparams(150, T, d, int(kind), loss, B=B, epochs=2))
    plan = g.fit_begin(*data)
    rows = [plan.minibatch_rows(mb) for mb in range(plan.epoch_prepare())]
    plan.close()
    g.close()
    return rows


@pytest.mark.parametrize("rows", [1023, 1024, 1025])
def test_training_rows_around_a_dense_gradient_chunk(guard, rows):
    """One step of 33 sequences packing one row below, exactly, and one row above SBR_DW_CHUNK_ROWS = 1 024: the chunk partials and
    the pad rows of the last chunk.  LSTM, WARP, d = 64."""
    q, r = divmod(rows, 33)
    data = _histories_of_rows([q + 1] * r + [q] * (33 - r), 150, rows)
    assert _step_rows(NORMAL, LOSS_WARP, 64, 40, 33, data) == [rows]
    poisoned._fit(NORMAL, LOSS_WARP, 64, T=40, B=33, data=data)


@pytest.mark.parametrize("fusion", [2, 0])
@pytest.mark.parametrize("kind,loss", [(EWMA, LOSS_HINGE), (COUPLED, LOSS_BPR)], ids=case_ids)
def test_training_one_sequence_steps_of_64_65_255_rows(guard, kind, loss, fusion):
    """B = 1 at d = 16, both fusion settings: steps of 64, 65 and 255 rows (and short ones between them) — the LDS-staged tails."""
    data = _histories_of_rows([64, 5, 65, 2, 255, 9, 64], 97, 7)
    assert sorted(_step_rows(kind, loss, 16, 256, 1, data)) == [2, 5, 9, 64, 64, 65, 255]
    poisoned._fit(kind, loss, 16, items=97, T=256, B=1, fusion=fusion, data=data)


# ------------------------------------------------------------------------------------------------
# both hooks at once: the poison byte in the payload, the guard byte in the bands
# ------------------------------------------------------------------------------------------------
def test_both_hooks_compose(guard, monkeypatch):
    monkeypatch.setenv(POISON_HOOK, str(0xFF))
    for where in (GUARD_DEVICE_BLOCK, GUARD_PINNED_BLOCK, GUARD_ARENA_TAKE):  # the poison fill leaves the bands alone: still exactly one byte
        g = Model(hparams(50, 8, 16, int(EWMA), LOSS_HINGE))
        _assert_selftest_exact({(where, 1): selftest_guard(g, where, 1)})
        g.close()
    for what, buf in poisoned._selftest_copies(0xFF, big=False).items():  # and the guard fill leaves the payload poisoned
        assert np.all(buf == 0xFF), what
    poisoned.test_serving_recommend(None, NORMAL, 16)
    poisoned.test_serving_log_partition(None, NORMAL, 16)
    poisoned._fit(NORMAL, LOSS_WARP, 64)
