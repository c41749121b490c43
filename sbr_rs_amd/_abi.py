"""ctypes view of include/sbr_hip.h (struct layout, enums, constants).  No library is loaded here."""
from __future__ import annotations

import ctypes as C
import enum


class Status(enum.IntEnum):
    OK = 0
    NO_INTERACTIONS = 1
    INVALID_PREDICTION = 2
    INVALID_ARGUMENT = 3
    UNSUPPORTED = 4
    NO_DEVICE = 5
    HIP = 6
    OUT_OF_MEMORY = 7


class ModelKind(enum.IntEnum):
    LSTM_NORMAL = 0
    LSTM_COUPLED = 1
    EWMA = 2


class Param(enum.IntEnum):
    ITEM_EMBEDDING = 0
    ITEM_EMBEDDING_ACC = 1
    ITEM_BIAS = 2
    ITEM_BIAS_ACC = 3
    LSTM_W = 4
    LSTM_W_ACC = 5
    LSTM_B = 6
    LSTM_B_ACC = 7
    EWMA_ALPHA = 8
    EWMA_ALPHA_ACC = 9
    ITEM_EMBEDDING_M = 10
    ITEM_BIAS_M = 11
    LSTM_W_M = 12
    LSTM_B_M = 13
    EWMA_ALPHA_M = 14


class Debug(enum.IntEnum):
    HIDDEN = 0
    NEGATIVES = 1
    COEF = 2
    LOSS = 3
    DHIDDEN = 4
    DINPUT = 5
    DENSE_GRAD = 6
    IN_IDX = 7
    OUT_IDX = 8
    TRIES = 9
    DZ = 10


class KernelFamily(enum.IntEnum):
    RECURRENT_FWD = 0
    SCORE = 1
    RECURRENT_BWD = 2
    DENSE_GRAD = 3
    DENSE_UPDATE = 4
    SPARSE_UPDATE = 5
    RANK = 6
    SPARSE_SORT = 7


NUM_KERNEL_FAMILIES = 8
ABI_VERSION = 13


class SbrHparams(C.Structure):
    _fields_ = [
        ("num_items", C.c_uint32),
        ("max_sequence_length", C.c_uint32),
        ("embedding_dim", C.c_uint32),
        ("learning_rate", C.c_float),
        ("l2_penalty", C.c_float),
        ("model", C.c_int32),
        ("loss", C.c_int32),
        ("optimizer", C.c_int32),
        ("parallelism", C.c_int32),
        ("seed", C.c_uint8 * 16),
        ("num_epochs", C.c_uint32),
        ("num_devices", C.c_uint32),
        ("device_rank", C.c_uint32),
        ("batch_sequences", C.c_uint32),
    ]


class SbrSampleArgs(C.Structure):
    """struct sbr_sample_args of the *_sampled calls"""
    _fields_ = [
        ("temperature", C.c_float),
        ("seed", C.c_uint64),
        ("streams", C.c_void_p),
    ]


# ROLLOUT — sbr_sessions_rollout (include/sbr_hip.h): a session's next `steps` items, each picked by the k = 1 scan over what the
# row may still see and fed back as the next cell step's input and the next scan's exclusion, on the device; the store is read only.
# flags: ROLLOUT_SAMPLE (the pick is recommend_sampled's draw at seed + step; else the top-1), ROLLOUT_ALLOW_REPEATS (picks are not
# excluded from later steps), ROLLOUT_INCLUDE_SEEN (a store with memory: its seen items stay eligible).  The sample arguments'
# temperature is also the per-step partition's, which a non-null out_shift asks for.
ROLLOUT_MAX_STEPS = 1024
ROLLOUT_SAMPLE = 1
ROLLOUT_ALLOW_REPEATS = 2
ROLLOUT_INCLUDE_SEEN = 4


class SbrRolloutArgs(C.Structure):
    """struct sbr_rollout_args of sbr_sessions_rollout"""
    _fields_ = [
        ("steps", C.c_uint32),
        ("flags", C.c_uint32),
        ("sample", SbrSampleArgs),
    ]


# BEAM SEARCH — sbr_sessions_beam_search (include/sbr_hip.h): the `width` most likely next-`steps` continuations of each session,
# searched on the device; the store is read only.  flags: ROLLOUT_ALLOW_REPEATS, ROLLOUT_INCLUDE_SEEN (ROLLOUT_SAMPLE is refused).
BEAM_MAX_WIDTH = 32


class SbrBeamArgs(C.Structure):
    """struct sbr_beam_args of sbr_sessions_beam_search"""
    _fields_ = [
        ("steps", C.c_uint32),
        ("width", C.c_uint32),
        ("flags", C.c_uint32),
        ("temperature", C.c_float),
    ]


class SbrCapArgs(C.Structure):
    """struct sbr_cap_args of the *_capped calls"""
    _fields_ = [
        ("cap", C.c_uint32),
        ("pool", C.c_uint32),
    ]


# sbr_item_set_rollout / sbr_item_set_beam_search take a store descriptor (store / slots, the optional lists and masks, flags 0) and
# then the argument tail of sbr_sessions_rollout / sbr_sessions_beam_search after their masks: (args, outputs...).
class SbrScanRows(C.Structure):
    """struct sbr_scan_rows of the sbr_item_set_* scans: exactly one of user_ptr / reps / store names the rows"""
    _fields_ = [
        ("user_ptr", C.c_void_p),
        ("item_ids", C.c_void_p),
        ("flags", C.c_uint32),
        ("reps", C.c_void_p),
        ("store", C.c_void_p),
        ("slots", C.c_void_p),
        ("excl_ptr", C.c_void_p),
        ("excl_items", C.c_void_p),
        ("any_of", C.c_void_p),
        ("none_of", C.c_void_p),
    ]


GUARD_NONE, GUARD_DEVICE_BLOCK, GUARD_PINNED_BLOCK, GUARD_ARENA_TAKE, GUARD_BIG_BLOCK = range(5)  # SBR_GUARD_*
GUARD_WHERE = ("none", "device block", "pinned block", "arena take")


class SbrGuardReport(C.Structure):
    """struct sbr_guard_report of sbr_test_guard_report / sbr_selftest_guard (SBR_TEST_GUARD)"""
    _fields_ = [
        ("blocks", C.c_uint64),
        ("takes", C.c_uint64),
        ("bytes", C.c_uint64),
        ("violations", C.c_uint64),
        ("where", C.c_uint64),
        ("ordinal", C.c_uint64),
        ("requested", C.c_uint64),
        ("offset", C.c_int64),
        ("changed", C.c_uint64),
    ]

    @property
    def checked(self) -> int:
        """blocks and takes checked"""
        return int(self.blocks + self.takes)

    def first(self):
        """(where, ordinal, requested, offset, changed) of the first violated band, or None"""
        if not self.violations:
            return None
        return int(self.where), int(self.ordinal), int(self.requested), int(self.offset), int(self.changed)

    def __str__(self):
        s = f"{self.blocks} blocks + {self.takes} takes checked ({self.bytes} guard bytes): {self.violations} violated"
        if self.violations:
            side = f"{self.offset} bytes past its end" if self.offset > 0 else f"{-self.offset} bytes before its start"
            s += (f"; first: {GUARD_WHERE[self.where]} #{self.ordinal} of {self.requested} requested bytes, first changed byte {side}, "
                  f"{self.changed} bytes changed")
        return s


def storage_dim(embedding_dim: int) -> int:
    """Width the engine stores an embedding_dim in (16 / 32 / 64 / 128 / 256; the extra columns are zero and stay
    zero — sbr_engine.hip `storage_dim`).  Parameters, user representations and predictions use embedding_dim;
    the debug views and exchange blocks (`sbr_fit_debug_fetch`, dense gradient) use this width."""
    for p in (16, 32, 64, 128, 256):
        if 1 <= int(embedding_dim) <= p:
            return p
    raise ValueError(f"embedding_dim {embedding_dim}: 1..256 supported")


def make_hparams(num_items, max_sequence_length, embedding_dim, learning_rate, l2_penalty, model, loss,
                 optimizer, parallelism, seed, num_epochs, num_devices=1, device_rank=0,
                 batch_sequences=1) -> SbrHparams:
    hp = SbrHparams()
    hp.num_items = int(num_items)
    hp.max_sequence_length = int(max_sequence_length)
    hp.embedding_dim = int(embedding_dim)
    hp.learning_rate = float(learning_rate)
    hp.l2_penalty = float(l2_penalty)
    hp.model = int(model)
    hp.loss = int(loss)
    hp.optimizer = int(optimizer)
    hp.parallelism = int(parallelism)
    seed = bytes(seed)
    assert len(seed) == 16
    for i in range(16):
        hp.seed[i] = seed[i]
    hp.num_epochs = int(num_epochs)
    hp.num_devices = int(num_devices)
    hp.device_rank = int(device_rank)
    hp.batch_sequences = int(batch_sequences)
    return hp
