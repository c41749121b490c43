"""CPU: the 34 entry points of the top-k scan families (18 on the model, 9 on a session store, 7 on an item set) refuse what needs
no device before they touch one: a null handle, and through a set every malformed descriptor, are argument errors that write to no
output.  ENTRY, the table of the 34 argument lists over one `Args`, is also what test_scan_entry_gpu.py drives."""
import ctypes as C

import numpy as np

from sbr_rs_amd._abi import SbrCapArgs, SbrSampleArgs, SbrScanRows, Status
from test_item_set_cpu import _lib_loaded

SENTINEL = 7
MAX_K = 1024  # SBR_RECOMMEND_MAX_K
INCLUDE_HISTORY = 1  # SBR_RECOMMEND_INCLUDE_HISTORY
OUTPUTS = ("oi", "osc", "okeys", "shift", "mass", "counts", "cuts", "ids", "idscores", "complete")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Args:
    """One call's arguments, well-formed for three rows, and every output array filled with SENTINEL.  A test changes the fields it
    is about.  `source` is what a set's descriptor names ("hist", "reps" or "store"); `desc`, where not None, replaces the
    descriptor made from the fields."""

    def __init__(self, dim=16, **over):
        self.n, self.k, self.pool, self.flags = 3, 4, 8, 0
        self.user_ptr = np.array([0, 0, 1, 6], np.uint64)
        self.item_ids = np.array([3, 9, 2, 7, 9, 11], np.uint32)
        self.reps = np.zeros((3, dim), np.float32)
        self.slots = np.arange(3, dtype=np.uint32)
        self.store = None  # a set's store descriptor: the store's handle value
        self.excl_ptr = self.excl_items = self.any_of = self.none_of = None
        self.temperature, self.seed, self.trade_off, self.metric = 1.0, 5, 0.5, 0
        self.cap, self.cap_pool = 1, 0
        self.th = np.full(3, -100.0, np.float32)  # every eligible item passes
        self.budget = np.full(3, 3, np.uint64)
        self.capacity = 3 * 64
        self.source, self.desc = "hist", None
        rows = 3 * (MAX_K + 1)
        self.oi, self.osc, self.okeys = (np.full(rows, SENTINEL, dt) for dt in (np.uint32, np.float32, np.float32))
        self.shift, self.mass, self.fb = np.full(3, SENTINEL, np.float32), np.full(3, SENTINEL, np.uint64), C.c_uint32(SENTINEL)
        self.counts, self.total, self.cuts = np.full(3, SENTINEL, np.uint64), C.c_uint64(SENTINEL), np.full(3, SENTINEL, np.float32)
        self.ids, self.idscores = np.full(self.capacity, SENTINEL, np.uint32), np.full(self.capacity, SENTINEL, np.float32)
        self.complete = np.full(3, SENTINEL, np.uint8)
        for name, value in over.items():
            assert hasattr(self, name), name
            setattr(self, name, value)

    def untouched(self):
        return all(np.all(getattr(self, o) == SENTINEL) for o in OUTPUTS) and self.fb.value == SENTINEL and self.total.value == SENTINEL

    def touched(self):
        return [o for o in OUTPUTS if not np.all(getattr(self, o) == SENTINEL)] + [o for o in ("fb", "total") if getattr(self, o).value != SENTINEL]

    def descriptor(self):
        if self.desc is not None:
            return self.desc
        d = SbrScanRows()
        if self.source == "hist":
            d.user_ptr, d.item_ids, d.flags = self.user_ptr.ctypes.data, self.item_ids.ctypes.data, self.flags
        elif self.source == "reps":
            d.reps = self.reps.ctypes.data
        else:
            d.store, d.slots, d.flags = self.store, self.slots.ctypes.data, self.flags
        for name in ("excl_ptr", "excl_items", "any_of", "none_of"):
            if getattr(self, name) is not None:
                setattr(d, name, getattr(self, name).ctypes.data)
        return d


# the pieces the 34 argument lists are made of, in the header's order
def _hist(c): return [_p(c.user_ptr), _p(c.item_ids), c.n]  # noqa: E704
def _reps(c): return [_p(c.reps), c.n]  # noqa: E704
def _slots(c): return [_p(c.slots), c.n]  # noqa: E704
def _excl(c): return [_p(c.excl_ptr), _p(c.excl_items)]  # noqa: E704
def _masks(c): return [_p(c.any_of), _p(c.none_of)]  # noqa: E704
def _out(c): return [_p(c.oi), _p(c.osc)]  # noqa: E704
def _part(c): return [_p(c.shift), _p(c.mass), C.byref(c.fb)]  # noqa: E704
def _above(c): return [_p(c.counts), C.byref(c.total), c.capacity, _p(c.ids), _p(c.idscores)]  # noqa: E704
def _div(c): return [c.k, c.pool, c.trade_off, c.metric]  # noqa: E704


def _sample(c):
    c._sa = SbrSampleArgs(c.temperature, c.seed, None)
    return [C.byref(c._sa)]


def _cap(c):
    c._ca = SbrCapArgs(c.cap, c.cap_pool)
    return [C.byref(c._ca)]


def _rows(c):
    c._d = c.descriptor()
    return [None if c._d is False else C.byref(c._d), c.n]


# name -> (source, family, arguments after the handle); family names what the call reads beside its rows
ENTRY = {
    "sbr_recommend": ("hist", "plain", lambda c: _hist(c) + [c.k, c.flags] + _out(c)),
    "sbr_recommend_reps": ("reps", "plain", lambda c: _reps(c) + [c.k] + _excl(c) + _out(c)),
    "sbr_recommend_filtered": ("hist", "filtered", lambda c: _hist(c) + [c.k, c.flags] + _masks(c) + _out(c)),
    "sbr_recommend_filtered_reps": ("reps", "filtered", lambda c: _reps(c) + [c.k] + _excl(c) + _masks(c) + _out(c)),
    "sbr_recommend_sampled": ("hist", "sampled", lambda c: _hist(c) + [c.k, c.flags] + _sample(c) + _masks(c) + _out(c) + [_p(c.okeys)]),
    "sbr_recommend_sampled_reps": ("reps", "sampled", lambda c: _reps(c) + [c.k] + _excl(c) + _sample(c) + _masks(c) + _out(c) + [_p(c.okeys)]),
    "sbr_log_partition": ("hist", "partition", lambda c: _hist(c) + [c.flags, c.temperature] + _masks(c) + _part(c)),
    "sbr_log_partition_reps": ("reps", "partition", lambda c: _reps(c) + _excl(c) + [c.temperature] + _masks(c) + _part(c)),
    "sbr_recommend_above": ("hist", "above", lambda c: _hist(c) + [_p(c.th), c.flags] + _masks(c) + _above(c)),
    "sbr_recommend_above_reps": ("reps", "above", lambda c: _reps(c) + [_p(c.th)] + _excl(c) + _masks(c) + _above(c)),
    "sbr_recommend_top": ("hist", "top", lambda c: _hist(c) + [_p(c.budget), c.flags] + _masks(c) + [_p(c.cuts)] + _above(c)),
    "sbr_recommend_top_reps": ("reps", "top", lambda c: _reps(c) + [_p(c.budget)] + _excl(c) + _masks(c) + [_p(c.cuts)] + _above(c)),
    "sbr_recommend_capped": ("hist", "capped", lambda c: _hist(c) + [c.k, c.flags] + _cap(c) + _masks(c) + _out(c) + [_p(c.complete)]),
    "sbr_recommend_capped_reps": ("reps", "capped", lambda c: _reps(c) + [c.k] + _excl(c) + _cap(c) + _masks(c) + _out(c) + [_p(c.complete)]),
    "sbr_recommend_diverse": ("hist", "diverse", lambda c: _hist(c) + _div(c) + [c.flags] + _out(c)),
    "sbr_recommend_diverse_reps": ("reps", "diverse", lambda c: _reps(c) + _div(c) + _excl(c) + _out(c)),
    "sbr_recommend_diverse_filtered": ("hist", "diverse_filtered", lambda c: _hist(c) + _div(c) + [c.flags] + _masks(c) + _out(c)),
    "sbr_recommend_diverse_filtered_reps": ("reps", "diverse_filtered", lambda c: _reps(c) + _div(c) + _excl(c) + _masks(c) + _out(c)),
    "sbr_sessions_recommend": ("store", "plain", lambda c: _slots(c) + [c.k] + _excl(c) + [c.flags] + _out(c)),
    "sbr_sessions_recommend_filtered": ("store", "filtered", lambda c: _slots(c) + [c.k] + _excl(c) + [c.flags] + _masks(c) + _out(c)),
    "sbr_sessions_recommend_sampled": ("store", "sampled",
                                       lambda c: _slots(c) + [c.k] + _excl(c) + [c.flags] + _sample(c) + _masks(c) + _out(c) + [_p(c.okeys)]),
    "sbr_sessions_log_partition": ("store", "partition", lambda c: _slots(c) + _excl(c) + [c.flags, c.temperature] + _masks(c) + _part(c)),
    "sbr_sessions_recommend_above": ("store", "above", lambda c: _slots(c) + [_p(c.th)] + _excl(c) + [c.flags] + _masks(c) + _above(c)),
    "sbr_sessions_recommend_top": ("store", "top", lambda c: _slots(c) + [_p(c.budget)] + _excl(c) + [c.flags] + _masks(c) + [_p(c.cuts)] + _above(c)),
    "sbr_sessions_recommend_capped": ("store", "capped",
                                      lambda c: _slots(c) + [c.k] + _excl(c) + [c.flags] + _cap(c) + _masks(c) + _out(c) + [_p(c.complete)]),
    "sbr_sessions_recommend_diverse": ("store", "diverse", lambda c: _slots(c) + _div(c) + _excl(c) + _out(c)),
    "sbr_sessions_recommend_diverse_filtered": ("store", "diverse_filtered", lambda c: _slots(c) + _div(c) + _excl(c) + _masks(c) + _out(c)),
    "sbr_item_set_recommend": ("set", "plain", lambda c: _rows(c) + [c.k] + _out(c)),
    "sbr_item_set_recommend_diverse": ("set", "diverse", lambda c: _rows(c) + _div(c) + _out(c)),
    "sbr_item_set_recommend_sampled": ("set", "sampled", lambda c: _rows(c) + [c.k] + _sample(c) + _out(c) + [_p(c.okeys)]),
    "sbr_item_set_log_partition": ("set", "partition", lambda c: _rows(c) + [c.temperature] + _part(c)),
    "sbr_item_set_recommend_above": ("set", "above", lambda c: _rows(c) + [_p(c.th)] + _above(c)),
    "sbr_item_set_recommend_top": ("set", "top", lambda c: _rows(c) + [_p(c.budget), _p(c.cuts)] + _above(c)),
    "sbr_item_set_recommend_capped": ("set", "capped", lambda c: _rows(c) + [c.k] + _cap(c) + _out(c) + [_p(c.complete)]),
}
HAS_K = ("plain", "filtered", "sampled", "capped", "diverse", "diverse_filtered")  # the families with a k argument
ALWAYS_FILTERED = ("filtered", "diverse_filtered")  # the families whose masks make a filter even where both are null


def call(L, name, handle, c):
    return getattr(L, name)(handle, *ENTRY[name][2](c))


def test_the_table_names_the_34_entry_points():
    L = _lib_loaded()
    by_source = {s: [n for n, e in ENTRY.items() if e[0] == s] for s in ("hist", "reps", "store", "set")}
    assert len(ENTRY) == 34 and len(by_source["hist"]) + len(by_source["reps"]) == 18 and len(by_source["store"]) == 9 and len(by_source["set"]) == 7
    for name in ENTRY:
        assert len(getattr(L, name).argtypes) == 1 + len(ENTRY[name][2](Args())), name


def test_a_null_handle_is_an_argument_error_that_writes_nothing():
    L = _lib_loaded()
    for name, (source, _, _) in ENTRY.items():
        for src in (("hist", "reps", "store") if source == "set" else (source,)):
            c = Args(source=src, store=0x1000)  # the store's address is never read: the set is refused first
            assert call(L, name, None, c) == Status.INVALID_ARGUMENT, (name, src)
            assert c.untouched(), (name, src, c.touched())


def test_a_set_refuses_every_malformed_descriptor_without_a_device():
    """test_item_set_cpu.py's descriptors, on a null set: each of the seven set entry points, nothing written"""
    L = _lib_loaded()
    ptr, reps = np.array([0, 0, 0, 0], np.uint64), np.zeros((3, 16), np.float32)
    descriptors = {"histories": SbrScanRows(user_ptr=ptr.ctypes.data), "representations": SbrScanRows(reps=reps.ctypes.data),
                   "no source": SbrScanRows(), "two sources": SbrScanRows(user_ptr=ptr.ctypes.data, reps=reps.ctypes.data),
                   "no descriptor": False}
    for what, d in descriptors.items():
        for name in (n for n, e in ENTRY.items() if e[0] == "set"):
            c = Args(desc=d)
            assert call(L, name, None, c) == Status.INVALID_ARGUMENT, (what, name)
            assert c.untouched(), (what, name, c.touched())
