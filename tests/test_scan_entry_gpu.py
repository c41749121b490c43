"""GPU: the 34 entry points of the top-k scan families behave as one path — the same refusals, in the same order, with nothing
written; the same success tails; and the same bytes whichever way the same three rows are given: as histories, as representations
with the histories as exclusion lists, as a session store's slots, or as any of those through an item set of the whole catalogue.

One tiny LSTM model (64 items, embedding width 1, max_sequence_length 8), three rows with histories of 0, 1 and 5 items, a store
without memory and one with, a set of 5 ids and an empty set, item tags and groups set.  ENTRY / Args: test_scan_entry_cpu.py."""
import numpy as np
import pytest

from helpers import LOSS_HINGE, hparams
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ModelKind, Param, Status
from sbr_rs_amd.engine import Above, Model, Partition, softmax_frac_bits
from test_item_set_gpu import _same_rows
from test_scan_entry_cpu import ALWAYS_FILTERED, ENTRY, HAS_K, INCLUDE_HISTORY, MAX_K, SENTINEL, Args, call

pytestmark = pytest.mark.gpu

ITEMS, DIM, T, CAPACITY = 64, 1, 8, 4
PTR = np.array([0, 0, 1, 6], np.uint64)
IDS = np.array([3, 9, 2, 7, 9, 11], np.uint32)
LISTS = [IDS[int(PTR[u]): int(PTR[u + 1])] for u in range(3)]
SLOTS = np.arange(3, dtype=np.uint32)
OK, REFUSED = Status.OK, Status.INVALID_ARGUMENT


def _new_model():
    m = Model(hparams(ITEMS, T, DIM, int(ModelKind.LSTM_NORMAL), LOSS_HINGE))
    rs = np.random.RandomState(3)
    m.set_param(Param.ITEM_BIAS, (rs.randn(ITEMS) * 0.5).astype(np.float32))
    m.set_item_tags(rs.randint(1, 8, ITEMS).astype(np.uint32))
    m.set_item_groups(rs.randint(0, 6, ITEMS).astype(np.uint32))
    return m


def _store(m, remember):
    st = m.sessions(CAPACITY, remember=remember)
    st.append(SLOTS, (PTR, IDS))
    return st


class Env:
    def __init__(self):
        self.L = _lib.load()
        self.m, self.other = _new_model(), _new_model()
        self.st0, self.st4, self.st_other = _store(self.m, 0), _store(self.m, 4), _store(self.other, 0)
        self.s5, self.s0, self.s_all = self.m.item_set([60, 2, 9, 33, 7]), self.m.item_set([]), self.m.item_set(np.arange(ITEMS))
        self.reps = self.m.user_representations(PTR, IDS)

    def close(self):
        for o in (self.s5, self.s0, self.s_all, self.st0, self.st4, self.st_other, self.m, self.other):
            o.close()

    def run(self, name, src, c, store="st0", item_set="s5"):
        """the entry point on the handle its source names; `src` is the source of rows, which a set's descriptor states"""
        c.source = src
        if src == "store" and c.store is None:
            c.store = getattr(self, store)._h.value
        if c.reps is not None and c.reps.shape == (3, 16):
            c.reps = self.reps
        kind = ENTRY[name][0]
        h = getattr(self, item_set)._h if kind == "set" else getattr(self, store)._h if kind == "store" else self.m._h
        return call(self.L, name, h, c)


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def _targets():
    """(entry point, source of rows): 18 + 9 and the set's 7 over its three descriptors"""
    for name, (source, _, _) in ENTRY.items():
        for src in (("hist", "reps", "store") if source == "set" else (source,)):
            yield name, src


def _has_flags(name, src):
    source, family, _ = ENTRY[name]
    return src == "hist" or (src == "store" and not (source == "store" and family.startswith("diverse")))


def _takes_masks(name):
    source, family, _ = ENTRY[name]
    return source == "set" or family not in ("plain", "diverse")


def _refused(env, name, src, what, store="st0", item_set="s5", **over):
    c = Args(**over)
    st = env.run(name, src, c, store, item_set)
    assert st == REFUSED, (name, src, what, Status(st))
    assert c.untouched(), (name, src, what, c.touched())


def _accepted(env, name, src, what, store="st0", item_set="s5", **over):
    c = Args(**over)
    st = env.run(name, src, c, store, item_set)
    assert st == OK, (name, src, what, Status(st))
    return c


def test_every_entry_point_accepts_the_well_formed_call_and_writes_its_tails(env):
    fb = softmax_frac_bits(ITEMS)
    for name, src in _targets():
        family = ENTRY[name][1]
        for item_set in ("s5", "s0") if ENTRY[name][0] == "set" else ("s5",):
            c = _accepted(env, name, src, "well-formed", item_set=item_set)
            if family == "partition":  # the model's F, with or without a set
                assert c.fb.value == fb and c.total.value == SENTINEL, (name, src, item_set)
            elif family in ("above", "top"):
                assert c.total.value == int(c.counts.sum()) and c.fb.value == SENTINEL, (name, src, item_set)
                assert c.total.value > 0 or item_set == "s0", (name, src)
            else:
                assert c.fb.value == SENTINEL and c.total.value == SENTINEL and not np.all(c.oi == SENTINEL), (name, src, item_set)


def test_refusals_leave_every_output_alone(env):
    other_ptr = np.array([0, 1, 1, 2], np.uint64)
    for name, src in _targets():
        source, family, _ = ENTRY[name]
        if _has_flags(name, src):
            for bit in range(1, 32):
                _refused(env, name, src, f"flag bit {bit}", flags=1 << bit)
                _refused(env, name, src, f"flag bit {bit} with include_history", flags=(1 << bit) | INCLUDE_HISTORY, store="st4")
        if src == "store" and _has_flags(name, src):
            _refused(env, name, src, "include_history on a store without memory", flags=INCLUDE_HISTORY)
            _accepted(env, name, src, "include_history on a store with memory", flags=INCLUDE_HISTORY, store="st4")
        if src in ("reps", "store"):
            _refused(env, name, src, "lists without items", excl_ptr=other_ptr)
            _refused(env, name, src, "items without lists", excl_items=IDS)
            _accepted(env, name, src, "empty lists without items", excl_ptr=np.full(4, 5, np.uint64))
            _refused(env, name, src, "an excluded id = num_items", excl_ptr=np.array([0, 1, 1, 1], np.uint64), excl_items=np.array([ITEMS], np.uint32))
            _refused(env, name, src, "decreasing lists", excl_ptr=np.array([0, 2, 1, 2], np.uint64), excl_items=IDS)
        if src == "hist":
            _refused(env, name, src, "a decreasing user_ptr", user_ptr=np.array([0, 2, 1, 6], np.uint64))
            _refused(env, name, src, "an item id = num_items", item_ids=np.array([3, 9, 2, ITEMS, 9, 11], np.uint32))
        if src == "store":
            _refused(env, name, src, "a slot = capacity", slots=np.array([0, 1, CAPACITY], np.uint32))
            _refused(env, name, src, "a duplicate slot", slots=np.array([0, 1, 1], np.uint32))
        if family in HAS_K:
            _refused(env, name, src, "k = 0", k=0)
            _refused(env, name, src, "k above the maximum", k=MAX_K + 1)
        if family.startswith("diverse"):
            _refused(env, name, src, "pool < k", k=4, pool=3)
            _refused(env, name, src, "a NaN trade_off", trade_off=float("nan"))
        if family == "capped":
            _refused(env, name, src, "pool < k", k=4, cap_pool=3)
            _refused(env, name, src, "cap = 0", cap=0)
        if family in ("sampled", "partition"):
            _refused(env, name, src, "temperature 0", temperature=0.0)
        if source == "set":
            if src == "store":
                _refused(env, name, src, "a store of another model", store="st_other")
                _refused(env, name, src, "a store descriptor with item_ids", desc=_desc(env, src, item_ids=IDS.ctypes.data))
            if src == "hist":
                _refused(env, name, src, "a histories descriptor with lists", excl_ptr=other_ptr, excl_items=IDS)
                _refused(env, name, src, "a histories descriptor with a list pointer alone", excl_ptr=np.full(4, 5, np.uint64))
            if src == "reps":
                _refused(env, name, src, "a representations descriptor with flags", desc=_desc(env, src, flags=INCLUDE_HISTORY))
                _refused(env, name, src, "a representations descriptor with slots", desc=_desc(env, src, slots=SLOTS.ctypes.data))
                _refused(env, name, src, "a representations descriptor with item_ids", desc=_desc(env, src, item_ids=IDS.ctypes.data))
            _refused(env, name, src, "two sources", desc=_desc(env, src, **({"reps": env.reps.ctypes.data} if src != "reps" else {"user_ptr": PTR.ctypes.data})))
            _refused(env, name, src, "no descriptor", desc=False)


def _desc(env, src, **fields):
    c = Args(source=src, store=env.st0._h.value)
    c.reps = env.reps
    d = c.descriptor()
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def test_masks_need_tags_and_a_cap_needs_groups(env):
    m = env.m
    tags, groups = m.item_tags(), m.item_groups()
    ones = np.ones(3, np.uint32)
    try:
        m.set_item_tags(None)
        for name, src in _targets():
            family = ENTRY[name][1]
            if family in ALWAYS_FILTERED:
                _refused(env, name, src, "a filtered call without tags")
            if _takes_masks(name):
                _refused(env, name, src, "masks without tags", any_of=ones)
                _refused(env, name, src, "masks without tags", none_of=ones)
            elif family not in ALWAYS_FILTERED:
                _accepted(env, name, src, "no masks, no tags")
    finally:
        m.set_item_tags(tags)
    try:
        m.set_item_groups(None)
        for name, src in _targets():
            if ENTRY[name][1] == "capped":
                _refused(env, name, src, "a capped call without groups")
    finally:
        m.set_item_groups(groups)
    for name, src in _targets():
        _accepted(env, name, src, "tags and groups set again", **({"any_of": ones} if _takes_masks(name) else {}))


def test_the_empty_reps_calls_are_legal_and_write_no_row(env):
    for name, src in _targets():
        if src != "reps" or ENTRY[name][0] == "set":
            continue
        family = ENTRY[name][1]
        c = _accepted(env, name, src, "no rows", n=0, reps=None, oi=None, osc=None)
        assert c.fb.value == (softmax_frac_bits(ITEMS) if family == "partition" else SENTINEL), name
        assert c.total.value == (0 if family in ("above", "top") else SENTINEL), name
        c.fb.value = c.total.value = SENTINEL
        c.oi, c.osc = c.ids, c.idscores  # untouched() reads every array
        assert c.untouched(), (name, c.touched())


def test_a_stale_set_or_store_refuses_every_scan_until_it_is_bound_again(env):
    m = env.m
    st0, st4, s5 = _store(m, 0), _store(m, 4), m.item_set([60, 2, 9, 33, 7])
    env.t0, env.t4, env.t5 = st0, st4, s5
    try:
        m.set_param(Param.ITEM_BIAS, m.get_param(Param.ITEM_BIAS))
        for name, src in _targets():
            kind = ENTRY[name][0]
            if kind == "set":
                _refused(env, name, src, "a stale set", store="st0", item_set="t5")  # the set's entry comes before the store's
            elif kind == "store":
                _refused(env, name, src, "a stale store", store="t0")
                _refused(env, name, src, "a stale store with memory", store="t4")
        s5.refresh()
        for name, src in _targets():
            if ENTRY[name][0] != "set":
                continue
            if src == "store":
                _refused(env, name, src, "a current set over a stale store", store="t0", item_set="t5")
            else:
                _accepted(env, name, src, "a refreshed set", item_set="t5")
        st4.replay()
        st0.reset()
        st0.append(SLOTS, (PTR, IDS))
        for name, src in _targets():
            if src == "store":
                _accepted(env, name, src, "a store emptied and filled again", store="t0", item_set="t5")
                _accepted(env, name, src, "a replayed store", store="t4", item_set="t5")
    finally:
        for o in (s5, st0, st4):
            o.close()
        # the module's own stores and sets went stale with the same set_param: bind them again
        for s in (env.s5, env.s0, env.s_all):
            s.refresh()
        env.st4.replay()
        env.st0.reset()
        env.st0.append(SLOTS, (PTR, IDS))


def _arrays(x):
    if isinstance(x, np.ndarray):
        return (x,)
    if isinstance(x, Partition):
        return (x.shift, x.mass, np.array([x.frac_bits]))
    if isinstance(x, Above):
        return (x.ptr, x.ids, x.scores) + (() if x.cuts is None else (x.cuts,))
    return tuple(a for part in x for a in _arrays(part))


def test_the_same_rows_give_the_same_bytes_from_every_source_and_through_the_whole_set(env):
    m, st, s = env.m, env.st0, env.s_all
    assert np.array_equal(st.lengths(SLOTS), np.diff(PTR))
    reps = m.user_representations(PTR, IDS)
    th = float(m.recommend(PTR, IDS, 8)[1][:, -1].min())  # every row has at least 8 items at or over it
    ways = {"histories": (m, "", (PTR, IDS), {}), "representations": (m, "_reps", (reps,), {"exclude": LISTS}),
            "store": (st, "", (SLOTS,), {"exclude": LISTS}), "set, histories": (s, "", (PTR, IDS), {}),
            "set, representations": (s, "_reps", (reps,), {"exclude": LISTS}), "set, store": (s.on(st), "", (SLOTS,), {"exclude": LISTS})}
    families = {"recommend": ((4,), {}), "recommend_sampled": ((4,), {"temperature": 0.7, "seed": 3}),
                "log_partition": ((), {"temperature": 0.7}), "recommend_above": ((th,), {}), "count_above": ((th,), {}),
                "recommend_top": ((5,), {}), "nth_score": ((5,), {}), "recommend_capped": ((4,), {"cap": 1}),
                "recommend_diverse": ((3, 8), {})}
    masks = {"any_of": np.array([1, 3, 6], np.uint32), "none_of": np.array([4, 0, 1], np.uint32)}
    for fam, (args, kw) in families.items():
        for filt in ({}, masks):
            want = None
            for way, (obj, suffix, lead, extra) in ways.items():
                got = _arrays(getattr(obj, fam + suffix)(*lead, *args, **kw, **extra, **filt))
                if want is None:
                    want = got
                    assert any(a.size for a in got), fam
                else:
                    _same_rows(got, want, f"{fam}{' filtered' if filt else ''}: {way} against histories")
