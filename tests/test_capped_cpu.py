"""CPU: the rule of the *_capped calls stated twice (capped_expect.py) and once in the package (engine.capped_keep), the completion
helper against a fake recommend_top backed by a full ranking, the new surface at every layer, the refusals that never reach the
library, and the no-device behaviour."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from capped_expect import NO_GROUP, capped_rows, rule_ordinal, rule_walk
from recommend_expect import NO_ITEM
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ABI_VERSION, Status

CAPPED = ("sbr_recommend_capped", "sbr_recommend_capped_reps", "sbr_sessions_recommend_capped")
GROUPS = ("sbr_model_set_item_groups", "sbr_model_get_item_groups")
HERE = os.path.dirname(os.path.abspath(__file__))


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def _group_patterns(rs, items):
    own = np.arange(items, dtype=np.uint32)
    none = np.full(items, NO_GROUP, dtype=np.uint32)
    few = rs.randint(0, 7, items).astype(np.uint32)               # heavily tied: seven groups
    edge = rs.choice(np.array([0, 0xFFFFFFFE, NO_GROUP], dtype=np.uint32), items)
    big = np.where(rs.rand(items) < 0.8, 5, own).astype(np.uint32)  # one group holds most items
    mixed = np.where(rs.rand(items) < 0.3, NO_GROUP, rs.randint(0, 40, items)).astype(np.uint32)
    return {"own": own, "none": none, "few": few, "edge": edge, "big": big, "mixed": mixed}


def test_the_two_statements_of_the_rule_and_the_package_agree():
    from sbr_rs_amd.engine import capped_keep

    rs = np.random.RandomState(1)
    items = 500
    for name, groups in _group_patterns(rs, items).items():
        for n in (0, 1, 2, 64, 257, 500):
            ids = rs.permutation(items)[:n].astype(np.uint32)
            for cap in (1, 2, 3, 10, 1000):
                for k in (1, 5, 33, 600):
                    a, b, c = rule_walk(ids, groups, cap, k), rule_ordinal(ids, groups, cap, k), capped_keep(ids, groups, cap, k)
                    assert a.tolist() == b.tolist() == c.tolist(), (name, n, cap, k)
                    g = groups[ids[a]]
                    assert a.size <= k and all(np.count_nonzero(g == x) <= cap for x in np.unique(g) if x != NO_GROUP)
    # the identities: own groups, no groups, cap >= k keep the first k
    ids = rs.permutation(items).astype(np.uint32)
    pats = _group_patterns(rs, items)
    assert rule_walk(ids, pats["own"], 1, 20).tolist() == rule_walk(ids, pats["none"], 1, 20).tolist() == list(range(20))
    assert rule_walk(ids, pats["few"], 20, 20).tolist() == list(range(20))


class _FakeTop:
    """recommend_top over full rankings: row(i) is the first n entries of the named row's ranking"""

    def __init__(self, ranks, rows, n):
        self.ranks, self.rows, self.n = ranks, rows, n

    def row(self, i):
        ids, sc = self.ranks[int(self.rows[i])]
        return ids[: self.n], sc[: self.n]


def test_completion_returns_the_rule_over_the_full_ranking_and_stops_as_soon_as_it_may():
    from sbr_rs_amd.engine import capped_complete

    rs = np.random.RandomState(2)
    items, users, k, cap, pool = 3000, 40, 10, 1, 16
    groups = np.where(rs.rand(items) < 0.97, 3, np.arange(items)).astype(np.uint32)  # about 90 items outside the large group
    ranks = []
    for u in range(users):
        m = items if u % 3 else int(rs.randint(0, items))  # some rows hold fewer eligible items than the catalogue
        ids = rs.permutation(items)[:m].astype(np.uint32)
        ranks.append((ids, np.sort(rs.randn(m).astype(np.float32))[::-1].copy()))
    ranks[0] = (ranks[0][0][:5], ranks[0][1][:5])  # shorter than the pool: complete by padding
    want = capped_rows(ranks, groups, cap, k)
    gi, gs, gc = capped_rows(ranks, groups, cap, k, pool)
    assert not gc.all() and gc[0]
    first = gc.copy()
    asked = []

    def top(rows, n):
        asked.append((np.asarray(rows).copy(), int(n)))
        return _FakeTop(ranks, rows, n)

    calls = capped_complete(top, gi, gs, gc, groups, cap, k, pool, items)
    assert calls == len(asked) and gc.all()
    assert np.array_equal(gi, want[0]) and np.array_equal(gs.view(np.uint32), want[1].view(np.uint32))
    # only incomplete rows are asked for; n is 4 pool, then fourfold, never past the catalogue; a row is asked again only while the n
    # it was given neither kept k nor exhausted its ranking
    ns = sorted({n for _, n in asked})
    assert ns[0] == 4 * pool and all(b == min(4 * a, items) for a, b in zip(ns, ns[1:])) and ns[-1] <= items
    seen_at = {}
    for rows, n in asked:
        for r in rows:
            assert not first[r]
            seen_at.setdefault(int(r), []).append(n)
    assert sorted(seen_at) == np.flatnonzero(~first).tolist()
    for r, at in seen_at.items():
        ids = ranks[r][0]
        for n in at[:-1]:
            assert rule_walk(ids[:n], groups, cap, k).size < k and ids.size >= n
        assert rule_walk(ids[: at[-1]], groups, cap, k).size >= k or ids.size < at[-1] or at[-1] == items
    # batches: rows x n within max_results
    gi2, gs2, gc2 = capped_rows(ranks, groups, cap, k, pool)
    asked.clear()
    capped_complete(top, gi2, gs2, gc2, groups, cap, k, pool, items, max_results=1000)
    assert all(len(rows) * n <= 1000 or len(rows) == 1 for rows, n in asked) and len(asked) > calls
    assert np.array_equal(gi2, want[0]) and gc2.all()
    # nothing incomplete: no call
    asked.clear()
    assert capped_complete(top, gi2, gs2, gc2, groups, cap, k, pool, items) == 0 and not asked
    assert np.all(gi2[0, 5:] == NO_ITEM) and np.all(np.isneginf(gs2[0, 5:]))


def test_surface_at_every_layer():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine

    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    L = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "sbr_hip.h")).read()
    for name in CAPPED + GROUPS:
        assert name in _lib.DECLARED_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name  # the loader table gave it a signature
        assert f"sbr_status {name}(" in header
    assert ABI_VERSION == 13 and L.sbr_abi_version() == 13 and "#define SBR_ABI_VERSION 13u" in header
    assert "#define SBR_NO_GROUP 0xFFFFFFFFu" in header and "typedef struct sbr_cap_args" in header
    assert engine.NO_GROUP == 0xFFFFFFFF
    assert [engine.capped_default_pool(k) for k in (1, 16, 17, 100, 256, 1024)] == [64, 64, 68, 400, 1024, 1024]
    for fn, lead in ((engine.Model.recommend_capped, ["self", "user_ptr", "item_ids", "k"]),
                     (engine.Model.recommend_capped_reps, ["self", "reps", "k"]),
                     (engine.Sessions.recommend_capped, ["self", "slots", "k"]),
                     (sbr.lstm.ImplicitLSTMModel.recommend_capped, ["self", "interactions_or_histories", "k"]),
                     (sbr.ewma.ImplicitEWMAModel.recommend_capped_reps, ["self", "reps", "k"])):
        p = inspect.signature(fn).parameters
        assert list(p)[: len(lead)] == lead, fn
        assert p["cap"].default == 1 and p["pool"].default is None and p["exact"].default is True, fn
        assert p["any_of"].default is None and p["none_of"].default is None, fn
    assert inspect.signature(engine.Model.recommend_capped).parameters["include_history"].default is False
    assert inspect.signature(engine.Sessions.recommend_capped).parameters["include_seen"].default is False
    assert inspect.signature(sbr.lstm.ImplicitLSTMModel.recommend_capped).parameters["exclude_history"].default is True
    for cls in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel, engine.Model):
        assert callable(cls.set_item_groups) and callable(cls.item_groups)
    hpp = open(os.path.join(HERE, "..", "include", "sbr.hpp")).read()
    assert "struct CapArgs" in hpp and "void set_item_groups(" in hpp
    for name in CAPPED:
        assert name + "(" in hpp, name


def test_argument_refusals_come_before_any_library_call():
    from sbr_rs_amd import engine

    m = engine.Model.__new__(engine.Model)  # no handle and no library: reaching either is an AttributeError, not a ValueError

    class _Hp:
        num_items = 50

    m.hp = _Hp()
    st = engine.Sessions.__new__(engine.Sessions)
    ptr, ids = np.array([0, 2], np.uint64), np.array([1, 2], np.uint32)
    reps = np.zeros((1, 16), np.float32)
    for kw in ({"cap": 0}, {"cap": -1}, {"pool": 4}, {"pool": 1025}, {"k": 0}, {"k": 1025}):
        k = kw.pop("k", 5)
        with pytest.raises(ValueError):
            m.recommend_capped(ptr, ids, k, **kw)
        with pytest.raises(ValueError):
            m.recommend_capped_reps(reps, k, **kw)
        with pytest.raises(ValueError):
            st.recommend_capped([0], k, **kw)
    with pytest.raises(ValueError):
        m.set_item_groups(np.zeros(49, np.uint32))
    with pytest.raises(ValueError):
        m.set_item_groups(np.full(50, -1, np.int64))
    with pytest.raises(ValueError):
        m.set_item_groups(np.full(50, 2 ** 32, np.int64))
    with pytest.raises(ValueError):
        m.set_item_groups(np.zeros(50, np.float32))


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device behaviour")
def test_capped_calls_without_device_fail_loudly():
    import sbr_rs_amd as sbr
    from sbr_rs_amd.errors import EngineError

    build = lambda: sbr.ewma.Hyperparameters.new(50, 8).embedding_dim(16).build()  # noqa: E731
    calls = [lambda: build().set_item_groups(np.zeros(50, np.uint32)),
             lambda: build().item_groups(),
             lambda: build().recommend_capped([[1, 2, 3]], 5),
             lambda: build().recommend_capped_reps(np.zeros((1, 16), np.float32), 5, cap=2, pool=10)]
    for call in calls:
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.NO_DEVICE
    # no model, no store, no answer: the entry points compute nothing on the host
    L = _lib.load()
    out = np.full(5, 7, np.uint32)
    flag = np.full(1, 7, np.uint8)
    ptr = np.array([0, 0], np.uint64)
    word = np.zeros(1, np.uint32)
    ca = np.array([1, 0], np.uint32)  # struct sbr_cap_args {cap, pool}
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.sbr_model_set_item_groups(None, vp(word)) == Status.INVALID_ARGUMENT
    assert L.sbr_model_get_item_groups(None, vp(out)) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_capped(None, vp(ptr), None, 1, 5, 0, vp(ca), None, None, vp(out), None, vp(flag)) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_capped_reps(None, None, 1, 5, None, None, vp(ca), None, None, vp(out), None, vp(flag)) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_recommend_capped(None, vp(word), 1, 5, None, None, 0, vp(ca), None, None, vp(out), None, vp(flag)) == Status.INVALID_ARGUMENT
    assert np.all(out == 7) and flag[0] == 7


def test_cpp_program_builds_without_a_device():
    from sbr_rs_amd import build as hip_build

    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_capped_tests(verbose=False))
