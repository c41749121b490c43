"""CPU: the expectation the GPU tests of the tag filter use (filter_expect.py) on its own, and what of the Python and C++ layers
needs no device: the mask arguments, the surface at every layer, and the refusal to run without a device."""
import ctypes as C
import os

import numpy as np
import pytest

from filter_expect import allowed, disallowed, equivalent_exclusions, filtered_expect, filtered_topk_expectation
from helpers import LOSS_HINGE, hparams
from recommend_expect import NO_ITEM, topk_expectation
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ModelKind, Status

FILTERED = ("sbr_recommend_filtered", "sbr_recommend_filtered_reps", "sbr_sessions_recommend_filtered", "sbr_recommend_diverse_filtered",
            "sbr_recommend_diverse_filtered_reps", "sbr_sessions_recommend_diverse_filtered", "sbr_similar_items_filtered")


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def _case(seed, items=200):
    rs = np.random.RandomState(seed)
    scores = np.round(rs.randn(items), 1).astype(np.float32)  # many exact ties
    tags = np.zeros(items, np.uint32)
    for _ in range(4):
        tags |= (np.uint32(1) << rs.randint(0, 31, items).astype(np.uint32)).astype(np.uint32)  # bit 31 stays free
    tags[::9] = 0
    return scores, tags


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("seed", range(4))
def test_allowed_is_the_contracts_formula(seed):
    scores, tags = _case(seed)
    rs = np.random.RandomState(seed + 10)
    for _ in range(20):
        a, n = (int(rs.randint(0, 2 ** 32)) & int(rs.randint(0, 2 ** 32)) & int(rs.randint(0, 2 ** 32)) for _ in range(2))
        want = [(int(t) & n) == 0 and (a == 0 or (int(t) & a) != 0) for t in tags]
        assert allowed(tags, a, n).tolist() == want
        assert disallowed(tags, a, n).tolist() == [i for i, w in enumerate(want) if not w]


@pytest.mark.parametrize("seed", range(4))
def test_expectation_properties(seed):
    """All-zero masks equal no filter; none_of = 0xFFFFFFFF leaves exactly the tag-0 items; an any_of bit that no item has gives a
    row of padding; the row never holds a disallowed or an excluded item, and is the plain row of the allowed items."""
    scores, tags = _case(seed)
    items = scores.size
    excluded = np.random.RandomState(seed).randint(0, items, 15)
    for k in (1, 10, items + 5):
        for ex in ((), excluded):
            plain = topk_expectation(scores, ex, k)
            got = filtered_topk_expectation(scores, tags, 0, 0, ex, k)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(_bits(got[1]), _bits(plain[1]))
        gi, gs = filtered_topk_expectation(scores, tags, 0, 0xFFFFFFFF, (), k)
        zero = np.flatnonzero(tags == 0)
        assert set(gi[gi != NO_ITEM].tolist()) <= set(zero.tolist())
        if k >= zero.size:
            assert set(gi[gi != NO_ITEM].tolist()) == set(zero.tolist()) and np.all(gi[zero.size:] == NO_ITEM) and np.all(np.isneginf(gs[zero.size:]))
        gi, gs = filtered_topk_expectation(scores, tags, 1 << 31, 0, (), k)
        assert np.all(gi == NO_ITEM) and np.all(np.isneginf(gs))
        a, n = 0b1011, 1 << 7
        gi, gs = filtered_topk_expectation(scores, tags, a, n, excluded, k)
        real = gi[gi != NO_ITEM]
        ok = allowed(tags, a, n)
        assert np.all(ok[real]) and not set(real.tolist()) & set(excluded.tolist())
        keep = np.flatnonzero(ok & ~np.isin(np.arange(items), excluded))
        sub = topk_expectation(scores[keep], (), k)  # the plain top k of the eligible items alone (ids ascending: ties alike)
        assert np.array_equal(real, keep[sub[0][sub[0] != NO_ITEM]]) and np.array_equal(_bits(gs[: real.size]), _bits(sub[1][: real.size]))


def test_rows_and_equivalent_exclusions():
    scores, tags = _case(7)
    users = 6
    S = np.stack([np.roll(scores, u) for u in range(users)])
    any_of = np.array([0, 1, 0, 6, 1 << 31, 0], np.uint32)
    none_of = np.array([0, 0, 8, 1, 0, 0xFFFFFFFF], np.uint32)
    own = [np.arange(u, dtype=np.uint32) for u in range(users)]
    rows = filtered_expect(S, tags, any_of, none_of, own, 12)
    eq = equivalent_exclusions(tags, any_of, none_of, users, own)
    for u in range(users):
        want = topk_expectation(S[u], eq[u], 12)
        assert np.array_equal(rows[0][u], want[0]) and np.array_equal(_bits(rows[1][u]), _bits(want[1]))
    assert np.all(rows[0][4] == NO_ITEM)
    # a scalar mask is every user's
    a = filtered_expect(S, tags, 6, None, None, 5)
    b = filtered_expect(S, tags, np.full(users, 6, np.uint32), np.zeros(users, np.uint32), None, 5)
    assert np.array_equal(a[0], b[0])


def test_mask_arguments_of_the_python_layer():
    from sbr_rs_amd import engine

    assert engine._tag_masks(None, None, 5) is None  # the plain entry point is used
    a, n = engine._tag_masks(3, None, 4)
    assert a.dtype == np.uint32 and a.tolist() == [3] * 4 and n.tolist() == [0] * 4
    a, n = engine._tag_masks(None, 0xFFFFFFFF, 2)
    assert a.tolist() == [0, 0] and n.tolist() == [0xFFFFFFFF] * 2
    a, n = engine._tag_masks([1, 2, 1 << 31], np.uint32(4), 3)
    assert a.tolist() == [1, 2, 1 << 31] and n.tolist() == [4, 4, 4]
    for bad in ([1, 2], np.zeros(4, np.uint32), []):
        with pytest.raises(ValueError):
            engine._tag_masks(bad, None, 3)
        with pytest.raises(ValueError):
            engine._tag_masks(None, bad, 3)
    # the wrappers raise before they reach the library: a model without a handle never gets that far
    m = engine.Model._from_handle(hparams(50, 8, 16, int(ModelKind.EWMA), LOSS_HINGE), None)
    reps = np.zeros((3, 16), np.float32)
    ptr, ids = np.array([0, 1, 2, 3], np.uint64), np.array([1, 2, 3], np.uint32)
    with pytest.raises(ValueError):
        m.recommend_reps(reps, 5, any_of=[1, 2])
    with pytest.raises(ValueError):
        m.recommend(ptr, ids, 5, none_of=[1, 2, 3, 4])
    with pytest.raises(ValueError):
        m.recommend_diverse_reps(reps, 2, 4, any_of=[1])
    with pytest.raises(ValueError):
        m.recommend_diverse(ptr, ids, 2, 4, none_of=[1])
    with pytest.raises(ValueError):
        m.similar_items([1, 2], 5, any_of=[1, 2, 3])
    with pytest.raises(ValueError):
        m.set_item_tags(np.zeros(49, np.uint32))
    st = engine.Sessions.__new__(engine.Sessions)
    with pytest.raises(ValueError):
        st.recommend([0, 1], 5, any_of=[1])
    with pytest.raises(ValueError):
        st.recommend_diverse([0, 1], 2, 4, none_of=[1, 2, 3])


def test_among_together_with_a_filter_is_refused():
    import sbr_rs_amd as sbr

    for cls in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel):
        model = cls.__new__(cls)  # no engine model: the refusal comes before any call into it
        for kw in ({"any_of": 1}, {"none_of": [1, 2]}, {"any_of": 0, "none_of": 0}):
            with pytest.raises(ValueError):
                model.recommend([[1, 2], [3]], 5, among=[1, 2, 3], **kw)


def test_surface_at_every_layer():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine
    import inspect

    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    L = _lib.load()
    for name in FILTERED + ("sbr_model_set_item_tags", "sbr_model_get_item_tags"):
        assert name in _lib.DECLARED_SYMBOLS and hasattr(L, name), name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sbr_hip.h")).read()
    for name in FILTERED + ("sbr_model_set_item_tags", "sbr_model_get_item_tags"):
        assert f"sbr_status {name}(" in header
    for fn in (engine.Model.recommend, engine.Model.recommend_reps, engine.Model.recommend_diverse, engine.Model.recommend_diverse_reps,
               engine.Model.similar_items, engine.Sessions.recommend, engine.Sessions.recommend_diverse):
        p = inspect.signature(fn).parameters
        assert p["any_of"].default is None and p["none_of"].default is None, fn
    for cls in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel, engine.Model):
        assert callable(cls.set_item_tags) and callable(cls.item_tags)
    for name in ("recommend", "recommend_diverse", "similar_items"):
        p = inspect.signature(getattr(sbr.lstm.ImplicitLSTMModel, name)).parameters
        assert "any_of" in p and "none_of" in p
    hpp = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sbr.hpp")).read()
    assert "struct TagFilter" in hpp and "void set_item_tags(" in hpp
    for name in FILTERED:  # the facade has no *_reps calls at all
        assert name.endswith("_reps") or name + "(" in hpp, name


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device behaviour")
def test_filtered_calls_without_device_fail_loudly():
    import sbr_rs_amd as sbr
    from sbr_rs_amd.errors import EngineError

    build = lambda: sbr.ewma.Hyperparameters.new(50, 8).embedding_dim(16).build()  # noqa: E731
    calls = [lambda: build().set_item_tags(np.zeros(50, np.uint32)),
             lambda: build().recommend([[1, 2, 3]], 5, any_of=1),
             lambda: build().recommend_diverse([[1, 2, 3]], 5, none_of=[2]),
             lambda: build().similar_items([1, 2, 3], 5, any_of=[1, 2, 4])]
    for call in calls:
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == Status.NO_DEVICE
    # no model, no store, no answer: the entry points compute nothing on the host
    L = _lib.load()
    out = np.full(5, 7, np.uint32)
    ptr = np.array([0, 0], np.uint64)
    mask = np.zeros(1, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.sbr_model_set_item_tags(None, vp(mask)) == Status.INVALID_ARGUMENT
    assert L.sbr_model_get_item_tags(None, vp(out)) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_filtered(None, vp(ptr), None, 1, 5, 0, vp(mask), vp(mask), vp(out), None) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_filtered_reps(None, None, 1, 5, None, None, vp(mask), vp(mask), vp(out), None) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_diverse_filtered(None, vp(ptr), None, 1, 2, 4, 0.5, 0, 0, vp(mask), vp(mask), vp(out), None) == Status.INVALID_ARGUMENT
    assert L.sbr_recommend_diverse_filtered_reps(None, None, 1, 2, 4, 0.5, 0, None, None, vp(mask), vp(mask), vp(out), None) == Status.INVALID_ARGUMENT
    assert L.sbr_similar_items_filtered(None, vp(mask), 1, 5, 0, 0, None, None, vp(mask), vp(mask), vp(out), None) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_recommend_filtered(None, vp(mask), 1, 5, None, None, 0, vp(mask), vp(mask), vp(out), None) == Status.INVALID_ARGUMENT
    assert L.sbr_sessions_recommend_diverse_filtered(None, vp(mask), 1, 2, 4, 0.5, 0, None, None, vp(mask), vp(mask), vp(out), None) == Status.INVALID_ARGUMENT
    assert np.all(out == 7)


def test_cpp_program_builds_without_a_device():
    from sbr_rs_amd import build as hip_build

    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_filtered_tests(verbose=False))
