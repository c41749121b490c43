"""CPU: the item-set surface at every layer — the symbols exported and declared, the descriptor's layout, the Python and C++
methods with their siblings' defaults — and the refusals that need no device: null handles and malformed descriptors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ABI_VERSION, SbrCapArgs, SbrSampleArgs, SbrScanRows, Status

HERE = os.path.dirname(os.path.abspath(__file__))
MANAGE = ("sbr_item_set_create", "sbr_item_set_destroy", "sbr_item_set_size", "sbr_item_set_items", "sbr_item_set_refresh")
SCANS = ("sbr_item_set_recommend", "sbr_item_set_recommend_diverse", "sbr_item_set_recommend_sampled", "sbr_item_set_log_partition",
         "sbr_item_set_recommend_above", "sbr_item_set_recommend_top", "sbr_item_set_recommend_capped")
FAMILIES = ("recommend", "recommend_sampled", "log_partition", "recommend_above", "count_above", "recommend_top", "nth_score",
            "recommend_capped", "recommend_diverse")


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    return _lib.load()


def test_every_symbol_is_exported_and_declared():
    L = _lib_loaded()
    header = open(os.path.join(HERE, "..", "include", "sbr_hip.h")).read()
    for name in MANAGE + SCANS:
        assert name in _lib.DECLARED_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
        assert f" {name}(" in header, name
    for name in SCANS:  # (set, const sbr_scan_rows*, num_rows, ...)
        assert f"sbr_status {name}(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows" in header, name
    assert "typedef struct sbr_item_set sbr_item_set;" in header and "typedef struct sbr_scan_rows {" in header
    assert ABI_VERSION == 13 and L.sbr_abi_version() == 13  # additions only: the version is the parent's
    # the descriptor mirrors the header's field order: ten words on a 64-bit host
    assert [f[0] for f in SbrScanRows._fields_] == ["user_ptr", "item_ids", "flags", "reps", "store", "slots", "excl_ptr", "excl_items",
                                                    "any_of", "none_of"]
    assert C.sizeof(SbrScanRows) == 80 and SbrScanRows.reps.offset == 24 and SbrScanRows.none_of.offset == 72
    doc = open(os.path.join(HERE, "..", "INTEGRATION.md")).read()
    for name in MANAGE + SCANS:
        assert name in doc, name


def test_null_handles_and_malformed_descriptors_are_argument_errors_without_a_device():
    L = _lib_loaded()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ids = np.array([1, 2], np.uint32)
    h = C.c_void_p(7)
    assert L.sbr_item_set_create(None, vp(ids), 2, C.byref(h)) == Status.INVALID_ARGUMENT and h.value == 7
    n = C.c_uint64(9)
    assert L.sbr_item_set_size(None, C.byref(n)) == Status.INVALID_ARGUMENT and n.value == 9
    assert L.sbr_item_set_items(None, vp(ids)) == Status.INVALID_ARGUMENT
    assert L.sbr_item_set_refresh(None) == Status.INVALID_ARGUMENT
    L.sbr_item_set_destroy(None)  # as every destroy: a null handle is nothing to do
    out_i, out_s, out_k = np.full(4, 7, np.uint32), np.full(4, 7, np.float32), np.full(4, 7, np.float32)
    ptr = np.array([0, 0], np.uint64)
    reps = np.zeros((1, 16), np.float32)
    th, bud = np.zeros(1, np.float32), np.ones(1, np.uint64)
    counts, total, cuts = np.full(1, 7, np.uint64), C.c_uint64(7), np.full(1, 7, np.float32)
    shift, mass, fb = np.full(1, 7, np.float32), np.full(1, 7, np.uint64), C.c_uint32(7)
    flag = np.full(1, 7, np.uint8)
    sa, ca = SbrSampleArgs(), SbrCapArgs()
    sa.temperature, ca.cap = 1.0, 1
    descriptors = {"histories": SbrScanRows(user_ptr=ptr.ctypes.data), "representations": SbrScanRows(reps=reps.ctypes.data),
                   "no source": SbrScanRows(), "two sources": SbrScanRows(user_ptr=ptr.ctypes.data, reps=reps.ctypes.data)}
    for what, d in list(descriptors.items()) + [("no descriptor", None)]:
        r = None if d is None else C.byref(d)
        calls = [L.sbr_item_set_recommend(None, r, 1, 4, vp(out_i), vp(out_s)),
                 L.sbr_item_set_recommend_diverse(None, r, 1, 2, 4, 0.5, 0, vp(out_i), vp(out_s)),
                 L.sbr_item_set_recommend_sampled(None, r, 1, 4, C.byref(sa), vp(out_i), vp(out_s), vp(out_k)),
                 L.sbr_item_set_log_partition(None, r, 1, 1.0, vp(shift), vp(mass), C.byref(fb)),
                 L.sbr_item_set_recommend_above(None, r, 1, vp(th), vp(counts), C.byref(total), 0, None, None),
                 L.sbr_item_set_recommend_top(None, r, 1, vp(bud), vp(cuts), vp(counts), C.byref(total), 0, None, None),
                 L.sbr_item_set_recommend_capped(None, r, 1, 4, C.byref(ca), vp(out_i), vp(out_s), vp(flag))]
        assert calls == [Status.INVALID_ARGUMENT] * 7, (what, calls)
    assert np.all(out_i == 7) and np.all(out_s == 7) and np.all(out_k == 7) and counts[0] == 7 and total.value == 7
    assert shift[0] == 7 and mass[0] == 7 and fb.value == 7 and flag[0] == 7 and cuts[0] == 7


def test_python_surface_has_the_siblings_names_and_defaults():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine
    from sbr_rs_amd.errors import EngineError, InvalidArgument

    assert issubclass(InvalidArgument, ValueError) and issubclass(InvalidArgument, EngineError)
    assert callable(engine.Model.item_set) and list(inspect.signature(engine.Model.item_set).parameters) == ["self", "item_ids"]
    for name in ("size", "items"):
        assert isinstance(getattr(engine.ItemSet, name), property), name
    for name in ("refresh", "close", "on"):
        assert callable(getattr(engine.ItemSet, name)), name
    for fam in FAMILIES:
        # histories and representations: Model's own signature, parameter for parameter and default for default
        for suffix in ("", "_reps"):
            mine = inspect.signature(getattr(engine.ItemSet, fam + suffix)).parameters
            theirs = inspect.signature(getattr(engine.Model, fam + suffix)).parameters
            assert list(mine) == list(theirs), (fam + suffix, list(mine), list(theirs))
            assert [p.default for p in mine.values()] == [p.default for p in theirs.values()], fam + suffix
        # a store: Sessions' own
        mine = inspect.signature(getattr(engine.ItemSetSessions, fam)).parameters
        theirs = inspect.signature(getattr(engine.Sessions, fam)).parameters
        assert list(mine) == list(theirs), (fam, list(mine), list(theirs))
        assert [p.default for p in mine.values()] == [p.default for p in theirs.values()], fam
    # the model wrappers: item_set returns the history-level view, with the wrappers' keywords
    for cls in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel):
        assert callable(cls.item_set)
    from sbr_rs_amd.lstm import ItemSetView

    for fam in FAMILIES:
        mine = inspect.signature(getattr(ItemSetView, fam)).parameters
        theirs = {n: p for n, p in inspect.signature(getattr(sbr.lstm.ImplicitLSTMModel, fam)).parameters.items() if n != "among"}
        assert list(mine) == list(theirs), (fam, list(mine), list(theirs))
        assert [p.default for p in mine.values()] == [p.default for p in theirs.values()], fam
    # recommend(among=) with a filter stays a ValueError, and now says where to go
    src = inspect.getsource(sbr.lstm._ImplicitSequenceModel.recommend)
    assert "item_set" in src


def test_python_refusals_come_before_any_library_call():
    from sbr_rs_amd import engine

    s = engine.ItemSet.__new__(engine.ItemSet)  # no handle and no library: reaching either is an AttributeError, not a ValueError

    class _Model:
        dim = 16

    s.model = _Model()
    reps = np.zeros((2, 16), np.float32)
    with pytest.raises(ValueError):
        s.recommend_reps(reps, 3, exclude=[[1]])  # one list per row
    with pytest.raises(ValueError):
        s.recommend_reps(reps, 3, any_of=[1, 2, 3])  # one mask per row
    with pytest.raises(ValueError):
        s.recommend_sampled_reps(reps, 3, streams=[1])
    with pytest.raises(ValueError):
        s.recommend_above_reps(reps, np.nan)
    with pytest.raises(ValueError):
        s.recommend_top_reps(reps, -1)
    with pytest.raises(ValueError):
        s.recommend_capped_reps(reps, 3, cap=0)

    class _Hp:
        num_items = 50

    m = engine.Model.__new__(engine.Model)
    m.hp = _Hp()
    for bad in ([50], [-1], [3, 2 ** 32]):
        with pytest.raises(ValueError):
            engine.ItemSet(m, bad)


def test_cpp_surface_and_program_build_without_a_device():
    from sbr_rs_amd import build as hip_build

    hpp = open(os.path.join(HERE, "..", "include", "sbr.hpp")).read()
    assert "class ItemSet {" in hpp and "ItemSet item_set(const std::vector<std::uint32_t>& item_ids) const" in hpp
    assert "OnSessions on(const Sessions& store) const" in hpp and "using ItemSet = models::ItemSet;" in hpp
    for name in MANAGE + SCANS:
        assert name + "(" in hpp, name
    for method in ("recommend", "recommend_reps", "recommend_sampled", "recommend_sampled_reps", "log_partition", "log_partition_reps",
                   "recommend_above", "recommend_above_reps", "recommend_top", "recommend_top_reps", "recommend_capped",
                   "recommend_capped_reps", "recommend_diverse", "recommend_diverse_reps", "count_above", "refresh", "items", "size"):
        assert f" {method}(" in hpp.split("class ItemSet {")[1].split("/// Owner of the device replicas")[0], method
    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_item_set_tests(verbose=False))


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device behaviour")
def test_item_set_without_a_device_fails_loudly():
    import sbr_rs_amd as sbr
    from sbr_rs_amd.errors import EngineError

    with pytest.raises(EngineError) as e:
        sbr.ewma.Hyperparameters.new(50, 8).embedding_dim(16).build().item_set([1, 2, 3])
    assert e.value.status == Status.NO_DEVICE
