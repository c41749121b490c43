"""CPU: the guarded-scratch hook's two entry points (SBR_TEST_GUARD; include/sbr_hip.h) are declared, exported and
loadable; they are additions, so the ABI version is 13 in header, loader and library; and without a device both answer NO_DEVICE
and leave the caller's memory alone.  What the hook sees is tests/test_guarded_scratch_gpu.py's."""
import ctypes as C
import os
import re

import pytest

from sbr_rs_amd import _abi, _lib
from sbr_rs_amd._abi import SbrGuardReport, Status
from test_abi import _declared_in_header, _have_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sbr_test_guard_report", "sbr_selftest_guard")


def _header():
    return open(os.path.join(ROOT, "include", "sbr_hip.h")).read()


def test_entry_points_are_declared_and_exported():
    L = _lib.load()
    declared = _declared_in_header()
    for name in NAMES:
        assert name in declared and name in _lib.DECLARED_SYMBOLS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == {"sbr_test_guard_report": 2, "sbr_selftest_guard": 4}[name]


def test_abi_version_stays_13():
    assert int(re.search(r"#define\s+SBR_ABI_VERSION\s+(\d+)", _header()).group(1)) == 13
    assert _abi.ABI_VERSION == 13 and _lib.load().sbr_abi_version() == 13


def test_report_struct_and_places_match_the_header():
    body = re.search(r"typedef struct sbr_guard_report \{(.*?)\} sbr_guard_report;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(u?int64_t)\s+(\w+);", body)
    ctype = {"uint64_t": C.c_uint64, "int64_t": C.c_int64}
    assert [(n, ctype[t]) for t, n in fields] == list(SbrGuardReport._fields_)
    assert C.sizeof(SbrGuardReport) == 8 * len(fields) == 72
    places = dict(re.findall(r"\b(SBR_GUARD_[A-Z_]+) = (\d+)", _header()))
    assert {k: int(v) for k, v in places.items()} == {
        "SBR_GUARD_NONE": _abi.GUARD_NONE, "SBR_GUARD_DEVICE_BLOCK": _abi.GUARD_DEVICE_BLOCK, "SBR_GUARD_PINNED_BLOCK": _abi.GUARD_PINNED_BLOCK,
        "SBR_GUARD_ARENA_TAKE": _abi.GUARD_ARENA_TAKE, "SBR_GUARD_BIG_BLOCK": _abi.GUARD_BIG_BLOCK}


def test_a_report_reads_as_a_sentence():
    r = SbrGuardReport(blocks=3, takes=2, bytes=99, violations=1, where=_abi.GUARD_ARENA_TAKE, ordinal=4, requested=4196, offset=-1, changed=1)
    assert r.checked == 5 and r.first() == (_abi.GUARD_ARENA_TAKE, 4, 4196, -1, 1)
    assert "arena take #4" in str(r) and "1 bytes before its start" in str(r)
    assert SbrGuardReport().first() is None and "0 violated" in str(SbrGuardReport())


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device behaviour")
@pytest.mark.parametrize("hook", [None, "256"])
def test_no_device_answers_and_touches_nothing(monkeypatch, hook):
    if hook is None:
        monkeypatch.delenv("SBR_TEST_GUARD", raising=False)
    else:
        monkeypatch.setenv("SBR_TEST_GUARD", hook)
    L = _lib.load()
    buf = (C.c_uint8 * (2 * C.sizeof(SbrGuardReport)))(*([7] * (2 * C.sizeof(SbrGuardReport))))
    assert L.sbr_test_guard_report(None, buf) == Status.NO_DEVICE and all(b == 7 for b in buf)
    for where in (_abi.GUARD_DEVICE_BLOCK, _abi.GUARD_PINNED_BLOCK, _abi.GUARD_ARENA_TAKE, _abi.GUARD_BIG_BLOCK):
        for side in (1, -1):
            assert L.sbr_selftest_guard(None, where, side, buf) == Status.NO_DEVICE and all(b == 7 for b in buf)
