"""CPU: the expectation the GPU tests of recommend_diverse use (diverse_expect.py) on its own — the contract's consequences and the
clustered table's condition — and what of the Python and C++ layers needs no device."""
import os

import numpy as np
import pytest

from diverse_expect import DiverseExpectation, clustered_case, pool_from_reps
from helpers import LOSS_HINGE, hparams
from oracle.oracle import OracleModel
from recommend_expect import NO_ITEM
from sbr_rs_amd import _lib
from sbr_rs_amd._abi import ModelKind, Param


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oracle(E, bias):
    items, d = E.shape
    o = OracleModel(hparams(items, 8, d, int(ModelKind.EWMA), LOSS_HINGE))
    o.set_param(Param.ITEM_EMBEDDING, E)
    o.set_param(Param.ITEM_BIAS, bias)
    return o


def test_trade_off_one_is_the_plain_top_k_and_pool_k_a_permutation():
    items, d, users = 500, 24, 30
    rs = np.random.RandomState(1)
    E = (rs.randn(items, d) * 0.3).astype(np.float32)
    E[rs.choice(np.arange(10, items), 20, replace=False)] = E[0]
    bias = np.round(rs.randn(items) * 0.5, 1).astype(np.float32)
    reps = (rs.randn(users, d) * 0.5).astype(np.float32)
    o = _oracle(E, bias)
    excl = [rs.randint(0, items, 5) for _ in range(users)]
    excl[3] = np.arange(items - 4)  # n = 4 < k
    for metric in ("cosine", "dot"):
        want = DiverseExpectation(E, metric)
        for k, pool in ((1, 1), (10, 10), (10, 64), (33, 65)):
            wide = pool_from_reps(o, items, reps, pool, excl)
            plain = pool_from_reps(o, items, reps, k, excl)
            one = want.rows(wide, k, 1.0)
            assert np.array_equal(one[0], plain[0]) and np.array_equal(_bits(one[1]), _bits(plain[1]))
            for t in (0.0, 0.3):
                gi, gs = want.rows(wide, k, t)
                assert np.array_equal(gi[:, 0], plain[0][:, 0])  # pick 0 is the best item
                assert np.all(gi[3, 4:] == NO_ITEM) and np.all(np.isneginf(gs[3, 4:])) and np.all(gi[3, : min(k, 4)] != NO_ITEM)
                for u in range(users):
                    row = gi[u][gi[u] != NO_ITEM]
                    assert len(set(row.tolist())) == row.size and set(row.tolist()) <= set(wide[0][u].tolist())
                    at = {int(i): b for i, b in zip(wide[0][u], _bits(wide[1][u]))}
                    assert [at[int(i)] for i in row] == _bits(gs[u][: row.size]).tolist()
                if pool == k:
                    assert np.array_equal(np.sort(gi, axis=1), np.sort(plain[0], axis=1))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("d", [16, 100, 128, 256])
def test_clustered_table_meets_its_condition(d, seed):
    """k = 10 of a pool of 64 at trade_off 0.3, cosine: at least 36 of the 40 rows differ from the plain top 10, and the mean number
    of distinct clusters per row goes from one (1.0 - 1.1: the plain list is copies of the favourite cluster) to at least two."""
    E, bias, reps = clustered_case(d, seed)
    o = _oracle(E, bias)
    items = E.shape[0]
    plain = pool_from_reps(o, items, reps, 10)
    got = DiverseExpectation(E, "cosine").rows(pool_from_reps(o, items, reps, 64), 10, 0.3)
    differ = int(np.count_nonzero(np.any(got[0] != plain[0], axis=1)))
    assert differ >= 36, differ
    before, after = (float(np.mean([len(set((r % 12).tolist())) for r in rows])) for rows in (plain[0], got[0]))
    assert 1.0 <= before <= 1.1 and after >= 2.0, (before, after)


def test_surface_and_argument_validation_without_a_device():
    import sbr_rs_amd as sbr
    from sbr_rs_amd import engine

    if not os.path.exists(_lib.LIB_PATH):
        from sbr_rs_amd import build

        build.build(verbose=False)
    L = _lib.load()
    for name in ("sbr_recommend_diverse_max_pool", "sbr_recommend_diverse", "sbr_recommend_diverse_reps", "sbr_sessions_recommend_diverse"):
        assert name in _lib.DECLARED_SYMBOLS and hasattr(L, name)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sbr_hip.h")).read()
    assert "#define SBR_DIVERSE_MAX_POOL 1024u" in header
    for mod in (sbr.lstm.ImplicitLSTMModel, sbr.ewma.ImplicitEWMAModel):
        assert callable(getattr(mod, "recommend_diverse"))
    for name in ("recommend_diverse", "recommend_diverse_reps", "diverse_max_pool"):
        assert callable(getattr(engine.Model, name))
    assert callable(engine.Sessions.recommend_diverse)
    # what the wrappers refuse before they reach the library: a metric by an unknown name, exclusion lists that do not match the users
    m = engine.Model._from_handle(hparams(50, 8, 16, int(ModelKind.EWMA), LOSS_HINGE), None)
    with pytest.raises(ValueError):
        m.recommend_diverse_reps(np.zeros((2, 16), np.float32), 3, 8, metric="euclid")
    with pytest.raises(ValueError):
        m.recommend_diverse(np.array([0, 1], np.uint64), np.array([1], np.uint32), 3, 8, metric="euclid")
    with pytest.raises(ValueError):
        m.recommend_diverse_reps(np.zeros((2, 16), np.float32), 3, 8, exclude=[[1]])
    # no model, no answer: the entry points compute nothing on the host
    import ctypes as C

    from sbr_rs_amd._abi import Status

    out = np.full(4, 7, np.uint32)
    n = C.c_uint32(5)
    assert L.sbr_recommend_diverse_max_pool(None, C.byref(n)) == Status.INVALID_ARGUMENT and n.value == 5
    assert L.sbr_recommend_diverse_reps(None, None, 1, 2, 4, 0.5, 0, None, None, out.ctypes.data_as(C.c_void_p), None) == Status.INVALID_ARGUMENT
    assert np.all(out == 7)


def test_cpp_program_builds_without_a_device():
    from sbr_rs_amd import build as hip_build

    hip_build.build(verbose=False)
    assert os.path.exists(hip_build.build_diverse_tests(verbose=False))
