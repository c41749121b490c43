"""CPU: the statement of recommend_sampled's noise that the GPU tests hold the device to (tests/sampled_expect.py) is itself what
the contract says it is — an accurate standard Gumbel variate per (seed, stream, item), independent across streams and items, whose
arg-max over keys draws from softmax(score / T) — and the expectation built on it has the contract's shape.  Nothing here runs
the engine."""
import functools

import numpy as np
import pytest

from recommend_expect import NO_ITEM
from sampled_expect import (gumbel_of_r, hash_r, inv_temperature, keys_of, log32, mix64, noise, row_keys, sampled_expect,
                            sampled_expectation, unit_of_r)

EULER_GAMMA = 0.5772156649015329
STREAMS = np.arange(200000, dtype=np.uint64)
CHI2_7_0001 = 24.32  # the 0.001 point of chi-square at 7 degrees of freedom
SCORES = np.array([0.5, -1, 2, 0, 1.5, -0.25, 1, 0.75], np.float32)
ITEM_SETS = {"0..7": np.arange(8), "1000..1007": np.arange(1000, 1008), "scattered": np.array([3, 7, 64, 65, 4096, 99999, 100000, 999999])}


@functools.lru_cache(maxsize=None)
def _all_g():
    g = gumbel_of_r(np.arange(1 << 23, dtype=np.uint32))
    g.setflags(write=False)
    return g


def test_noise_is_accurate_over_every_noise_value():
    """|noise - float64 (-log(-log u))| <= 1e-6 over all 2^23 values of r (measured: 5.7e-7), every value finite, u exact."""
    r = np.arange(1 << 23, dtype=np.uint32)
    u = unit_of_r(r)
    assert u.dtype == np.float32 and u.min() > 0 and u.max() < 1
    assert np.array_equal(u.astype(np.float64), (2.0 * r.astype(np.float64) + 1.0) * 2.0 ** -24)
    g = _all_g()
    assert g.dtype == np.float32 and np.all(np.isfinite(g))
    err = np.abs(g.astype(np.float64) - -np.log(-np.log(u.astype(np.float64)))).max()
    print("max |g - float64|", err, "range", g.min(), g.max())
    assert err <= 1e-6
    assert -2.85 <= g.min() and g.max() == np.float32(16.635532)


def test_noise_never_decreases_in_its_bits():
    """The scan's two bounds take the largest noise of a range of r to be the noise of the range's last r: that needs the computed
    g — not just the exact one — to be monotone in r."""
    assert np.all(np.diff(_all_g()) >= 0)
    assert np.mean(_all_g() <= 3.5) > 0.97


def test_log32_against_float64():
    rs = np.random.RandomState(0)
    x = np.concatenate([np.exp(rs.uniform(-80, 80, 200000)), [1.0, 2.0, 0.5, 1.41421356, 1.4142137, 2.0 ** -126, 3.4e38]]).astype(np.float32)
    got = log32(x).astype(np.float64)
    want = np.log(x.astype(np.float64))
    assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 2e-7
    assert log32(np.float32(1.0)) == 0.0


def test_row_keys_are_the_epoch_key_construction():
    assert mix64(0) == 0 and mix64(2 ** 64) == 0 and mix64(1) != mix64(2)
    k0, k1 = row_keys(7, [0, 1, 2 ** 63 + 5])
    for j, s in enumerate([0, 1, 2 ** 63 + 5]):
        K = mix64(7 ^ mix64((s * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1)))
        assert int(k0[j]) == K & 0xFFFFFFFF and int(k1[j]) == K >> 32
    assert hash_r(k0, k1, np.array([1, 2, 3], np.uint32)).max() < 1 << 23


def test_mean_and_variance():
    """Within 0.01 of gamma and pi^2 / 6 on 200 000 streams (seed 1, item 0: 0.5763 and 1.6354), and — without any sampling error —
    within 0.001 over all 2^23 equally likely values of the noise bits (0.577216 and 1.644933).  The sample variance of 200 000
    Gumbel draws scatters by 0.0077 (one sigma: sqrt((kurtosis - 1) / n) * pi^2 / 6, kurtosis 5.4), so 0.01 is a 1.3-sigma bound
    that a perfect generator misses for one configuration in five; the configuration is therefore fixed, not swept."""
    a = noise(1, STREAMS, np.array([0], np.uint32))[:, 0].astype(np.float64)
    print("200 000 streams: mean", a.mean(), "var", a.var())
    assert abs(a.mean() - EULER_GAMMA) < 0.01 and abs(a.var() - np.pi ** 2 / 6) < 0.01
    g = _all_g().astype(np.float64)
    print("all r: mean", g.mean(), "var", g.var())
    assert abs(g.mean() - EULER_GAMMA) < 0.001 and abs(g.var() - np.pi ** 2 / 6) < 0.001


@pytest.mark.parametrize("seed", [1, 2, 3, 12345])
def test_correlations(seed):
    """Adjacent streams on one item and adjacent items on one stream are uncorrelated: |rho| < 0.01 on 200 000 pairs (one sigma is
    0.0022; measured 0.0018 and -0.0020 for seed 1)."""
    g = noise(seed, STREAMS, np.array([0, 1], np.uint32)).astype(np.float64)
    rho_streams = np.corrcoef(g[:-1, 0], g[1:, 0])[0, 1]
    rho_pair = np.corrcoef(g[:, 0], g[:, 1])[0, 1]
    one_stream = noise(seed, [17], np.arange(200001, dtype=np.uint32))[0].astype(np.float64)
    rho_items = np.corrcoef(one_stream[:-1], one_stream[1:])[0, 1]
    print("rho adjacent streams", rho_streams, "items 0 and 1 across streams", rho_pair, "adjacent items on one stream", rho_items)
    assert abs(rho_streams) < 0.01 and abs(rho_pair) < 0.01 and abs(rho_items) < 0.01


@pytest.mark.parametrize("seed", [1, 2, 3, 12345])
@pytest.mark.parametrize("temperature", [0.5, 1.0, 3.0])
@pytest.mark.parametrize("which", list(ITEM_SETS))
def test_first_pick_follows_the_softmax(which, temperature, seed):
    """Chi-square of the first pick's frequencies over 200 000 streams against softmax(score / T), 8 items: below the 0.001 point
    at 7 degrees of freedom."""
    ids = ITEM_SETS[which].astype(np.uint32)
    inv_t = inv_temperature(temperature)
    keys = keys_of(SCORES[None, :], inv_t, noise(seed, STREAMS, ids))
    first = np.argmax(keys, axis=1)
    counts = np.bincount(first, minlength=8).astype(np.float64)
    z = SCORES.astype(np.float64) / temperature
    p = np.exp(z - z.max())
    p /= p.sum()
    stat = float(np.sum((counts - STREAMS.size * p) ** 2 / (STREAMS.size * p)))
    print(which, temperature, seed, "chi2", stat)
    assert stat < CHI2_7_0001


def test_noise_depends_on_seed_stream_and_item_only():
    items = np.array([3, 99, 100000], np.uint32)
    whole = noise(9, [4, 5, 6], items)
    assert np.array_equal(noise(9, [5], items[1:2]), whole[1:2, 1:2])      # not on the batch or the item set
    assert np.array_equal(noise(9, [6, 4], items)[::-1], whole[[0, 2]])    # not on the row's position
    assert np.all(noise(10, [4, 5, 6], items) != whole)
    assert noise(9, [2 ** 40 + 4], items)[0, 0] != whole[0, 0]             # all 64 bits of a stream count


def test_expectation_shape_order_padding_and_scores():
    rs = np.random.RandomState(3)
    n, items, k = 6, 50, 12
    scores = rs.randn(n, items).astype(np.float32)
    excl = [rs.choice(items, rs.randint(0, 45), replace=False) for _ in range(n)]
    excl[2] = np.arange(items)
    it, sc, keys = sampled_expect(scores, excl, k, 0.7, seed=4)
    g = noise(4, np.arange(n), np.arange(items))
    full = keys_of(scores, inv_temperature(0.7), g)
    for u in range(n):
        real = it[u] != NO_ITEM
        m = int(real.sum())
        assert m == min(k, items - len(set(excl[u].tolist()))) and np.all(real[:m])
        assert not set(it[u][:m].tolist()) & set(excl[u].tolist())
        assert np.array_equal(keys[u][:m], full[u][it[u][:m]]) and np.array_equal(sc[u][:m], scores[u][it[u][:m]])
        assert np.all(np.diff(keys[u][:m]) <= 0)
        assert np.all(np.isneginf(keys[u][m:])) and np.all(np.isneginf(sc[u][m:]))
    assert np.all(it[2] == NO_ITEM)
    # k is a prefix property, streams carry the noise, a tie goes to the lower id
    a = sampled_expect(scores, excl, 5, 0.7, seed=4)
    assert all(np.array_equal(x[:, :5], y) for x, y in zip((it, sc, keys), a))
    b = sampled_expect(scores[3:4], excl[3:4], k, 0.7, seed=4, streams=[3])
    assert all(np.array_equal(x[3:4], y) for x, y in zip((it, sc, keys), b))
    ti, _, tk = sampled_expectation(np.zeros(4, np.float32), (), 4, np.float32(1.0), np.array([1, 2, 2, 1], np.float32))
    assert ti.tolist() == [1, 2, 0, 3] and tk.tolist() == [2, 2, 1, 1]


def test_small_temperature_is_the_argmax():
    """Gaps of 0.05 at T = 1e-3: gap / T = 50 exceeds the noise's whole range (19.5), so the draw is the sort."""
    scores = (np.arange(40)[::-1] * 0.05).astype(np.float32)[None, :]
    it, sc, _ = sampled_expect(scores, None, 10, 1e-3, seed=1)
    assert it[0].tolist() == list(range(10)) and np.array_equal(sc[0], scores[0][:10])
    assert float(_all_g().max()) - float(_all_g().min()) < 19.5
