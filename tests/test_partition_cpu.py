"""CPU: the host statement of log_partition's weight chain (sbr_softmax_weights / sbr_softmax_frac_bits, which need no device) is
the numpy statement of tests/partition_expect.py bit for bit; the exponential is accurate, monotone and exactly 1 at 0; the slate
probabilities are exact-integer Plackett-Luce; and the weights are the distribution recommend_sampled's noise draws from."""
import numpy as np
import pytest

from partition_expect import (exp32, fix, frac_bits, log_z_expect, partition_expect, slate_log_prob_expect, weights)
from sampled_expect import inv_temperature, keys_of, noise
from sbr_rs_amd import engine

F = np.float32
EXP32_MAX_REL = 2.54e-7  # the recorded figure: test_exp32_recorded_figures measures it, 2.536e-7
CHI2_23_0001 = 49.73    # the 0.001 point of chi-square at 23 degrees of freedom


@pytest.fixture(scope="module")
def sweep():
    d = np.unique(np.concatenate([np.linspace(-70, 0, 1_200_001), -np.exp(np.linspace(-30, np.log(70), 300_000))]).astype(F))
    d.setflags(write=False)
    return d


@pytest.mark.parametrize("fbits", [40, 39, 31, 17, 0])
def test_weights_are_the_numpy_statement(sweep, fbits):
    """Integer equality over a dense sweep of d in [-70, 0] (1.5 M values) and the edges: 0, -64, just below it, positive d,
    non-finite scores."""
    assert sweep.size >= 1_000_000
    got = engine.softmax_weights(sweep, 1.0, 0.0, fbits)
    assert got.dtype == np.uint64 and np.array_equal(got, weights(sweep, 1.0, F(0), fbits))
    below = np.nextafter(F(-64), F(-np.inf))
    edges = np.array([0.0, -0.0, -64.0, below, 1e-30, 1.0, 80.0, -1e-30, np.inf, -np.inf, np.nan], F)
    w = engine.softmax_weights(edges, 1.0, 0.0, fbits)
    assert np.array_equal(w, weights(edges, 1.0, F(0), fbits))
    assert int(w[0]) == 1 << fbits and int(w[1]) == 1 << fbits  # the arg-max weighs exactly 2^F
    assert int(w[2]) == int(fix(exp32(F(-64)), fbits)) and not w[3:7].any() and not w[8:].any()


@pytest.mark.parametrize("temperature,shift", [(0.5, 3.25), (2.0, -1.5), (1e-3, 700.0), (7.0, 0.0)])
def test_weights_scale_and_shift(temperature, shift):
    rs = np.random.RandomState(5)
    s = (rs.randn(50000) * 3).astype(F)
    got = engine.softmax_weights(s, temperature, shift, 39)
    assert np.array_equal(got, weights(s, temperature, F(shift), 39))
    assert not got[s * inv_temperature(temperature) > F(shift)].any()  # d > 0: the clamp


def test_an_empty_rows_shift_gives_no_weight():
    s = np.array([0.0, 5.0, -5.0, -np.inf], F)
    assert not engine.softmax_weights(s, 1.0, -np.inf, 40).any() and not weights(s, 1.0, F(-np.inf), 40).any()


def test_weights_of_rows_take_each_rows_shift():
    s = np.array([[0.0, 1.0, 2.0], [5.0, 4.0, -np.inf]], F)
    got = engine.softmax_weights(s, 1.0, np.array([2.0, 5.0], F), 40)
    assert got.shape == (2, 3) and np.array_equal(got, weights(s, 1.0, np.array([[2.0], [5.0]], F), 40))
    assert int(got[0, 2]) == 1 << 40 and int(got[1, 0]) == 1 << 40 and got[1, 2] == 0


def test_bad_arguments_are_refused():
    for t in (0.0, -1.0, np.nan, np.inf, 1e-39):
        with pytest.raises(engine.EngineError):
            engine.softmax_weights(np.zeros(3, F), t, 0.0, 40)
    with pytest.raises(engine.EngineError):
        engine.softmax_weights(np.zeros(3, F), 1.0, 0.0, 41)


def test_exp32_is_accurate_monotone_and_one_at_zero(sweep):
    d = sweep[sweep >= -64]
    e = exp32(d)
    assert e.dtype == F and exp32(F(0)) == F(1) and exp32(F(-0.0)) == F(1)
    rel = np.abs(e.astype(np.float64) - np.exp(d.astype(np.float64))) / np.exp(d.astype(np.float64))
    print("exp32 max relative error", rel.max(), "at", d[rel.argmax()], "over", d.size, "arguments")
    assert rel.max() <= EXP32_MAX_REL
    assert np.all(np.diff(e) >= 0) and e.max() == F(1) and e.min() > 0  # d ascends
    w = engine.softmax_weights(d, 1.0, 0.0, 40)
    assert np.all(np.diff(w.astype(np.int64)) >= 0)


def test_exp32_recorded_figures():
    """The figures the documents record, measured here: over 6 000 001 equally spaced and 4 000 000 logarithmically spaced arguments
    in [-64, 0] the max relative error against float64 is 2.54e-7 (2.536e-7, at d = -26.686005), exp32 never decreases along either
    sorted sweep, and its maximum is exactly 1."""
    worst = 0.0
    for d in (np.linspace(-64, 0, 6_000_001).astype(F), np.sort(-np.exp(np.random.RandomState(0).uniform(-30, np.log(64), 4_000_000))).astype(F)):
        e = exp32(d)
        ref = np.exp(d.astype(np.float64))
        rel = np.abs(e.astype(np.float64) - ref) / ref
        print("exp32 max relative error", rel.max(), "at", d[rel.argmax()], "over", d.size, "arguments")
        worst = max(worst, float(rel.max()))
        assert np.all(np.diff(e) >= 0) and e.max() == F(1) and e.min() > 0
    assert 2.53e-7 < worst <= EXP32_MAX_REL


def test_log_prob_of_an_empty_row_is_minus_infinity():
    """A row that may see nothing (shift -inf, mass 0): every weight is 0, log_prob is -inf (not NaN), slate_log_prob NaN, log_z -inf;
    the row beside it is not disturbed.  An empty last axis gives empty results."""
    part = engine.Partition(1.0, np.array([-np.inf, 0.0], F), np.array([0, 2 << 40], np.uint64), 40)
    s = np.array([[0.0, 1.0, -np.inf], [0.0, 0.0, -90.0]], F)
    lp = part.log_prob(s)
    assert np.all(np.isneginf(lp[0])) and np.isneginf(lp[1, 2]) and np.allclose(lp[1, :2], np.log(0.5), rtol=0, atol=1e-12)
    assert np.all(np.isnan(part.slate_log_prob(s)[0])) and np.isneginf(part.log_z[0]) and part.log_z[1] == np.log(2.0)
    assert part.log_prob(np.zeros((2, 0), F)).shape == (2, 0) and part.slate_log_prob(np.zeros((2, 0), F)).shape == (2, 0)
    assert engine.softmax_weights(np.zeros((3, 0), F), 1.0, np.zeros(3, F), 40).shape == (3, 0)


def test_frac_bits():
    want = {1: 40, 2 ** 23: 39, 2 ** 23 + 1: 39, 10 ** 7: 39, 2 ** 32 - 1: 31, 2 ** 23 - 1: 40, 10 ** 6: 40, 2 ** 31: 31}
    for n, fb in want.items():
        assert engine.softmax_frac_bits(n) == fb == frac_bits(n), n
        assert n << fb < 1 << 63  # num_items weights of at most 2^F each cannot overflow


def test_fix_truncates():
    x = np.array([1.0, 0.5, 0.75, 2.0 ** -40, 2.0 ** -41, 1.5 * 2.0 ** -40, 1 - 2.0 ** -24, 2.0 ** -100], F)
    assert fix(x, 40).tolist() == [1 << 40, 1 << 39, 3 << 38, 1, 0, 1, (1 << 40) - (1 << 16), 0]
    assert fix(x, 0).tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_slate_log_prob_on_hand_built_masses():
    """Weights 4 : 2 : 1 : 1 by scores that are exact multiples of ln 2 apart would need exp32 to be exact; instead the masses are
    built from the weights themselves, so the remaining mass is an exact integer that reaches 0 behind the last draw."""
    fb = 40
    s = np.array([[2.0, 1.0, 0.5, 0.0, -np.inf], [0.0, 0.0, 0.0, -90.0, 0.0]], F)
    shift = np.array([2.0, 0.0], F)
    w = weights(s, 1.0, shift[:, None], fb)
    assert w[0, 4] == 0 and w[1, 3] == 0
    mass = np.array([sum(int(x) for x in w[0]), sum(int(x) for x in w[1])], np.uint64)
    part = engine.Partition(1.0, shift, mass, fb)
    got = part.slate_log_prob(s)
    want = slate_log_prob_expect(s, 1.0, shift, mass, fb)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[0, 4]) and np.isnan(got[1, 3])
    assert np.nanmax(np.abs(got - want)) <= 1e-12
    assert got[0, 3] == 0.0 and got[1, 4] == 0.0  # the last draw takes all that is left: the remaining mass is exactly its weight
    rest = [int(mass[0]) - sum(int(x) for x in w[0, :j]) for j in range(4)]
    assert np.allclose(got[0, :4], [np.log(int(w[0, j]) / rest[j]) for j in range(4)], rtol=0, atol=1e-12)
    # a slate that overdraws its partition has no probability
    short = engine.Partition(1.0, shift[:1], np.array([int(w[0, 0])], np.uint64), fb)
    over = short.slate_log_prob(s[:1])
    assert over[0, 0] == 0.0 and np.all(np.isnan(over[0, 1:]))
    # log_prob: one draw each; -inf where w == 0
    lp = part.log_prob(s)
    assert np.isneginf(lp[0, 4]) and np.isneginf(lp[1, 3])
    assert np.allclose(lp[0, :4], np.log(w[0, :4].astype(np.float64) / float(mass[0])), rtol=0, atol=1e-12)


@pytest.mark.parametrize("temperature", [0.5, 1.0, 2.0])
def test_probabilities_agree_with_a_float64_softmax(temperature):
    """|w_i / mass - softmax_i| within the truncation bound num_items 2^-F plus the recorded exp32 error, both relative to a mass
    of at least 1; log_z likewise."""
    rs = np.random.RandomState(11)
    n = 5000
    s = (rs.randn(3, n) * 2).astype(F)
    fb = frac_bits(n)
    shift, mass = partition_expect(s, None, temperature)
    part = engine.Partition(temperature, shift, mass, fb)
    t = (s * inv_temperature(temperature)).astype(np.float64)
    z = np.exp(t - shift[:, None].astype(np.float64))
    bound = n * 2.0 ** -fb + EXP32_MAX_REL
    p = np.exp(part.log_prob(s))
    errs = (np.max(np.abs(p - z / z.sum(1, keepdims=True))), np.max(np.abs(mass.astype(np.float64) / 2.0 ** fb - z.sum(1)) / z.sum(1)),
            np.max(np.abs(part.log_z - (shift + np.log(z.sum(1))))))
    print("T", temperature, "bound", bound, "max |p - softmax|, relative mass error, |log_z error|:", errs)
    assert max(errs) <= bound
    assert np.array_equal(part.log_z, log_z_expect(shift, mass, fb))
    assert np.all(mass >= np.uint64(1 << fb))


def test_expectation_rows():
    tags = np.array([1, 2, 4, 1, 3, 0], np.uint32)
    s = np.array([[0.0, 3.0, 1.0, 2.0, -1.0, 0.5]], F)
    sh, m = partition_expect(s, [[1, 1, 3]], 1.0)  # repeats count once; the arg-max is excluded
    assert sh[0] == F(1.0) and int(m[0]) == sum(int(x) for x in weights(s[0, [0, 2, 4, 5]], 1.0, F(1.0), frac_bits(6)))
    sh, m = partition_expect(s, [[1]], 1.0, tags=tags, any_of=1, none_of=2)  # items 0 and 3 pass
    assert sh[0] == F(2.0) and int(m[0]) == sum(int(x) for x in weights(s[0, [0, 3]], 1.0, F(2.0), 40))
    sh, m = partition_expect(s, [range(6)], 1.0)
    assert np.isneginf(sh[0]) and m[0] == 0 and np.isneginf(log_z_expect(sh, m, 40)[0])
    sh, m = partition_expect(np.zeros((1, 7), F) - F(0.0), None, 3.0)
    assert sh.view(np.uint32)[0] == 0 and int(m[0]) == 7 << 40  # flat scores; a zero shift is +0.0


@pytest.mark.parametrize("temperature", [0.5, 2.0])
def test_first_pick_of_the_sampler_follows_the_weights(temperature):
    """Closure with recommend_sampled's noise: over 200 000 streams the first pick's frequencies on a 24-item catalogue against
    w / mass give a chi-square below the 0.001 point at 23 degrees of freedom."""
    rs = np.random.RandomState(2)
    s = (rs.randn(24) * 1.2).astype(F)
    streams = np.arange(200000, dtype=np.uint64)
    keys = keys_of(s[None, :], inv_temperature(temperature), noise(3, streams, np.arange(24, dtype=np.uint32)))
    counts = np.bincount(np.argmax(keys, axis=1), minlength=24).astype(np.float64)
    shift, mass = partition_expect(s[None, :], None, temperature)
    p = np.exp(engine.Partition(temperature, shift, mass, frac_bits(24)).log_prob(s[None, :]))[0]
    assert abs(p.sum() - 1.0) < 1e-9
    stat = float(np.sum((counts - streams.size * p) ** 2 / (streams.size * p)))
    print("T", temperature, "chi2", stat)
    assert stat < CHI2_23_0001
