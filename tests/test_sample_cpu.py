"""The exploration-noise restatement (sample_reference.py) checked on its own,
before test_sample_gpu.py holds the kernels to it: the moments of its draws,
and the env ids at which the Box-Muller radius takes its two extremes.

Every statistical bound is 5 sigma of the statistic's own sampling error under
the null hypothesis (independent standard normals) at n = 2^20.
"""
import numpy as np
import pytest

import sample_reference as SR

SEED, AGENT, STEP = 7, 0, 3
N = 1 << 20

EDGE_IDS, R_MAX_IDS, R_ZERO_IDS, R_MAX = SR.EDGE_IDS, SR.R_MAX_IDS, SR.R_ZERO_IDS, SR.R_MAX


@pytest.fixture(scope="module")
def draws():
    gid = np.arange(N, dtype=np.int64)
    z, _, _ = SR.normals(SEED, AGENT, gid, STEP)
    z_next, _, _ = SR.normals(SEED, AGENT, gid, STEP + 1)
    return z[:, :3], z_next[:, :3]


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


def test_moments(draws):
    z, _ = draws
    for d in range(3):
        x = z[:, d]
        mean, var = float(x.mean()), float(x.var())
        kurt = float(((x - mean) ** 4).mean() / var ** 2)
        print(f"z[{d}]: mean {mean:+.2e} var-1 {var - 1:+.2e} kurtosis-3 {kurt - 3:+.2e}")
        assert abs(mean) < 5.0 / np.sqrt(N)
        assert abs(var - 1.0) < 5.0 * np.sqrt(2.0 / N)
        assert abs(kurt - 3.0) < 5.0 * np.sqrt(96.0 / N)


def test_correlations(draws):
    z, z_next = draws
    bound = 5.0 / np.sqrt(N)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        c = _corr(z[:, i], z[:, j])
        print(f"corr(z[{i}], z[{j}]) = {c:+.2e}")
        assert abs(c) < bound
    for d in range(3):
        c_env = _corr(z[:-1, d], z[1:, d])                 # consecutive env ids
        c_step = _corr(z[:, d], z_next[:, d])              # consecutive steps
        print(f"z[{d}]: corr over consecutive env ids {c_env:+.2e}, over consecutive steps {c_step:+.2e}")
        assert abs(c_env) < 5.0 / np.sqrt(N - 1)
        assert abs(c_step) < bound


def test_tail_fraction(draws):
    z, _ = draws
    p = 2.6998e-3                                          # P(|z| > 3)
    for d in range(3):
        frac = float((np.abs(z[:, d]) > 3.0).mean())
        print(f"z[{d}]: fraction beyond 3 sigma {frac:.4e}")
        assert abs(frac - p) < 5.0 * np.sqrt(p * (1.0 - p) / N)


def test_edge_ids_reach_both_ends_of_the_radius():
    assert sorted(R_MAX_IDS + R_ZERO_IDS) == EDGE_IDS
    top = SR.words(SEED, AGENT, np.array(EDGE_IDS), STEP)[:, 0] >> np.uint32(8)
    z, r0, _ = SR.normals(SEED, AGENT, np.array(EDGE_IDS), STEP)
    for k, gid in enumerate(EDGE_IDS):
        if gid in R_MAX_IDS:
            assert int(top[k]) == 0, gid
            assert r0[k] == R_MAX, gid
            assert np.isclose(np.hypot(z[k, 0], z[k, 1]), R_MAX, rtol=1e-15), gid
        else:
            assert int(top[k]) == 0xFFFFFF, gid
            assert r0[k] == 0.0 and z[k, 0] == 0.0 and z[k, 1] == 0.0, gid
    assert 5.76 < R_MAX < 5.77


def test_counter_uses_all_four_words():
    """The high halves of the env id and of the step are counter words of
    their own: dropping one, or adding it into the low half, changes the draw."""
    g, s = 5, 3
    base = SR.words(SEED, AGENT, [g], s)
    assert not np.array_equal(base, SR.words(SEED, AGENT, [g + (1 << 32)], s))
    assert not np.array_equal(base, SR.words(SEED, AGENT, [g], s + (1 << 32)))
    assert not np.array_equal(SR.words(SEED, AGENT, [g + (1 << 32)], s), SR.words(SEED, AGENT, [g], s + (1 << 32)))
    assert not np.array_equal(base, SR.words(SEED, 1, [g], s))
    assert not np.array_equal(base, SR.words(SEED + (1 << 32), AGENT, [g], s))
    # the counter of (2^32 - 1) + 2 carries into the step's high word
    assert np.array_equal(SR.words(SEED, AGENT, [g], (1 << 32) + 1), SR.words(SEED, AGENT, [g], (1 << 32) - 1 + 2))


def test_angle_is_the_f32_product():
    """6.283185307179586f has 24 significant bits and u1 at most 24: their
    product is exact in f64, so rounding it once gives the f32 product."""
    c = np.float32(6.283185307179586)
    m = int(float(c) * 2 ** 21)
    assert float(c) == m / 2 ** 21 and m < 2 ** 24
    rng = np.random.default_rng(0)
    k = np.concatenate([rng.integers(0, 1 << 24, 4096), [0, 1, (1 << 24) - 1]])
    exact = [int(m) * int(v) for v in k]                   # in units of 2^-45
    f64 = SR.TWO_PI_F32 * (k / 16777216.0)
    assert all(float(a) * 2.0 ** 45 == e for a, e in zip(f64, exact))
    assert np.array_equal(f64.astype(np.float32), c * (k / 16777216.0).astype(np.float32))


def test_act_logp_against_closed_forms():
    mean = np.float32([[0.3, -2.0, 1.6]])
    log_std = np.float32([-0.5, 0.0, 2.0])
    z = np.array([[1.0, 0.25, -0.25]])
    a, lp = SR.act_logp(mean, log_std, z, 1.6)
    want = np.clip(mean.astype(np.float64) + np.exp(log_std.astype(np.float64)) * z, -float(np.float32(1.6)),
                   float(np.float32(1.6)))
    assert np.array_equal(a, want)
    assert a[0, 1] == -float(np.float32(1.6))              # -2 + 0.25 is outside the box
    sd = np.exp(log_std.astype(np.float64))
    dens = np.exp(-0.5 * ((a - mean) / sd) ** 2) / (sd * np.sqrt(2.0 * np.pi))
    assert np.allclose(lp, np.log(dens), rtol=0, atol=1e-13)
    assert np.array_equal(lp, SR.logp_of(a, mean, log_std))
