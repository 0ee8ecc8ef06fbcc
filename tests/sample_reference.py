"""NumPy restatement of the policy's exploration noise (csrc/philox_device.h
philox_normal4 + gaussian_act; choose_action, ppo_continuous.py:184-188):
Philox4x32-10 keyed by (seed, agent) with counter (global env id, step),
Box-Muller, the clamp and the Normal log-density.  It shares nothing with the
product: the Philox rounds and the key schedule are reset_dist_reference's,
which test_reset_dist_cpu.py checks against the Random123 known-answer vectors.

Everything after the uniforms is f64, except the angle: the kernel's
t = 6.283185307179586f * u1 is one f32 product of a 24-bit constant and a
24-bit u1, so the exact product fits in 48 bits, f64 holds it, and one rounding
to f32 reproduces the kernel's angle bit for bit.  What is left between the
kernel's z and this one is the device library's logf / sqrtf / cosf / sinf and
two product roundings (Z_TOL below).
"""
import numpy as np

from reset_dist_reference import M32, philox4x32_10, philox_key

TWO_PI_F32 = float(np.float32(6.283185307179586))      # the kernel's constant as the compiler rounds it
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)

# per element: Z_TOL * max(1, r).  logf <= 3 ulp (halved by the square root),
# sqrtf <= 1 ulp, cosf / sinf <= 4 ulp, the -2 * log and r * cos products half
# an ulp each: |dz| <~ 8 * 2^-24 * r; the tolerance is twice that
Z_TOL = 16.0 * 2.0 ** -24

# env ids below 7e7 whose first Philox word at (seed 7, agent 0, step 3) has its
# top 24 bits all equal (test_sample_cpu.py asserts it): all zero -> u0 = 2^-24,
# the largest radius sqrt(2 ln 2^24) ~ 5.768; all one -> u0 = 1, r = 0, z0 = z1 = +-0
EDGE_IDS = [10768711, 14883186, 16419478, 24725485, 41329839, 51269297, 52283473]
R_MAX_IDS = [14883186, 16419478, 24725485, 41329839, 52283473]
R_ZERO_IDS = [10768711, 51269297]
R_MAX = float(np.sqrt(2.0 * np.log(2.0 ** 24)))


def _u64(x, shape=None):
    if isinstance(x, np.ndarray) and x.dtype.kind in "iu":
        a = x.astype(np.uint64)
    else:                                                  # python ints up to 2^64 - 1
        a = np.asarray(x, dtype=object)
        a = np.array([int(v) & (2 ** 64 - 1) for v in np.ravel(a)], dtype=np.uint64).reshape(a.shape)
    return a if shape is None else np.broadcast_to(a, shape)


def words(seed, agent, gid, step):
    """The four Philox output words uint32 [n, 4] of global env ids `gid`
    ([n] ints below 2^64) at `step` (an int or [n] ints below 2^64)."""
    gid = np.atleast_1d(_u64(gid))
    step = _u64(step, gid.shape)
    m, s = np.uint64(M32), np.uint64(32)
    ctr = np.stack([gid & m, gid >> s, step & m, step >> s], axis=-1)
    k0, k1 = philox_key(seed, agent)
    return philox4x32_10(ctr, k0, k1)


def normals(seed, agent, gid, step):
    """z f64 [n, 4] of philox_normal4 and the two Box-Muller radii f64 [n] x 2
    (z[:, 0:2] have radius r0, z[:, 2:4] radius r1)."""
    w = (words(seed, agent, gid, step) >> np.uint32(8)).astype(np.float64)   # the top 24 bits of each word
    z = np.empty(w.shape, dtype=np.float64)
    radii = []
    for p in range(2):
        u0 = (w[:, 2 * p] + 1.0) / 16777216.0                            # (0, 1]
        u1 = w[:, 2 * p + 1] / 16777216.0                                # [0, 1)
        r = np.sqrt(-2.0 * np.log(u0))
        t = (TWO_PI_F32 * u1).astype(np.float32).astype(np.float64)      # exact product, rounded once: the f32 angle
        z[:, 2 * p] = r * np.cos(t)
        z[:, 2 * p + 1] = r * np.sin(t)
        radii.append(r)
    return z, radii[0], radii[1]


def radius3(r0, r1):
    """The radius behind each of the three action components: [n, 3]."""
    return np.stack([r0, r0, r1], axis=-1)


def z_tol(r0, r1):
    """The tolerance of the kernel's z[:, :3] against normals(): [n, 3]."""
    return Z_TOL * np.maximum(1.0, radius3(r0, r1))


def logp_of(a, mean, log_std):
    """Normal(mean, exp(log_std)).log_prob(a) in f64."""
    a, mean, log_std = (np.asarray(v, dtype=np.float64) for v in (a, mean, log_std))
    return -((a - mean) ** 2) / (2.0 * np.exp(2.0 * log_std)) - log_std - LOG_SQRT_2PI


def logp_tol(a, mean, log_std):
    """2^-20 * (q + |log_std| + 1), q = (a - mean)^2 / 2 sigma^2: a few f32
    roundings of the largest term of the sum."""
    a, mean, log_std = (np.asarray(v, dtype=np.float64) for v in (a, mean, log_std))
    q = (a - mean) ** 2 / (2.0 * np.exp(2.0 * log_std))
    return 2.0 ** -20 * (q + np.abs(log_std) + 1.0)


def act_logp(mean, log_std, z, max_action):
    """gaussian_act in f64 from f32 inputs: the action clamp(mean + exp(log_std) * z,
    +-max_action) and its log-density.  (Tests evaluate logp_of at the action
    the kernel returned, so their log-prob check needs no agreement on z.)"""
    mean = np.asarray(mean, dtype=np.float32).astype(np.float64)
    log_std = np.asarray(log_std, dtype=np.float32).astype(np.float64)
    m = float(np.float32(max_action))
    a = np.clip(mean + np.exp(log_std) * np.asarray(z, dtype=np.float64), -m, m)
    return a, logp_of(a, mean, log_std)
