"""NumPy restatement of the env's randomised reset (include/satenv.h
satenv_reset_dist): Philox4x32-10, the engine's key schedule
and the affine map.  It is the reference of the bitwise checks in
test_reset_dist_cpu.py / test_reset_dist_gpu.py; test_reset_dist_cpu.py
checks it against the Random123 known-answer vectors.
"""
import numpy as np

M32 = 0xFFFFFFFF
RESET_STREAM = 2
# the reference's reset (environment.py:67-71): Pp Pv Ep Ev
CENTRE = np.array([200000.0, 0, 0, 0, 0, 0, 18000.0, 0, 0, 0, 0, 0])
# the issue's box: +-50 km on the positions, +-5 m/s on the velocities
HALF = np.array([50000.0] * 3 + [5.0] * 3 + [50000.0] * 3 + [5.0] * 3)
LO, HI = CENTRE - HALF, CENTRE + HALF


def philox4x32_10(ctr, k0, k1):
    """ctr: uint32 [..., 4]; k0, k1: python ints.  Returns uint32 [..., 4]."""
    c = [np.asarray(ctr[..., m], dtype=np.uint64) for m in range(4)]
    k0, k1 = int(k0) & M32, int(k1) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)
        c = [n0, p1 & np.uint64(M32), n2, p0 & np.uint64(M32)]
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_key(seed, stream):
    seed = int(seed) & (2 ** 64 - 1)
    k0 = (seed & M32) ^ ((stream * 0x85EBCA6B) & M32)
    k1 = (seed >> 32) ^ ((stream * 0xC2B2AE35 + 0x27D4EB2F) & M32)
    return k0, k1


def expected_draw(lo, hi, seed, gid, ep):
    """The 12 kinematic scalars [12, n] of the resets of global env ids `gid`
    (int array [n]) at episode indices `ep` (int or int array [n])."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    gid = np.asarray(gid, dtype=np.int64).astype(np.uint64)
    ep = np.broadcast_to(np.asarray(ep, dtype=np.int64), gid.shape).astype(np.uint64)
    k0, k1 = philox_key(seed, RESET_STREAM)
    words = []
    for j in range(3):
        ctr = np.stack([gid & np.uint64(M32), gid >> np.uint64(32), ep & np.uint64(M32),
                        np.full(gid.shape, j, dtype=np.uint64)], axis=-1)
        words.append(philox4x32_10(ctr, k0, k1))
    w = np.concatenate(words, axis=-1).T                     # [12, n] uint32
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    span = hi - lo
    return lo[:, None] + span[:, None] * u


def obs_of(k):
    """The f64 observation rows [n, 18] of kinematics k [12, n]: [Pp-Ep, Pv-Ev, Pp, Pv, Ep, Ev]."""
    Pp, Pv, Ep, Ev = k[0:3], k[3:6], k[6:9], k[9:12]
    return np.concatenate([Pp - Ep, Pv - Ev, Pp, Pv, Ep, Ev], axis=0).T.copy()


def fixed_actions(n, seed=7):
    """f32 [n, 3] x 2 inside the action box; no zero component."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.2, 1.6, size=(2, n, 3)) * rng.choice([-1.0, 1.0], size=(2, n, 3))
    return a[0].astype(np.float32), a[1].astype(np.float32)
