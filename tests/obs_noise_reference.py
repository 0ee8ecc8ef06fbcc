"""NumPy restatement of the env's observation noise (include/satenv.h
satenv_obs_noise): per tracked craft a bias held for an
episode and an error redrawn every `hold` steps, bounded uniforms of six
Philox4x32-10 blocks per (global env id, episode index, step count), added to
the true kinematics before the f32 observation row is formed.  It is the
reference of the bitwise checks in test_obs_noise_cpu.py /
test_obs_noise_gpu.py.  The Philox rounds and the key schedule are
reset_dist_reference's (checked there against the Random123 vectors); nothing
here is shared with the product.
"""
import numpy as np

from reset_dist_reference import M32, philox4x32_10, philox_key

BIAS_STREAM = 5                  # 0 / 1 sample the policies, 2 draws the resets, 3 / 4 the actuation noise
NOISE_STREAM = 6                 # + block j = 0, 1, 2
EXACT = (0.0, 0.0, 0.0, 0.0)     # a craft's (bias_pos, bias_vel, pos, vel)


def _z(seed, stream, gid, ep, last):
    """z f64 [n, 4] in (-1, 1): the block with counter (gid, ep, last), key (seed, stream)."""
    m = np.uint64(M32)
    ctr = np.stack([gid & m, gid >> np.uint64(32), ep & m, last & m], axis=-1)
    w = philox4x32_10(ctr, *philox_key(seed, stream))
    return 2.0 * ((w.astype(np.float64) + 0.5) * 2.0 ** -32) - 1.0


def errors(seed, gid, ep, cnt, hold):
    """(zb, zw) f64 [n, 12] each: the bias and the refreshed uniforms of scalars
    0..11 for global env ids `gid` (int array [n]) at episode indices `ep` and
    step counts `cnt` (ints or int arrays [n])."""
    gid = np.asarray(gid, dtype=np.int64).astype(np.uint64)
    ep = np.broadcast_to(np.asarray(ep, dtype=np.int64), gid.shape).astype(np.uint64)
    cnt = np.broadcast_to(np.asarray(cnt, dtype=np.int64), gid.shape)
    win = (cnt // int(hold)).astype(np.uint64)
    zb = np.concatenate([_z(seed, BIAS_STREAM, gid, ep, np.full(gid.shape, j, dtype=np.uint64)) for j in range(3)],
                        axis=1)
    zw = np.concatenate([_z(seed, NOISE_STREAM + j, gid, ep, win) for j in range(3)], axis=1)
    return zb, zw


def widths(craft):
    """(B, W) f64 [12] of craft = ((bias_pos, bias_vel, pos, vel) of the pursuer, ... of the evader)."""
    B, W = np.zeros(12), np.zeros(12)
    for s in range(12):
        bp, bv, p, v = craft[s // 6]
        B[s], W[s] = (bv, v) if s % 6 >= 3 else (bp, p)
    return B, W


def measured(craft, hold, seed, gid, ep, cnt, k):
    """The measured kinematics f64 [n, 12] of the true ones k f64 [n, 12]."""
    k = np.ascontiguousarray(k, dtype=np.float64)
    B, W = widths(craft)
    zb, zw = errors(seed, gid, ep, cnt, hold)
    m = k.copy()
    for s in range(12):
        if B[s] != 0.0 and W[s] != 0.0:
            m[:, s] = k[:, s] + (B[s] * zb[:, s] + W[s] * zw[:, s])
        elif B[s] != 0.0:
            m[:, s] = k[:, s] + B[s] * zb[:, s]
        elif W[s] != 0.0:
            m[:, s] = k[:, s] + W[s] * zw[:, s]
    return m


def row_of(m):
    """The f32 observation rows [n, 18] of kinematics m [n, 12]: [Pp-Ep, Pv-Ev, Pp, Pv, Ep, Ev],
    the differences in f64, then the cast."""
    return np.concatenate([m[:, 0:6] - m[:, 6:12], m], axis=1).astype(np.float32)


def measured_rows(craft, hold, seed, gid, ep, cnt, obs64):
    """The f32 rows the env writes for the true f64 rows obs64 [n, 18] (their columns 6..17 are k)."""
    return row_of(measured(craft, hold, seed, gid, ep, cnt, np.asarray(obs64)[:, 6:18]))


def craft_of(spec_craft):
    """(bias_pos, bias_vel, pos, vel) of a dict with keys among those names."""
    return tuple(float(spec_craft.get(k, 0.0)) for k in ("bias_pos", "bias_vel", "pos", "vel"))
