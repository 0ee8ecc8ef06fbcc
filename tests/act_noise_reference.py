"""NumPy restatement of the env's actuation noise (include/satenv.h
satenv_act_noise): one Philox4x32-10 block per (agent, global
env id, episode index, step count), four bounded uniforms, a magnitude error
along the commanded action and a pointing error that scales with it.  It is
the reference of the bitwise checks in test_act_noise_cpu.py /
test_act_noise_gpu.py.  The Philox rounds and the key schedule are
reset_dist_reference's (checked there against the Random123 vectors); nothing
here is shared with the product.
"""
import numpy as np

from reset_dist_reference import M32, philox4x32_10, philox_key

NOISE_STREAM = 3                 # + agent (0 pursuer, 1 evader); 0 / 1 sample the policies, 2 draws the resets
A_MAX = np.float32(1.6)


def clip16(a):
    a = np.asarray(a, dtype=np.float32)
    return np.where(a < -A_MAX, -A_MAX, np.where(a > A_MAX, A_MAX, a)).astype(np.float32)


def uniforms(seed, agent, gid, ep, cnt):
    """z f64 [n, 4] in (-1, 1) of global env ids `gid` (int array [n]) at episode
    indices `ep` and step counts `cnt` (ints or int arrays [n])."""
    gid = np.asarray(gid, dtype=np.int64).astype(np.uint64)
    ep = np.broadcast_to(np.asarray(ep, dtype=np.int64), gid.shape).astype(np.uint64)
    cnt = np.broadcast_to(np.asarray(cnt, dtype=np.int64), gid.shape).astype(np.uint64)
    m = np.uint64(M32)
    ctr = np.stack([gid & m, gid >> np.uint64(32), ep & m, cnt & m], axis=-1)
    w = philox4x32_10(ctr, *philox_key(seed, NOISE_STREAM + int(agent)))
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    return 2.0 * u - 1.0


def executed(mag, dire, seed, agent, gid, ep, cnt, a):
    """The executed actions f32 [n, 3] for the commanded, already clipped
    actions `a` f32 [n, 3] of agent `agent` with half-widths (mag, dire)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    mag, dire = float(mag), float(dire)
    if mag == 0.0 and dire == 0.0:
        return a.copy()
    z = uniforms(seed, agent, gid, ep, cnt)
    a64 = a.astype(np.float64)
    s = 1.0 + mag * z[:, 0]
    # the squares of widened f32 are exact in f64, so the kernel's fma chain rounds where these sums do
    norm = np.sqrt((a64[:, 0] * a64[:, 0] + a64[:, 1] * a64[:, 1]) + a64[:, 2] * a64[:, 2])
    r = dire * norm
    out = s[:, None] * a64 + r[:, None] * z[:, 1:4]
    return clip16(out.astype(np.float32))


def executed_pair(noise, seed, gid, ep, cnt, pa, ea):
    """(pa', ea') under noise = ((mag, dir) of the pursuer, (mag, dir) of the
    evader), from raw (unclipped) action tensors as the step takes them."""
    return tuple(executed(noise[g][0], noise[g][1], seed, g, gid, ep, cnt, clip16(x)) for g, x in enumerate((pa, ea)))


def actions(n, seed=7):
    """f32 [n, 3] x 2: mostly generic rows inside the action box, plus the
    edge rows -- a zero action, one zero component, +-1.6 on every component
    and a row beyond the box (the step clips it first)."""
    rng = np.random.default_rng(seed)
    a = (rng.uniform(0.2, 1.6, size=(2, n, 3)) * rng.choice([-1.0, 1.0], size=(2, n, 3))).astype(np.float32)
    for g in range(2):
        a[g, 3 + g] = 0.0
        a[g, 10 + g, 1] = 0.0
        a[g, 20 + g] = [1.6, -1.6, 1.6]
        a[g, 30 + g] = [2.5, -0.3, -7.0]
    return a[0], a[1]
