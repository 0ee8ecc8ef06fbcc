"""Host side of the running observation normalisation and reward scaling
(satrl.norm): the moment merge against long-double and Welford references,
the device statistics, the state round trip, the C entry points' argument
refusals (no device call), and slot_total's sharding invariance over gloo."""
import ctypes as C
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG_DIR

# raw-scale observation features: positions near 2e6 m, velocities near 1e3 m/s
MEANS = np.array([2e6, 2e6, 1e6, 1710.0, 1140.0, 1300.0])
SPREADS = np.array([1e4, 5e4, 1e3, 1.0, 0.5, 2.0])
ROWS = (1000, 777, 2048)             # rows per batch (the first two leave a part-filled slot)


def _batches(seed):
    """Three f32 batches drifting by three spreads per batch."""
    rng = np.random.default_rng(seed)
    return [(MEANS + 3.0 * b * SPREADS + SPREADS * rng.standard_normal((n, 6))).astype(np.float32)
            for b, n in enumerate(ROWS)]


def _slot_sums(x, pivot32):
    """What the kernel hands over: f64 sums of d and d*d per 32-row slot, then the slots' total."""
    d = x.astype(np.float64) - pivot32.astype(np.float64)
    s = np.zeros((2, x.shape[1]))
    for k in range(0, x.shape[0], 32):
        s[0] += d[k:k + 32].sum(0)
        s[1] += (d[k:k + 32] * d[k:k + 32]).sum(0)
    return s


def _merged(batches):
    from satrl.norm import RunningMoments
    rm = RunningMoments((6,))
    pivot = MEANS.astype(np.float32)                         # the reset row
    for x in batches:
        s = _slot_sums(x, pivot)
        rm.merge_shifted(x.shape[0], s[0], s[1], pivot)
        pivot = rm.mean.astype(np.float32)                   # the previous mean, as the device holds it
    return rm


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_merge_matches_long_double_moments(seed):
    batches = _batches(seed)
    rm = _merged(batches)
    x = np.concatenate(batches).astype(np.longdouble)
    ref_mean = x.mean(0)
    ref_std = np.sqrt(((x - ref_mean) ** 2).mean(0))
    xmax = np.abs(x).max(0)
    err_m = np.abs(rm.mean.astype(np.longdouble) - ref_mean)
    err_s = np.abs(rm.std().astype(np.longdouble) - ref_std)
    print("mean err / max|x|:", (err_m / xmax).max(), " std rel err:", (err_s / ref_std).max())
    assert rm.n == sum(ROWS)
    assert (err_m <= 1e-13 * xmax).all()
    assert (err_s <= 1e-10 * ref_std).all()


def test_merge_agrees_with_a_welford_loop():
    batches = _batches(7)
    rm = _merged(batches)
    n, mean, M2 = 0, np.zeros(6), np.zeros(6)
    for x in np.concatenate(batches).astype(np.float64):
        n += 1
        d = x - mean
        mean = mean + d / n
        M2 = M2 + d * (x - mean)
    std = np.sqrt(M2 / n)
    xmax = np.abs(np.concatenate(batches)).max(0).astype(np.float64)
    assert (np.abs(rm.mean - mean) <= 1e-13 * xmax).all()
    assert (np.abs(rm.std() - std) <= 1e-10 * std).all()


def test_device_stats_reproduce_the_reference_constant():
    from satrl.norm import RunningMoments
    rm = RunningMoments((6,))
    assert np.array_equal(rm.device_stats(), np.stack([np.zeros(6, np.float32), np.ones(6, np.float32)]))
    x = _batches(3)[0].copy()
    x[:, 4] = np.float32(1140.0)                             # a zero-variance feature
    piv = x[0]
    s = _slot_sums(x, piv)
    rm.merge_shifted(x.shape[0], s[0], s[1], piv)
    st = rm.device_stats()
    assert st.dtype == np.float32 and st.shape == (2, 6)
    for f in range(6):
        assert st[0, f] == np.float32(rm.mean[f])
        assert st[1, f] == np.float32(1.0 / (rm.std()[f] + 1e-8))
    assert rm.std()[4] == 0.0 and np.isfinite(st[1, 4]) and st[1, 4] == np.float32(1e8)
    # the scalar form the return moments use
    r = RunningMoments(())
    r.merge_shifted(4, 10.0, 30.0, 0.0)                      # 1, 2, 3, 4
    assert float(r.mean) == 2.5 and float(r.std()) == pytest.approx(np.std([1.0, 2.0, 3.0, 4.0]), rel=1e-15)


def test_state_dict_round_trip_is_exact():
    from satrl.norm import RunningMoments
    rm = _merged(_batches(5))
    sd = rm.state_dict()
    assert all(isinstance(v, np.ndarray) for v in sd.values())
    rm2 = RunningMoments((6,)).load_state_dict({k: v.copy() for k, v in sd.items()})
    assert rm2.n == rm.n and np.array_equal(rm2.mean, rm.mean) and np.array_equal(rm2.M2, rm.M2)
    assert np.array_equal(rm2.device_stats(), rm.device_stats())
    with pytest.raises(ValueError):
        RunningMoments((18,)).load_state_dict(sd)


def test_norm_entry_points_refuse_bad_arguments_before_any_device_call():
    """include/satrl_rollout.h: -1 and a satrl_last_error text naming the
    argument; the checks run on the host before any HIP call, and the non-null
    dummy pointer is never dereferenced on these paths."""
    import satrl._lib as L
    lib = L.lib()
    fake, fake2 = C.c_void_p(16), C.c_void_p(32)

    def refused(fn, args, word):
        assert fn(*args) == -1
        msg = lib.satrl_last_error()
        assert fn.__name__.encode() in msg and word in msg, msg

    on = lib.satrl_obs_normalize
    refused(on, (4, None, fake, 10.0, fake2, None, None, None), b"raw")
    refused(on, (4, fake, None, 10.0, fake2, None, None, None), b"stats")
    refused(on, (4, fake, fake, 10.0, None, None, None, None), b"out")
    refused(on, (0, fake, fake, 10.0, fake2, None, None, None), b"N must")
    refused(on, (-3, fake, fake, 10.0, fake2, None, None, None), b"N must")
    refused(on, (4, fake, fake, 10.0, fake2, None, fake, None), b"pivot")
    refused(on, (4, fake, fake, 10.0, fake, None, None, None), b"out")          # out is raw
    rs = lib.satrl_return_scan
    refused(rs, (0, 4, fake, fake, 0.99, fake, fake, None), b"T must")
    refused(rs, (4, 0, fake, fake, 0.99, fake, fake, None), b"N must")
    refused(rs, (4, 4, None, fake, 0.99, fake, fake, None), b"r is")
    refused(rs, (4, 4, fake, None, 0.99, fake, fake, None), b"done")
    refused(rs, (4, 4, fake, fake, 0.99, None, fake, None), b"carry")
    refused(rs, (4, 4, fake, fake, 0.99, fake, None, None), b"acc")


def test_new_keywords_default_off():
    from satrl.trainer import args_param
    a = args_param()
    assert a.obs_norm is False and a.reward_scaling is False
    assert a.obs_clip == 10.0 and a.obs_norm_calib_steps == 64
    # the reference's own (dead) keywords keep their defaults
    assert a.use_state_norm is True and a.use_reward_norm is False and a.use_reward_scaling is True


# -- slot_total over gloo -------------------------------------------------------------
def _slots(seed=11):
    return np.random.default_rng(seed).normal(0.0, 1e6, (8, 2, 18))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    sys.path.insert(0, PKG_DIR)
    from satrl.norm import slot_total
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        first, k = ((0, 3), (3, 5))[rank]
        acc = torch.from_numpy(_slots()[first:first + k].copy())
        q.put((rank, slot_total(acc, dist.group.WORLD, first, 8)))
    finally:
        dist.destroy_process_group()


def test_slot_total_world2_gloo_has_the_one_process_bits():
    from satrl.norm import slot_total
    one = slot_total(torch.from_numpy(_slots()), None, 0, 8)
    assert one.dtype == np.float64 and one.shape == (2, 18)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(2):
        assert np.array_equal(res[r], one), r
    with pytest.raises(ValueError):
        slot_total(torch.zeros((3, 2)), None, 6, 8)
