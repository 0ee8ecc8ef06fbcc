"""Randomised episode starts on the host build (include/satenv.h
satenv_reset_dist): the NumPy restatement against Random123's vectors, then
the host build against the restatement bit for bit.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import reset_dist_reference as R

N = 130            # two 64-env workgroups + 2 lanes on the device; the same N here
SEED = 0x1234ABCD5678EF01
OFFSET = 1000


def _env(n=N, **kw):
    from satrl.env import VecSatellites
    kw.setdefault("d_capture", 1000.0)       # no start of the box is inside it: every episode times out
    kw.setdefault("max_episode_steps", 3)
    return VecSatellites(n, device="cpu", threads=2, **kw)


def _kin(env):
    return env.get_state()[0][:12].numpy().copy()


def _vel_int(env):
    return (env.get_state()[1][2].numpy() >> 4) & 1


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_numpy_philox_reproduces_random123_vectors():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32_10(np.array(ctr, dtype=np.uint32), *key)
        assert tuple(int(x) for x in got) == want
    # vectorised over a leading axis, the same words
    ctrs = np.array([k[0] for k in kat[:1] * 3], dtype=np.uint32)
    assert (R.philox4x32_10(ctrs, 0, 0) == np.array(kat[0][2], dtype=np.uint32)).all()


def test_reset_and_autoreset_draws_equal_restatement_bitwise():
    env = _env()
    env.set_reset_dist(R.LO, R.HI, SEED, env_offset=OFFSET)
    d = env.reset_dist
    assert _bits_equal(d["lo"], R.LO) and _bits_equal(d["hi"], R.HI)
    assert d["seed"] == SEED and d["env_offset"] == OFFSET
    assert (env.episode_index().numpy() == 0).all()
    gid = OFFSET + np.arange(N)
    obs = env.reset(0)
    want = R.expected_draw(R.LO, R.HI, SEED, gid, 0)
    assert _bits_equal(_kin(env), want)
    assert _bits_equal(obs.numpy(), R.obs_of(want).astype(np.float32))
    assert (_vel_int(env) == 0).all()
    assert (env.episode_index().numpy() == 1).all()
    assert len({want[:, i].tobytes() for i in range(N)}) == N
    pa, ea = (torch.from_numpy(a) for a in R.fixed_actions(N))
    for step in range(1, 8):
        obs, rew, done = env.step_autoreset(pa, ea)
        assert (done.numpy() == (1 if step % 3 == 0 else 0)).all(), step
        if step % 3 == 0:                     # the autoreset of episode step // 3
            want = R.expected_draw(R.LO, R.HI, SEED, gid, step // 3)
            assert _bits_equal(_kin(env), want), step
            assert _bits_equal(obs.numpy(), R.obs_of(want).astype(np.float32)), step
            assert (_vel_int(env) == 0).all()
    assert (env.episode_index().numpy() == 3).all()
    assert env.check_errors() == 0


def test_masked_reset_redraws_only_masked_envs():
    env = _env()
    env.set_reset_dist(R.LO, R.HI, SEED, env_offset=OFFSET)
    env.reset(0)
    before = _kin(env)
    mask = torch.zeros(N, dtype=torch.uint8)
    sel = np.array([0, 5, 63, 64, 129])
    mask[torch.from_numpy(sel)] = 1
    env.reset(0, mask=mask)
    after, ep = _kin(env), env.episode_index().numpy()
    want = before.copy()
    want[:, sel] = R.expected_draw(R.LO, R.HI, SEED, OFFSET + sel, 1)
    assert _bits_equal(after, want)
    assert (ep[sel] == 2).all() and (np.delete(ep, sel) == 1).all()


def test_cleared_distribution_is_the_fixed_reset_bitwise():
    a, b = _env(), _env()
    a.set_reset_dist(R.LO, R.HI, SEED, env_offset=OFFSET)
    assert a.reset_dist is not None
    a.clear_reset_dist()
    assert a.reset_dist is None and b.reset_dist is None
    pa, ea = (torch.from_numpy(x) for x in R.fixed_actions(N))
    oa, ob = a.reset(0), b.reset(0)
    assert _bits_equal(oa.numpy(), ob.numpy())
    assert _bits_equal(_kin(a), np.repeat(R.CENTRE[:, None], N, axis=1))
    assert (_vel_int(a) == 1).all()
    for step in range(1, 8):
        ra, rb = a.step_autoreset(pa, ea), b.step_autoreset(pa, ea)
        for x, y in zip(ra, rb):
            assert _bits_equal(x.numpy(), y.numpy()), step
        for x, y in zip(a.get_state(), b.get_state()):
            assert _bits_equal(x.numpy(), y.numpy()), step
        if step % 3 == 0:
            assert (ra[2].numpy() == 1).all() and (_vel_int(a) == 1).all()
    # the index counts the fixed resets too
    assert (a.episode_index().numpy() == 3).all() and (b.episode_index().numpy() == 3).all()


def test_degenerate_box_gives_exactly_lo():
    env = _env(n=7)
    lo = R.LO + np.arange(12) * 0.3
    env.set_reset_dist(lo, lo, SEED)
    env.reset(0)
    assert _bits_equal(_kin(env), np.repeat(lo[:, None], 7, axis=1))


def test_episode_index_set_and_zero():
    env = _env(n=5)
    t = torch.tensor([4, 0, 7, 1, 2], dtype=torch.int32)
    env.set_episode_index(t)
    assert (env.episode_index() == t).all()
    env.set_reset_dist(R.LO, R.HI, SEED)
    env.reset(0)
    assert _bits_equal(_kin(env), R.expected_draw(R.LO, R.HI, SEED, np.arange(5), t.numpy()))
    assert (env.episode_index() == t + 1).all()
    env.set_episode_index(None)
    assert (env.episode_index() == 0).all()
    # not part of the public state
    assert env.get_state()[1].shape[0] == 3


def test_bad_arguments_are_refused():
    import satrl._lib as L
    lib = L.lib()
    env = _env(n=3)
    good = L.SatenvResetDist()
    assert lib.satenv_default_reset_dist(C.byref(good)) == 0
    assert list(good.lo) == list(R.CENTRE) and list(good.hi) == list(R.CENTRE) and good.enabled == 0
    cpu_default = L.SatenvResetDist()
    assert lib.satenv_cpu_default_reset_dist(C.byref(cpu_default)) == 0
    assert bytes(cpu_default) == bytes(good)
    dummy = C.create_string_buffer(4096)          # a non-null handle: refused before it is looked at
    dev_h = C.cast(dummy, C.c_void_p)

    def variants():
        d = L.SatenvResetDist.from_buffer_copy(bytes(good))
        d.lo[4] = 1.0                             # lo > hi
        yield d
        for bad in (float("nan"), float("inf"), float("-inf")):
            for field in ("lo", "hi"):
                d = L.SatenvResetDist.from_buffer_copy(bytes(good))
                getattr(d, field)[7] = bad
                yield d
        d = L.SatenvResetDist.from_buffer_copy(bytes(good))
        d.lo[0], d.hi[0] = -1.7e308, 1.7e308      # finite bounds, infinite span
        yield d

    for d in variants():
        assert lib.satenv_cpu_set_reset_dist(env._h, C.byref(d), None) == -1
        assert lib.satenv_set_reset_dist(dev_h, C.byref(d), None) == -1
    assert env.reset_dist is None                 # nothing was taken over
    for pre, h in (("satenv_cpu_", env._h), ("satenv_", dev_h)):
        fn = lambda name: getattr(lib, pre + name)        # noqa: E731
        assert fn("default_reset_dist")(None) == -1
        assert fn("set_reset_dist")(None, C.byref(good), None) == -1
        assert fn("set_reset_dist")(h, None, None) == -1
        assert fn("get_reset_dist")(None, C.byref(good)) == -1
        assert fn("get_reset_dist")(h, None) == -1
        assert fn("get_episode_index")(None, dummy, None) == -1
        assert fn("get_episode_index")(h, None, None) == -1
        assert fn("set_episode_index")(None, None, None) == -1
    with pytest.raises(L.NativeError):
        env.set_reset_dist(R.HI, R.LO, SEED)
    with pytest.raises(ValueError):
        env.set_reset_dist(R.LO[:5], R.HI, SEED)


def test_distribution_over_4096_envs():
    n, seed = 4096, 20260101
    lo, hi = R.LO, R.HI
    # the seed is chosen so that the restatement alone satisfies the three properties
    ref = R.expected_draw(lo, hi, seed, np.arange(n), 0)
    env = _env(n=n)
    env.set_reset_dist(lo, hi, seed)
    env.reset(0)
    k = _kin(env)
    assert _bits_equal(k, ref)
    for x in (ref, k):
        assert ((x > lo[:, None]) & (x < hi[:, None])).all()
        assert len({x[:, i].tobytes() for i in range(n)}) == n
        span = hi - lo
        assert (np.abs(x.mean(axis=1) - (lo + hi) / 2) <= 6 * span / np.sqrt(12 * n)).all()


def test_args_param_and_reset_box():
    from satrl.env import reset_box, reset_constants
    from satrl.trainer import args_param
    a = args_param()
    assert a.reset_spread is None and a.reset_seed is None
    assert _bits_equal(reset_constants(), R.CENTRE)
    assert reset_box(None) is None
    lo, hi = reset_box(list(R.HALF))
    assert _bits_equal(lo, R.LO) and _bits_equal(hi, R.HI)
    lo, hi = reset_box({"lo": R.LO - 1, "hi": R.HI + 2})
    assert _bits_equal(lo, R.LO - 1) and _bits_equal(hi, R.HI + 2)
    with pytest.raises(ValueError):
        reset_box([1.0] * 11)
    with pytest.raises(ValueError):
        reset_box([-1.0] * 12)
