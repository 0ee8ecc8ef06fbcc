"""Observation noise on the host build (include/satenv.h satenv_obs_noise):
the model's host entry against the NumPy restatement bit for bit, the error's
bounds and its bias / refresh structure, an autoreset run whose f32 rows are
the restatement of its truth while everything else is the run without the
noise, the bitwise identities of a disabled or all-zero noise, the refusals
and the Python keywords.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import obs_noise_reference as R
from reset_dist_reference import HI, LO

SEED = 0x0BADC0DE12345678
OFFSET = 2 ** 32 - 2          # the five envs' global ids straddle the counter's second word
BOTH = ((120.0, 0.04, 35.0, 0.015), (300.0, 0.08, 60.0, 0.03))     # (bias_pos, bias_vel, pos, vel) per craft
SPEC = {"pursuer": dict(zip(("bias_pos", "bias_vel", "pos", "vel"), BOTH[0])),
        "evader": dict(zip(("bias_pos", "bias_vel", "pos", "vel"), BOTH[1]))}


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _spec(craft=(R.EXACT, R.EXACT), hold=1, seed=0, enabled=1, offset=0):
    import satrl._lib as L
    d = L.SatenvObsNoise()
    for g in (0, 1):
        d.bias_pos[g], d.bias_vel[g], d.pos[g], d.vel[g] = craft[g]
    d.hold, d.seed, d.env_offset, d.enabled = hold, seed, offset, enabled
    return d


def _host(fn, d, gid, ep, cnt, k, rows=True):
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    m, obs = np.empty_like(k), np.empty((len(k), 18), dtype=np.float32)
    for i in range(len(k)):
        src, dst, row = np.ascontiguousarray(k[i]), np.empty(12), np.empty(18, dtype=np.float32)
        assert fn(C.byref(d), int(gid[i]), int(ep[i]), int(cnt[i]), src.ctypes.data_as(dp), dst.ctypes.data_as(dp),
                  row.ctypes.data_as(fp) if rows else None) == 0
        m[i], obs[i] = dst, row
    return m, obs


def _cases(hold=3):
    """Every (gid, ep, cnt) of gids around 0 and 2^32 + 5, two episodes and counts on both sides of a
    boundary of hold 3; a GEO-sized truth with -0.0 entries."""
    gids = [0, 1, 2, 2 ** 32 + 4, 2 ** 32 + 5, 2 ** 32 + 6, 2 ** 40 + 9]
    grid = [(g, e, c) for g in gids for e in (0, 1, 7) for c in (0, 2, 3, 5, 6)]
    gid, ep, cnt = (np.array(x, dtype=np.int64) for x in zip(*grid))
    rng = np.random.default_rng(5)
    k = rng.uniform(LO, HI, (len(grid), 12))
    k[::4, 1] = -0.0
    k[1::4, 10] = -0.0
    k[2::4, 4] = 0.0
    return gid, ep, cnt, k


@pytest.mark.parametrize("entry", ["satenv_obs_noise_host", "satenv_cpu_obs_noise_host"])
def test_host_entry_equals_restatement_bitwise(entry):
    import satrl._lib as L
    fn = getattr(L.lib(), entry)
    gid, ep, cnt, k = _cases()
    bias_only = ((120.0, 0.04, 0.0, 0.0), (300.0, 0.08, 0.0, 0.0))
    refresh_only = ((0.0, 0.0, 35.0, 0.015), (0.0, 0.0, 60.0, 0.03))
    mixed = ((120.0, 0.0, 0.0, 0.015), (0.0, 0.08, 60.0, 0.0))       # one product per scalar, of either kind
    for craft in (BOTH, bias_only, refresh_only, mixed, (R.EXACT, BOTH[1]), (BOTH[0], R.EXACT)):
        d = _spec(craft, hold=3, seed=SEED, offset=77)                 # (the offset is not part of gid here)
        m, obs = _host(fn, d, gid, ep, cnt, k)
        want = R.measured(craft, 3, SEED, gid, ep, cnt, k)
        assert _bits_equal(m, want), (entry, craft)
        assert _bits_equal(obs, R.row_of(want)), (entry, craft)
        for g in (0, 1):
            cols = slice(6 * g, 6 * g + 6)
            if craft[g] == R.EXACT:                                    # an exact craft keeps its bits, -0.0 included
                assert _bits_equal(m[:, cols], k[:, cols])
            else:
                assert (m[:, cols] != k[:, cols]).any(axis=1).all()
    d = _spec(BOTH, hold=3, seed=SEED)
    m, _ = _host(fn, d, gid, ep, cnt, k, rows=False)                   # obs_out may be null
    assert _bits_equal(m, R.measured(BOTH, 3, SEED, gid, ep, cnt, k))
    d.enabled = 0
    m, obs = _host(fn, d, gid, ep, cnt, k)
    assert _bits_equal(m, k) and _bits_equal(obs, R.row_of(k))


@pytest.mark.parametrize("entry", ["satenv_obs_noise_host", "satenv_cpu_obs_noise_host"])
def test_error_is_bounded_and_its_bias_is_held_for_the_episode(entry):
    import satrl._lib as L
    fn = getattr(L.lib(), entry)
    gid, ep, cnt, _ = _cases()
    zero = np.zeros((len(gid), 12))
    B, W = R.widths(BOTH)
    e, _ = _host(fn, _spec(BOTH, hold=3, seed=SEED), gid, ep, cnt, zero)
    assert (np.abs(e) <= B + W).all() and (e != 0.0).all()
    # cnt 3 and 5 share the refreshed error of hold 3 (as 0 and 2 do); 2 and 6 have their own
    e = e.reshape(7, 3, 5, 12)                                         # [gid, ep, cnt 0 2 3 5 6, scalar]
    assert (e[:, :, 2] == e[:, :, 3]).all() and (e[:, :, 0] == e[:, :, 1]).all()
    assert (e[:, :, 1] != e[:, :, 2]).all() and (e[:, :, 3] != e[:, :, 4]).all()
    b, _ = _host(fn, _spec((BOTH[0][:2] + (0.0, 0.0), BOTH[1][:2] + (0.0, 0.0)), hold=3, seed=SEED), gid, ep, cnt, zero)
    assert (np.abs(b) <= B).all() and (b != 0.0).all()
    b = b.reshape(7, 3, 5, 12)
    assert (b == b[:, :, :1]).all()                                    # one bias over all cnt of an ep
    assert (b[:, 0] != b[:, 1]).all() and (b[:, 1] != b[:, 2]).all()   # ... and another in the next
    w, _ = _host(fn, _spec(((0.0, 0.0) + BOTH[0][2:], (0.0, 0.0) + BOTH[1][2:]), hold=3, seed=SEED), gid, ep, cnt, zero)
    assert (np.abs(w) <= W).all() and (w != 0.0).all()


N, T, MAX_STEPS, HOLD = 5, 14, 5, 3
ACT = ((0.05, 0.02), (0.2, 0.1))


def _env(n=N, **kw):
    from satrl.env import VecSatellites
    kw.setdefault("d_capture", 1000.0)          # the starts are far outside it: every episode times out
    kw.setdefault("max_episode_steps", MAX_STEPS)
    return VecSatellites(n, device="cpu", threads=2, **kw)


def _actions(n=N, t=T):
    rng = np.random.default_rng(11)
    return torch.from_numpy(rng.uniform(-1.6, 1.6, (2, t, n, 3)).astype(np.float32))


def _run(env, with_resets=True):
    """reset, then T autoreset steps under a reset box and act noise: per write the f32 row, the
    reward, done, the state planes, the episode index, and stats at the end."""
    act = _actions()
    if with_resets:
        env.set_reset_dist(LO, HI, SEED ^ 1, env_offset=OFFSET)
        env.set_act_noise(*ACT, seed=SEED ^ 2, env_offset=OFFSET)
    out = []
    obs = env.reset(0)
    for t in range(T + 1):
        if t:
            obs, r, d = env.step_autoreset(act[0, t - 1], act[1, t - 1])
        f, i = env.get_state()
        rec = {"obs": obs.numpy().copy(), "f64": f.numpy().copy(), "i32": i.numpy().copy(),
               "ep": env.episode_index().numpy().copy()}
        if t:
            rec["rew"], rec["done"] = r.numpy().copy(), d.numpy().copy()
        out.append(rec)
    out[-1]["stats"] = env.stats.numpy().copy()
    return out


def test_autoreset_run_measures_its_truth_and_changes_nothing_else():
    plain, noisy = _env(), _env()
    noisy.set_obs_noise(SPEC["pursuer"], SPEC["evader"], hold=HOLD, seed=SEED, env_offset=OFFSET)
    assert noisy.measures and not plain.measures
    assert noisy.obs_noise() == dict(SPEC, hold=HOLD, seed=SEED, env_offset=OFFSET)
    a, b = _run(plain), _run(noisy)
    gid = OFFSET + np.arange(N)
    resets = 0
    for t, (x, y) in enumerate(zip(a, b)):
        for key in x:
            if key != "obs":
                assert _bits_equal(x[key], y[key]), (t, key)
        truth = y["f64"][0:12].T
        assert _bits_equal(x["obs"], R.row_of(truth)), t                       # the plain run writes the truth
        ep, cnt = y["ep"], y["i32"][1]
        assert (cnt == (t % MAX_STEPS)).all() and (ep == 1 + t // MAX_STEPS).all(), t
        want = R.row_of(R.measured(BOTH, HOLD, SEED, gid, ep, cnt, truth))
        assert _bits_equal(y["obs"], want), t
        assert (y["obs"] != x["obs"]).any(axis=1).all(), t
        resets += int(t > 0 and y["done"].all())
    assert resets == 2 and noisy.check_errors() == 0


def test_step_and_masked_reset_follow_the_same_rule():
    env = _env()
    env.set_obs_noise(SPEC["pursuer"], SPEC["evader"], hold=HOLD, seed=SEED, env_offset=OFFSET)
    gid = OFFSET + np.arange(N)
    act = _actions()
    env.reset(0)
    cnt = torch.tensor([1, 2, 3, 5, 6], dtype=torch.int32)            # the caller's counts, not the device's
    obs64 = torch.empty((N, 18), dtype=torch.float64)
    obs = torch.empty((N, 18), dtype=torch.float32)
    env.step(act[0, 0], act[1, 0], cnt, obs_out=obs, obs64_out=obs64)
    f, _ = env.get_state()
    assert _bits_equal(obs64.numpy()[:, 6:18], f.numpy()[0:12].T.copy())           # obs64 is the truth
    assert _bits_equal(obs64.numpy()[:, 0:6], (f.numpy()[0:6] - f.numpy()[6:12]).T.copy())
    assert _bits_equal(obs.numpy(), R.measured_rows(BOTH, HOLD, SEED, gid, 1, cnt.numpy(), obs64.numpy()))
    # a masked reset rewrites every row: the reset envs at (advanced index, 0), the others where they are
    env.step_autoreset(act[0, 1], act[1, 1])                         # (counts 2 3 4, and 6 7: those two time out)
    ep0, cnt0 = env.episode_index().numpy(), env.get_state()[1].numpy()[1]
    assert list(ep0) == [1, 1, 1, 2, 2] and list(cnt0) == [2, 3, 4, 0, 0]
    mask = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    obs = env.reset(0, mask=mask, obs_out=obs, obs64_out=obs64)
    ep, (_, i) = env.episode_index().numpy(), env.get_state()
    assert list(ep) == [2, 1, 1, 3, 2] and list(i.numpy()[1]) == [0, 3, 4, 0, 0]
    assert _bits_equal(obs.numpy(), R.measured_rows(BOTH, HOLD, SEED, gid, ep, i.numpy()[1], obs64.numpy()))


def test_disabled_and_all_zero_noise_are_the_exact_env_bitwise():
    plain = _run(_env())
    off = _env()
    off.set_obs_noise(SPEC["pursuer"], SPEC["evader"], hold=HOLD, seed=SEED, env_offset=OFFSET)
    off.clear_obs_noise()
    assert off.measures and off.obs_noise() is None
    zero = _env()
    zero.set_obs_noise(hold=HOLD, seed=SEED, env_offset=OFFSET)
    assert zero.obs_noise() is not None
    for what, env in (("disabled", off), ("all zero", zero)):
        for t, (x, y) in enumerate(zip(_run(env), plain)):
            for key in x:
                assert _bits_equal(x[key], y[key]), (what, t, key)


def test_bad_arguments_are_refused_by_name():
    import satrl._lib as L
    lib = L.lib()
    env = _env(n=3)
    good = _spec((BOTH[0], BOTH[1]), 9, 3, enabled=1)
    assert lib.satenv_default_obs_noise(C.byref(good)) == 0
    want = L.SatenvObsNoise()
    want.hold = 1
    assert bytes(good) == bytes(want) and good.enabled == 0 and good.hold == 1
    cpu_default = _spec((BOTH[0], BOTH[1]), 9, 3)
    assert lib.satenv_cpu_default_obs_noise(C.byref(cpu_default)) == 0 and bytes(cpu_default) == bytes(good)
    dummy = C.create_string_buffer(4096)          # a non-null handle: refused before it is looked at
    dev_h = C.cast(dummy, C.c_void_p)
    k = (C.c_double * 12)()
    m = (C.c_double * 12)()
    row = (C.c_float * 18)()
    slots = {"satenv_cpu_": lib.satenv_cpu_last_error, "satenv_": lib.satenv_last_error}

    def variants():
        for field in ("bias_pos", "bias_vel", "pos", "vel"):
            for g in (0, 1):
                for bad in (float("nan"), float("inf"), -0.25):
                    d = _spec()
                    getattr(d, field)[g] = bad
                    yield d, f"{field}[{g}]".encode(), b"finite and >= 0"
        for hold in (0, -3):
            yield _spec(hold=hold), b"hold", b">= 1"

    for pre, h in (("satenv_cpu_", env._h), ("satenv_", dev_h)):
        fn = lambda name: getattr(lib, pre + name)        # noqa: E731

        def refused(name, *args, words=()):
            assert fn("default_obs_noise")(None) == -1     # another entry point's text first
            assert slots[pre]().startswith((pre + "default_obs_noise: ").encode())
            assert fn(name)(*args) == -1, (pre, name)
            msg = slots[pre]()
            assert msg.startswith((pre + name + ": ").encode()), msg
            for w in words:
                assert w in msg, (w, msg)

        for d, field, why in variants():
            refused("set_obs_noise", h, C.byref(d), None, words=(field, why))
            refused("obs_noise_host", C.byref(d), 0, 0, 1, k, m, row, words=(field, why))
        refused("set_obs_noise", None, C.byref(good), None, words=(b"null",))
        refused("set_obs_noise", h, None, None, words=(b"null",))
        refused("get_obs_noise", None, C.byref(good), words=(b"null",))
        refused("get_obs_noise", h, None, words=(b"null",))
        refused("obs_noise_host", None, 0, 0, 1, k, m, row, words=(b"null",))
        refused("obs_noise_host", C.byref(good), 0, 0, 1, None, m, row, words=(b"null",))
        refused("obs_noise_host", C.byref(good), 0, 0, 1, k, None, row, words=(b"null",))
        assert fn("obs_noise_host")(C.byref(good), 0, 0, 1, k, m, None) == 0      # obs_out alone may be null
    assert env.obs_noise() is None and not env.measures          # nothing was taken over
    with pytest.raises(L.NativeError, match=r"satenv_cpu_set_obs_noise: hold"):
        env.set_obs_noise((1.0, 0.1), (1.0, 0.1), hold=0)
    with pytest.raises(ValueError, match=r"obs_noise: evader's vel"):
        env.set_obs_noise((1.0, 0.1), (1.0, -0.1))


def test_args_param_and_spec_validation():
    from satrl.env import obs_noise_spec
    from satrl.trainer import args_param
    a = args_param()
    assert a.obs_noise is None and a.obs_noise_seed is None
    assert obs_noise_spec(None) is None
    assert obs_noise_spec((50, 0.02)) == ((0.0, 0.0, 50.0, 0.02), (0.0, 0.0, 50.0, 0.02), 1)
    assert obs_noise_spec({"evader": [10, 0]}) == (R.EXACT, (0.0, 0.0, 10.0, 0.0), 1)
    assert obs_noise_spec({"pursuer": {"bias_pos": 3, "vel": 1}, "hold": 10}) == ((3.0, 0.0, 0.0, 1.0), R.EXACT, 10)
    assert obs_noise_spec(SPEC) == (BOTH[0], BOTH[1], 1)
    assert obs_noise_spec({}) == (R.EXACT, R.EXACT, 1)
    b = args_param(obs_noise={"pursuer": (50.0, 0.02), "hold": 4}, obs_noise_seed=9)
    assert b.obs_noise == {"pursuer": (50.0, 0.02), "hold": 4} and b.obs_noise_seed == 9
    for bad, key in [((0.1,), "pair"), ((0.1, 0.2, 0.3), "pair"), (0.1, "pair"), ("both", "pair"),
                     ((-0.1, 0.0), "pos"), ((0.0, -1.0), "vel"), ((float("nan"), 0.0), "pos"),
                     ((0.0, float("inf")), "vel"), ({"chaser": (0.1, 0.1)}, "chaser"),
                     ({"pursuer": {"bias": 1.0}}, "bias"), ({"evader": "x"}, "evader"),
                     ({"pursuer": (0.1, None)}, "vel"), ({"pursuer": {"bias_vel": -1}}, "bias_vel"),
                     ({"hold": 0}, "hold"), ({"hold": 2.5}, "hold"), ({"evader": {"bias_pos": "x"}}, "bias_pos")]:
        with pytest.raises(ValueError, match="obs_noise") as e:
            obs_noise_spec(bad)
        assert key in str(e.value), (bad, str(e.value))
        with pytest.raises(ValueError, match="obs_noise"):
            args_param(obs_noise=bad)
