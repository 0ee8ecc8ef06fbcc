"""Actuation noise on the host build (include/satenv.h satenv_act_noise):
the model's host entry against the NumPy restatement bit for bit, the
restatement's own bounds, a noisy autoreset run step-locked to the oracle fed
with the restatement's executed actions, the bitwise identities of a disabled
or all-zero noise, the refusals and the Python keywords.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import act_noise_reference as A
from conftest import assert_dz_libm_ties

N = 130            # two 64-env workgroups + 2 lanes on the device; the same N here
SEED = 0x1234ABCD5678EF01
OFFSET = 1000
D_CAPTURE = 1000.0  # the reset's 182 km are far outside it: every episode times out on its third step
NOISE = ((0.05, 0.02), (0.2, 0.1))


def _env(n=N, **kw):
    from satrl.env import VecSatellites
    kw.setdefault("d_capture", D_CAPTURE)
    kw.setdefault("max_episode_steps", 3)
    return VecSatellites(n, device="cpu", threads=2, **kw)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _spec(mag=(0.0, 0.0), dire=(0.0, 0.0), seed=0, enabled=1, offset=0):
    import satrl._lib as L
    d = L.SatenvActNoise()
    d.mag[:], d.dir[:] = list(mag), list(dire)
    d.seed, d.env_offset, d.enabled = seed, offset, enabled
    return d


def _host(fn, d, gid, ep, cnt, agent, a):
    out = np.empty_like(a)
    fp = C.POINTER(C.c_float)
    for i in range(len(a)):
        row, dst = np.ascontiguousarray(a[i]), np.empty(3, dtype=np.float32)
        assert fn(C.byref(d), int(gid[i]), int(ep[i]), int(cnt[i]), agent, row.ctypes.data_as(fp),
                  dst.ctypes.data_as(fp)) == 0
        out[i] = dst
    return out


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    gid = rng.integers(0, 2 ** 20, n)
    gid[: n // 4] = rng.integers(2 ** 32, 2 ** 62, n // 4)           # the counter's second word
    ep = rng.integers(0, 2 ** 31 - 1, n)
    cnt = rng.integers(1, 1001, n)
    a = rng.uniform(-1.6, 1.6, (n, 3)).astype(np.float32)
    a[0:8] = 0.0
    a[8:16] = np.float32(1.6) * rng.choice([-1.0, 1.0], (8, 3)).astype(np.float32)
    a[16:24, 1] = 0.0
    return gid, ep, cnt, a


@pytest.mark.parametrize("entry", ["satenv_act_noise_host", "satenv_cpu_act_noise_host"])
def test_host_entry_equals_restatement_bitwise(entry):
    import satrl._lib as L
    fn = getattr(L.lib(), entry)
    gid, ep, cnt, a = _cases(1500, 3)
    moved = 0
    for agent, (mag, dire) in [(0, (0.05, 0.02)), (1, (0.05, 0.02)), (0, (1.0, 0.0)), (1, (0.0, 0.5)), (0, (0.0, 0.0))]:
        d = _spec((mag, mag), (dire, dire), SEED, offset=77)          # (the offset is not part of gid here)
        got = _host(fn, d, gid, ep, cnt, agent, a)
        want = A.executed(mag, dire, SEED, agent, gid, ep, cnt, a)
        assert _bits_equal(got, want), (entry, agent, mag, dire)
        assert (got[0:8] == 0.0).all()                                # coasting is exact
        if mag == 0.0 and dire == 0.0:
            assert _bits_equal(got, a)                                # no draw, the commanded bits
        else:
            moved += int((got != a).any(axis=1).sum())
    assert moved > 4 * 1400
    # the two agents' streams differ, and a disabled spec copies
    d = _spec((0.05, 0.05), (0.02, 0.02), SEED)
    assert not _bits_equal(_host(fn, d, gid, ep, cnt, 0, a), _host(fn, d, gid, ep, cnt, 1, a))
    d.enabled = 0
    assert _bits_equal(_host(fn, d, gid, ep, cnt, 1, a), a)


def test_restatement_stays_inside_its_bounds():
    gid, ep, cnt, a = _cases(4000, 4)
    a64 = a.astype(np.float64)
    norm = np.sqrt((a64 ** 2).sum(axis=1))
    for mag, dire in [(0.05, 0.02), (1.0, 0.0), (0.0, 0.5), (0.3, 0.3), (1.0, 1.0)]:
        for agent in (0, 1):
            out = A.executed(mag, dire, SEED, agent, gid, ep, cnt, a)
            assert out.dtype == np.float32 and (np.abs(out) <= np.float32(1.6)).all()
            # where the clip cuts, it moves a' towards a (|a| <= 1.6); 2^-22: two f32 half-ulps at 1.6
            bound = mag * np.abs(a64) + (dire * norm)[:, None] + 2.0 ** -22
            assert (np.abs(out.astype(np.float64) - a64) <= bound).all(), (mag, dire, agent)
            z = A.uniforms(SEED, agent, gid, ep, cnt)
            assert (np.abs(z) < 1.0).all()


def _dz_term(dz):
    return np.where(dz == 0, -1.0, dz * 0.5)


def test_noisy_autoreset_run_equals_oracle_fed_with_the_executed_actions(oracle):
    env, twin = _env(), _env()
    env.set_act_noise(*NOISE, seed=SEED, env_offset=OFFSET)
    twin.set_act_noise(*NOISE, seed=SEED, env_offset=OFFSET)
    assert env.noisy and env.act_noise() == {"pursuer": NOISE[0], "evader": NOISE[1], "seed": SEED,
                                             "env_offset": OFFSET}
    gid = OFFSET + np.arange(N)
    pa, ea = A.actions(N)
    tpa, tea = torch.from_numpy(pa), torch.from_numpy(ea)
    env.reset(0)
    ties = counted = moved = 0
    for step in range(1, 8):
        f0, i0 = [x.numpy().copy() for x in env.get_state()]
        ep = env.episode_index().numpy().copy()
        cnt = i0[1] + 1
        assert (ep == 1 + (step - 1) // 3).all() and (cnt == 1 + (step - 1) % 3).all()
        xpa, xea = A.executed_pair(NOISE, SEED, gid, ep, cnt, pa, ea)
        moved += int((xpa != A.clip16(pa)).any(axis=1).sum()) + int((xea != A.clip16(ea)).any(axis=1).sum())
        fo, io, ro, do = oracle.step_planes(f0, i0, xpa, xea, cnt, d_capture=D_CAPTURE, max_episode_steps=3)
        # the same step through satenv_cpu_step with the caller's count, for the f64 reward and obs
        twin.set_state(torch.from_numpy(f0), torch.from_numpy(i0))
        twin.set_episode_index(torch.from_numpy(ep))
        obs64 = torch.empty((N, 18), dtype=torch.float64)
        _, r64, d64 = twin.step(tpa, tea, torch.from_numpy(cnt.astype(np.int32)), obs64_out=obs64)
        ft, it = [x.numpy() for x in twin.get_state()]
        obs, r, dn = env.step_autoreset(tpa, tea)
        f1, i1 = [x.numpy() for x in env.get_state()]
        dn = dn.numpy().astype(np.int32)
        assert np.array_equal(dn, do) and np.array_equal(d64.numpy().astype(np.int32), do), step
        assert (dn == (1 if step % 3 == 0 else 0)).all(), step
        live = dn == 0
        assert _bits_equal(f1[:, live], fo[:, live]) and _bits_equal(ft, fo), step
        assert np.array_equal(i1[2, live], io[2, live]) and np.array_equal(it[2], io[2]), step
        ob_o = np.concatenate([fo[0:3] - fo[6:9], fo[3:6] - fo[9:12], fo[0:12]]).T
        assert _bits_equal(obs.numpy()[live], ob_o.astype(np.float32)[live]), step
        assert _bits_equal(obs64.numpy(), ob_o.copy()), step
        # tests/test_env_gpu.py's tie rule for the danger-zone count, and its cap
        bad = assert_dz_libm_ties(oracle, fo[0:3].T, fo[3:6].T, fo[6:9].T, fo[9:12].T, fo[12], io[2] & 3,
                                  np.where(live, i1[0], io[0]), io[0], f"act noise step {step}")
        assert np.array_equal(np.where(live, it[0], io[0]), np.where(live, i1[0], io[0]))
        ties += len(bad)
        counted += int(live.sum())
        expect = ro.copy()
        expect[bad] = ro[bad] + (_dz_term(i1[0][bad]) - _dz_term(io[0][bad]))
        assert (np.abs(r64.numpy() - expect) <= 1e-12).all(), (step, np.abs(r64.numpy() - expect).max())
        e32 = expect.astype(np.float32)
        assert (np.abs(r.numpy() - e32) <= np.spacing(np.abs(e32))).all(), step
        # the fuel is charged for the executed action (an over-burn costs fuel)
        assert _bits_equal(ft[12], fo[12]) and _bits_equal(ft[13], fo[13])
    assert counted == 5 * N and ties <= 2, (ties, counted)
    assert moved > 7 * 2 * (N - 4)
    assert (env.episode_index().numpy() == 3).all() and env.check_errors() == 0


def _run7(env, pa, ea):
    out = [(env.reset(0).numpy().copy(),)]
    for _ in range(7):
        o, r, d = env.step_autoreset(pa, ea)
        out.append((o.numpy().copy(), r.numpy().copy(), d.numpy().copy()) +
                   tuple(x.numpy().copy() for x in env.get_state()) + (env.episode_index().numpy().copy(),))
    return out


def test_disabled_and_all_zero_noise_are_the_exact_env_bitwise():
    pa, ea = (torch.from_numpy(x) for x in A.actions(N))
    plain = _run7(_env(), pa, ea)
    off = _env()
    off.set_act_noise(*NOISE, seed=SEED, env_offset=OFFSET)
    off.clear_act_noise()
    assert off.noisy and off.act_noise() is None
    zero = _env()
    zero.set_act_noise((0.0, 0.0), (0.0, 0.0), seed=SEED, env_offset=OFFSET)
    assert zero.act_noise() is not None
    one = _env()                                   # one agent exact: its actions keep their bits, the other's move
    one.set_act_noise((0.0, 0.0), NOISE[1], seed=SEED, env_offset=OFFSET)
    runs = {"disabled": _run7(off, pa, ea), "all zero": _run7(zero, pa, ea)}
    for what, run in runs.items():
        for step, (x, y) in enumerate(zip(run, plain)):
            for k, (p, q) in enumerate(zip(x, y)):
                assert _bits_equal(p, q), (what, step, k)
    noisy = _run7(one, pa, ea)
    assert _bits_equal(noisy[1][3][0:6], plain[1][3][0:6]) and _bits_equal(noisy[1][3][12], plain[1][3][12])
    assert not _bits_equal(noisy[1][3][9:12], plain[1][3][9:12]) and not _bits_equal(noisy[1][3][13], plain[1][3][13])


def test_bad_arguments_are_refused_by_name():
    import satrl._lib as L
    lib = L.lib()
    env = _env(n=3)
    good = L.SatenvActNoise()
    assert lib.satenv_default_act_noise(C.byref(good)) == 0
    assert bytes(good) == bytes(L.SatenvActNoise()) and good.enabled == 0
    cpu_default = _spec((0.5, 0.5), (0.5, 0.5), 9)
    assert lib.satenv_cpu_default_act_noise(C.byref(cpu_default)) == 0 and bytes(cpu_default) == bytes(good)
    dummy = C.create_string_buffer(4096)          # a non-null handle: refused before it is looked at
    dev_h = C.cast(dummy, C.c_void_p)
    a = (C.c_float * 3)(0.1, 0.2, 0.3)
    out = (C.c_float * 3)()
    slots = {"satenv_cpu_": lib.satenv_cpu_last_error, "satenv_": lib.satenv_last_error}

    def variants():
        for field in ("mag", "dir"):
            for g in (0, 1):
                for bad in (float("nan"), float("inf"), -0.25):
                    d = _spec()
                    getattr(d, field)[g] = bad
                    yield d, f"{field}[{g}]".encode(), b"finite and >= 0"
        for g in (0, 1):
            d = _spec()
            d.mag[g] = 1.0 + 2.0 ** -52
            yield d, f"mag[{g}]".encode(), b"must not exceed 1"

    for pre, h in (("satenv_cpu_", env._h), ("satenv_", dev_h)):
        fn = lambda name: getattr(lib, pre + name)        # noqa: E731

        def refused(name, *args, words=()):
            assert fn("default_act_noise")(None) == -1     # another entry point's text first
            assert slots[pre]().startswith((pre + "default_act_noise: ").encode())
            assert fn(name)(*args) == -1, (pre, name)
            msg = slots[pre]()
            assert msg.startswith((pre + name + ": ").encode()), msg
            for w in words:
                assert w in msg, (w, msg)

        for d, field, why in variants():
            refused("set_act_noise", h, C.byref(d), None, words=(field, why))
            refused("act_noise_host", C.byref(d), 0, 0, 1, 0, a, out, words=(field, why))
        refused("set_act_noise", None, C.byref(good), None, words=(b"null",))
        refused("set_act_noise", h, None, None, words=(b"null",))
        refused("get_act_noise", None, C.byref(good), words=(b"null",))
        refused("get_act_noise", h, None, words=(b"null",))
        refused("act_noise_host", None, 0, 0, 1, 0, a, out, words=(b"null",))
        refused("act_noise_host", C.byref(good), 0, 0, 1, 0, None, out, words=(b"null",))
        refused("act_noise_host", C.byref(good), 0, 0, 1, 0, a, None, words=(b"null",))
        refused("act_noise_host", C.byref(good), 0, 0, 1, 2, a, out, words=(b"agent",))
        refused("act_noise_host", C.byref(good), 0, 0, 1, -1, a, out, words=(b"agent",))
    assert env.act_noise() is None and not env.noisy          # nothing was taken over
    d = _spec((1.0, 0.0), (0.0, 3.0), 5)                      # the edges are valid: mag 1, a wide pointing error
    assert lib.satenv_cpu_set_act_noise(env._h, C.byref(d), None) == 0
    with pytest.raises(L.NativeError, match=r"satenv_cpu_set_act_noise: mag\[1\]"):
        env.set_act_noise((0.1, 0.1), (1.5, 0.1), seed=1)
    with pytest.raises(L.NativeError, match=r"dir\[0\]"):
        env.set_act_noise((0.1, -0.1), (0.5, 0.1), seed=1)


def test_args_param_and_spec_validation():
    from satrl.env import act_noise_spec
    from satrl.trainer import args_param
    a = args_param()
    assert a.act_noise is None and a.act_noise_seed is None
    assert act_noise_spec(None) is None
    assert act_noise_spec((0.05, 0.02)) == ((0.05, 0.02), (0.05, 0.02))
    assert act_noise_spec({"evader": [0.1, 0]}) == ((0.0, 0.0), (0.1, 0.0))
    assert act_noise_spec({"pursuer": (1, 2), "evader": (0, 0)}) == ((1.0, 2.0), (0.0, 0.0))
    assert act_noise_spec({}) == ((0.0, 0.0), (0.0, 0.0))
    b = args_param(act_noise={"pursuer": (0.05, 0.02)}, act_noise_seed=9)
    assert b.act_noise == {"pursuer": (0.05, 0.02)} and b.act_noise_seed == 9
    for bad in [(0.1,), (0.1, 0.2, 0.3), 0.1, "both", (-0.1, 0.0), (0.0, -1.0), (1.5, 0.0), (float("nan"), 0.0),
                (0.0, float("inf")), {"chaser": (0.1, 0.1)}, {"pursuer": (2.0, 0.0)}, {"evader": "x"},
                {"pursuer": (0.1, None)}]:
        with pytest.raises(ValueError, match="act_noise"):
            act_noise_spec(bad)
        with pytest.raises(ValueError, match="act_noise"):
            args_param(act_noise=bad)
