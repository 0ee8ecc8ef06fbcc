"""tests/test_env_errors_cpu.py on the GPU: the error word, the error lanes
and non-finite input on every schedule of the step (the wide kernel at 64 / 32
/ 16 envs per workgroup, the four-solve split kernel, the one-lane kernel --
each records the code by code of its own, satenv_kernels.hip) and, at
propagator 2, on every RK45 instantiation of the split kernel.  The host
build of the same tree is the reference: state planes, done and dz bit for
bit, rewards within 1e-12 relative (libm differs).
"""
import numpy as np
import pytest
import torch

import env_error_cases as X
from conftest import assert_dz_libm_ties

pytestmark = pytest.mark.gpu

_host = {}
FIGURES = {}   # worst relative differences from the host build seen by same_as_host, printed by the tests


def host_lanes(oracle, fx, row, flag):
    """the host build's outputs of the planted launch (row, flag), computed once"""
    if (row, flag) not in _host:
        _host[(row, flag)] = X.check_error_lanes("cpu", None, oracle, fx, row, flag)
    return _host[(row, flag)]


def same_as_host(got, ref, what, nan_lanes=(), rk45=False):
    """State planes, done and dz bitwise the host build's, rewards within 1e-12
    relative.  In `nan_lanes` (envs fed a non-finite value) a NaN must be a NaN
    in both and everything else has the same bits: which NaN an invalid
    operation returns (its sign, its payload) is the hardware's choice, x86
    and gfx950 choose differently, and IEEE 754 leaves it open.  rk45: the
    propagated kinematics are not the same bits on the two targets -- the step
    size control calls pow(err, -0.2), OCML here and glibc there -- so the 12
    kinematic planes, dis and the obs are held to rel 1e-13 of the plane's
    scale, the bar of test_env_rk45_cw_mode_vs_reference_solve_ivp; fuel, done,
    dz, count and bits stay bitwise."""
    for k in ("f64", "i32", "done", "obs64"):
        a, b = got[k], ref[k]
        if k in ("f64", "i32"):
            a, b = a.T, b.T
        if rk45 and k in ("f64", "obs64"):
            cols = [c for c in range(a.shape[1]) if k == "obs64" or c not in (12, 13)]
            x, y = a[:, cols], b[:, cols]
            fin = np.isfinite(y)
            assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~fin & ~np.isnan(y)],
                                                                                y[~fin & ~np.isnan(y)]), (what, k)
            bad = sorted(set(np.nonzero(~fin)[0].tolist()))
            assert set(bad) <= set(nan_lanes), (what, k, bad)
            scale = np.maximum(np.abs(np.where(fin, y, 0.0)).max(axis=0, keepdims=True), 1e-300)
            with np.errstate(invalid="ignore"):
                err = (np.abs(np.where(fin, x - y, 0.0)) / scale).max()
            FIGURES[k] = max(FIGURES.get(k, 0.0), float(err))
            assert err <= 1e-13, (what, k, err)
            if k == "obs64":
                continue
            a, b = a[:, 12:14], b[:, 12:14]
        for lane in range(X.N):
            x, y = np.ascontiguousarray(a[lane]), np.ascontiguousarray(b[lane])
            if lane in nan_lanes and x.dtype.kind == "f":
                nx, ny = np.isnan(x), np.isnan(y)
                assert np.array_equal(nx, ny), (what, k, lane, x, y)
                x, y = x[~nx], y[~ny]
            assert x.tobytes() == y.tobytes(), (what, k, lane, x, y)
    r, rr = got["reward"], ref["reward"]
    both_nan = np.isnan(r) & np.isnan(rr)
    with np.errstate(invalid="ignore"):
        rel = np.where(both_nan, 0.0, np.abs(r - rr) / np.abs(rr))
    FIGURES["reward"] = max(FIGURES.get("reward", 0.0), float(np.nanmax(rel)))
    assert (both_nan | (rel <= 1e-12)).all(), (what, np.nonzero(~(rel <= 1e-12))[0], r, rr)


@pytest.mark.parametrize("row", range(7))
@pytest.mark.parametrize("schedule", X.SCHEDULES)
def test_gpu_error_lanes(oracle, schedule, row):
    """test_host_error_lanes on one device schedule, Flag 0 and Flag 1, and the
    whole launch against the host build's."""
    fx = X.fixtures()
    for flag in (0, 1):
        got = X.check_error_lanes("cuda", schedule, oracle, fx, row, flag)
        same_as_host(got, host_lanes(oracle, fx, row, flag), (schedule, row, flag))


@pytest.mark.parametrize("schedule", X.SCHEDULES)
def test_gpu_two_kinds_in_different_lanes(schedule):
    """-5 in lanes 0 and 64, -4 in lanes 31 and 129: one of the two is recorded."""
    fx = X.fixtures()
    f, i32, pa, ea, cnt = X.clean_launch(fx, 1, 0)
    for lane, row in ((0, 5), (64, 5), (31, 3), (129, 3)):
        X.plant(f, i32, pa, ea, lane, fx["step_kin"][row], 0)
    env = X.make_env("cuda", 1, 0, fx, schedule)
    X.step_once(env, f, i32, pa, ea, cnt)
    assert env.check_errors() in (-4, -5)


def test_gpu_danger_zone_returns_the_codes(oracle):
    """satenv_danger_zone: the negative code exactly in the planted rows; the
    other rows are the golden counts (up to libm ties, as test_danger_zone_counts)."""
    from satrl import _lib
    fx = X.fixtures()
    d, Xs, want = X.dz_planted(fx)
    n = len(Xs)
    Xd = torch.tensor(Xs, dtype=torch.float64, device="cuda")
    fuel = torch.tensor(d["fuel"], dtype=torch.float64, device="cuda")
    mode = torch.tensor(d["mode"], dtype=torch.int32, device="cuda")
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().satenv_danger_zone(n, _lib.ptr(Xd), _lib.ptr(fuel), _lib.ptr(mode), _lib.ptr(out),
                                             _lib.stream_ptr()), "satenv_danger_zone")
    got = out.cpu().numpy()
    rows = sorted(want)
    assert got[rows].tolist() == [want[r] for r in rows]
    rest = np.setdiff1d(np.arange(n), rows)
    assert (got[rest] >= 0).all()
    bad = assert_dz_libm_ties(oracle, Xs[rest, 0:3], Xs[rest, 3:6], Xs[rest, 6:9], Xs[rest, 9:12], d["fuel"][rest],
                              d["mode"][rest], got[rest], d["count_glibc"][rest], "dz_cases planted", absolute=True)
    assert len(bad) <= 2, len(bad)          # test_danger_zone_counts' bar


def test_gpu_rd_orbits_status():
    """satenv_rd_orbits: -4 / -5 in the envs whose pursuer holds the circular /
    parabolic absolute state (as a relative state: R - R_cw and V - V_cw are
    exact, test_fixture_rows_return_their_code_in_the_oracle), 0 elsewhere."""
    from satrl import reachable as RD
    from conftest import R_CW, V_CW
    fx = X.fixtures()
    f, i32, _, _, _ = X.clean_launch(fx, 0, 2)
    want = np.zeros(X.N, np.int32)
    for j, lane in enumerate(X.LANES):
        k = j % 2
        f[0:3, lane], f[3:6, lane] = fx["abs_R"][k] - R_CW, fx["abs_V"][k] - V_CW
        want[lane] = fx["abs_code"][k]
    env = X.make_env("cuda", 0, 2, fx)
    env.set_state(torch.from_numpy(f).cuda(), torch.from_numpy(i32).cuda())
    orbits, status = RD.env_orbits(env)
    assert np.array_equal(status.cpu().numpy(), want)
    o = orbits.cpu().numpy()
    assert (o[list(X.LANES), 0:3] == 0).all() and np.isfinite(o).all()


HOST_LIMIT, GPU_LIMIT = 60.0, 120.0   # caps, far above the healthy times printed beside them


@pytest.mark.parametrize("propagator", [0, 1, 2])
def test_gpu_nonfinite_input_returns(tmp_path, propagator):
    """test_host_nonfinite_input_returns on every device schedule (propagator
    2: every RK45 instantiation of the split kernel, step and step_autoreset),
    in a fresh child process under a time limit.  The host build's child runs
    and is checked first: no case reaches the GPU that did not return there."""
    zh, _ = X.run_child("cpu", propagator, tmp_path / "host.npz", HOST_LIMIT)
    X.check_nonfinite(zh, "cpu", propagator)
    zg, _ = X.run_child("cuda", propagator, tmp_path / "gpu.npz", GPU_LIMIT)
    X.check_nonfinite(zg, "cuda", propagator)
    variants = X.rk45_variants("cuda") if propagator == 2 else ("plain",)
    scheds = X.SCHEDULES if propagator != 2 else X.SCHEDULES[:1]
    for si in range(len(scheds)):
        for variant in variants:
            for name, _, _, lane in [("clean", None, None, None)] + X.nonfinite_cases():
                got = {k: zg[f"s{si}_{variant}_{name}_{k}"] for k in X.OUT_KEYS}
                ref = {k: zh[f"s0_plain_{name}_{k}"] for k in X.OUT_KEYS}
                same_as_host(got, ref, (propagator, si, variant, name), () if lane is None else (lane,),
                             rk45=propagator == 2)
    print(f"propagator {propagator}: worst relative difference from the host build so far: {FIGURES}")


def _trainer():
    from satrl.trainer import VecTrainer, args_param
    args = args_param(batch_size=64 * 4, mini_batch_size=64, hidden_width=64, K_epochs=2, num_envs=64, horizon=4,
                      max_episode_steps=50, seed=2, chkpt_dir="/tmp")
    return VecTrainer(args, flag=0, d_capture=X.D_CAPTURE)


def test_trainer_raises_on_a_recorded_error():
    """VecTrainer.finish_iteration reads the error word: with one of 64 envs on
    the chaser-parabolic fixture (pursuer frozen, so whatever the policies
    sample the first step records -5) iteration() raises an EnvError naming
    the code; the same trainer without it does not."""
    from satrl.env import EnvError
    fx = X.fixtures()
    tr = _trainer()
    tr.iteration()
    assert tr.env.check_errors() == 0
    tr = _trainer()
    f, i32 = tr.env.get_state()
    lane = 37
    f[0:12, lane] = torch.from_numpy(fx["step_kin"][0]).to(f.device)
    f[14, lane] = 50000.0
    i32[0, lane] = 1
    i32[2, lane] = 0                    # float velocities (vel_int 0), Flag 0
    tr.env.set_state(f, i32)
    with pytest.raises(EnvError, match=r"-5 \(SATENV_ERR_ORBIT_PARABOLIC\)") as e:
        tr.iteration()
    assert e.value.code == -5
