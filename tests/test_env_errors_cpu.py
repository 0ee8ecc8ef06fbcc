"""The env step's device error word and its behaviour on non-finite input, on
the host build (include/satenv_cpu.h: the kernels' own source compiled by g++).
CPU only; tests/test_env_errors_gpu.py runs the same cases on every device
schedule.

include/satenv.h promises SATENV_ERR_ORBIT_CIRCULAR (-4), _PARABOLIC (-5) and
SATENV_ERR_STEP_TOO_SMALL (-6), sticky and reported by satenv_check().  The
states that raise -4 / -5 are measure zero, so they are fixtures
(tests/golden/error_states.npz, capture_error_states.py) planted into the
state planes of otherwise clean launches of N = 130 envs; env_error_cases.py
holds the cases.
"""
import ctypes as C

import numpy as np
import pytest

import env_error_cases as X

ROWS = range(7)


def test_fixture_rows_return_their_code_in_the_oracle(oracle):
    """Every fixture row returns the planted code from the oracle: as the
    chaser and as the target of orc_danger_zone (absolute rows, also after the
    relative round trip through the CW point), and from orc_step under Flag 0
    (pursuer frozen with a random action; both moving with zero actions) and
    Flag 1; Flag 2 returns 0.  The clean rows return 0."""
    fx = X.fixtures()
    from conftest import R_CW, V_CW
    other = (R_CW + [2000.0, 2000.0, 1000.0], V_CW + [1.71, 1.14, 1.3])
    for R, V, code in zip(fx["abs_R"], fx["abs_V"], fx["abs_code"]):
        R2, V2 = R_CW + (R - R_CW), V_CW + (V - V_CW)
        assert np.array_equal(R2, R) and np.array_equal(V2, V)
        assert oracle.danger_zone(R, V, *other, 320.0, 0)[0] == code
        assert oracle.danger_zone(*other, R, V, 320.0, 0)[0] == code
        assert oracle.orbital_elements(R, V)[0] == code
    rng = np.random.default_rng(5)
    for row in ROWS:
        pset, code, kin = int(fx["step_set"][row]), int(fx["step_code"][row]), fx["step_kin"][row]
        got = [X.oracle_step(oracle, fx, pset, kin, 0, pa=rng.uniform(-1.6, 1.6, 3))[0],
               X.oracle_step(oracle, fx, pset, kin, 0, dz=0, dis=np.inf)[0],
               X.oracle_step(oracle, fx, pset, kin, 1)[0], X.oracle_step(oracle, fx, pset, kin, 1, dz=0)[0],
               X.oracle_step(oracle, fx, pset, kin, 2)[0]]
        assert got == [code] * 4 + [0], (str(fx["step_names"][row]), got)
    for pset in (0, 1):
        assert X.oracle_step(oracle, fx, pset, fx["clean_kin"][pset], 0)[0] == 0
    assert sorted(set(fx["step_code"].tolist())) == [-5, -4]


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("row", ROWS)
def test_host_error_lanes(oracle, row, flag):
    """One fixture row planted at lanes 0, 31, 63, 64 and 129 (step_lane's
    error return, satenv_cpu.cpp's first-wins sink): check_errors() is the
    planted code, stays it across a later clean step, and is 0 on a fresh
    handle; the error lanes finish their step (the oracle's post-step state bit
    for bit, dz stored 0, not done) with the count-0 reward of an independent
    f64 restatement within 1e-12 relative; every other lane's obs, obs64,
    reward, done and state planes are bitwise those of the same launch with
    the lanes clean; under Flag 2 the same states record nothing.  Rows 5 and
    6 hold a parabolic chaser with a circular target and the reverse: the
    chaser's code is the one recorded."""
    X.check_error_lanes("cpu", None, oracle, X.fixtures(), row, flag)


def test_host_two_kinds_in_different_lanes():
    """-5 in lanes 0 and 64, -4 in lanes 31 and 129: the first to record wins
    and the order is free, so the word is one of the two."""
    fx = X.fixtures()
    f, i32, pa, ea, cnt = X.clean_launch(fx, 1, 0)
    for lane, row in ((0, 5), (64, 5), (31, 3), (129, 3)):
        X.plant(f, i32, pa, ea, lane, fx["step_kin"][row], 0)
    env = X.make_env("cpu", 1, 0, fx)
    X.step_once(env, f, i32, pa, ea, cnt)
    assert env.check_errors() in (-4, -5)


def test_host_danger_zone_returns_the_codes():
    """satenv_cpu_danger_zone: the negative code exactly in the planted rows,
    the golden counts everywhere else."""
    from satrl import _lib
    fx = X.fixtures()
    d, Xs, want = X.dz_planted(fx)
    n = len(Xs)
    assert n > 64
    fuel = np.ascontiguousarray(d["fuel"], np.float64)
    mode = np.ascontiguousarray(d["mode"], np.int32)
    out = np.zeros(n, np.int32)
    vp = C.c_void_p
    _lib.check(_lib.lib().satenv_cpu_danger_zone(n, Xs.ctypes.data_as(vp), fuel.ctypes.data_as(vp),
                                                 mode.ctypes.data_as(vp), out.ctypes.data_as(vp), None),
               "satenv_cpu_danger_zone")
    ref = d["count_glibc"].astype(np.int32).copy()
    for r, code in want.items():
        ref[r] = code
    assert np.array_equal(out, ref)
    assert (out < 0).sum() == len(want)


HOST_LIMIT = 60.0   # a cap, far above the healthy time printed beside it; a step that never returns ends here


@pytest.mark.parametrize("propagator", [0, 1, 2])
def test_host_nonfinite_input_returns(tmp_path, propagator):
    """NaN, +inf and -inf in a position, a velocity, fuel_c, a pursuer and an
    evader action component, each in one env of a clean launch, in a fresh
    child process under a time limit (before cw_rk45's exit test was written
    !(hc >= min_step), propagator 2 never returned from a non-finite state).
    The call returns; the word is 0 under propagators 0 and 1 and what
    env_error_cases.expected_word derives under 2; every other env is bitwise
    the clean launch's; with max_episode_steps 3 and the autoreset the poisoned
    env ends on its count and its 12 kinematic planes are finite again."""
    z, dt = X.run_child("cpu", propagator, tmp_path / "host.npz", HOST_LIMIT)
    X.check_nonfinite(z, "cpu", propagator)
