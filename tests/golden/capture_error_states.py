#!/usr/bin/env python3
"""Capture the exactly degenerate f64 states of error_states.npz: the inputs
under which calculate_orbital_elements (satellite_function.py:161-255) takes
its 4-element (e == 0, circular) or 5-element (2/r - v**2/mu == 0, parabolic)
branch, which the env step records as SATENV_ERR_ORBIT_CIRCULAR (-4) and
SATENV_ERR_ORBIT_PARABOLIC (-5).  Uses the project's own oracle only.

Such states are measure zero, so they are found by search: bisect a scale on
a velocity until the sign of 2/r - v**2/mu changes, then scan the ulp
neighbours for an exact zero.  Every hit is accepted only if

  * the oracle (orc_danger_zone / orc_step) returns the code, and
  * an exact-fma restatement of the branch tests returns it both with
    v_norm ** 2 = pow(v_norm, 2.0) (glibc: the oracle and the host build) and
    with v_norm * v_norm (the gfx950 build, satenv_device.h pow2): everything
    else on the path is +, -, *, /, sqrt and fma, the same bits on both.

Fixture error_states.npz:
  mu                         3.986e14
  abs_R, abs_V [2][3]        absolute states, abs_code [2] = (-4, -5)
  step_kin [7][12]           PRE-step kinematics Pp Pv Ep Ev of one env each
  step_code [7]              what one step records for the row
  step_set [7]               0: the default parameters (STM, the reference's
                             CW point); 1: the `alt` parameters below
  step_names [7]
  clean_kin [2][12]          a clean counterpart per parameter set
  alt_R_cw, alt_V_cw [3]     parameter set 1: this CW point, propagator 1
                             (RK4) with cw_omega 0 -- a craft moves on a
                             straight line, exactly for the drift used, and
                             arrives on the circular absolute state
Every row is to be stepped with zero actions for both agents, vel_int 0 (under
Flag 0 with the pursuer frozen, planes dis < d_range and dz != 0, the
pursuer's action is free: environment.py:91-97 zeroes it).

Run:  python tests/golden/capture_error_states.py      (~2 s)
"""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import oracle as O  # noqa: E402

MU = 3.986e14
R_CW = np.array([27098000.0, 32306000.0, 0.0])
V_CW = np.array([-2350.0, 1970.0, 0.0])
PV0 = [3.5, -1.25, 0.5]          # clean velocities (exact in f32 and f64)
EV0 = [0.5, -0.25, 0.25]
P_RESET, E_RESET = [200000.0, 0.0, 0.0], [18000.0, 0.0, 0.0]   # environment.py:67-71


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # one rounding


def dot3(a, b):
    return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]))


def branch(R, V, square):
    """(code, en) of orbital_elements' two exact-zero tests (satenv_device.h)."""
    R, V = [float(x) for x in R], [float(x) for x in V]
    r, v = np.sqrt(dot3(R, R)), np.sqrt(dot3(V, V))
    v2 = float(square(v))
    en = 2.0 / r - v2 / MU
    if en == 0.0:
        return -5, en
    c1, c2 = v2 / MU - 1.0 / r, dot3(R, V) / MU
    E = [c1 * R[i] - c2 * V[i] for i in range(3)]
    return (-4 if np.sqrt(dot3(E, E)) == 0.0 else 0), en


SQUARES = (lambda v: v * v, lambda v: v ** 2.0)


def ulps(x, k):
    """x moved by k units in the last place (x != 0)"""
    b = np.array([x], np.float64).view(np.int64)
    return float((b + (k if x > 0 else -k)).view(np.float64)[0])


def codes(R, V):
    return [branch(R, V, s)[0] for s in SQUARES]


def params(alt=None):
    p = O.params(d_capture=15000.0, max_episode_steps=1000)
    if alt is not None:
        p.R_cw[:], p.V_cw[:] = list(alt[0]), list(alt[1])
        p.cw_omega, p.propagator, p.rk4_substeps = 0.0, 1, 10
    return p


def step(p, kin, flag=0, dz=1, dis=50000.0, pa=(0, 0, 0), ea=(0, 0, 0)):
    """orc_step of one env from the pre-step kinematics: (rc, post-step kin)."""
    e = O.OrcEnv()
    O.lib().orc_env_init(C.byref(e))
    e.Pp[:], e.Pv[:], e.Ep[:], e.Ev[:] = (list(kin[0:3]), list(kin[3:6]), list(kin[6:9]), list(kin[9:12]))
    e.fuel_c = e.fuel_t = 320.0
    e.dis, e.dz, e.vel_int, e.flag = dis, dz, 0, flag
    pa, ea = np.array(pa, np.float32), np.array(ea, np.float32)
    obs, r, d = np.zeros(18), C.c_double(0), C.c_int32(0)
    fp = C.POINTER(C.c_float)
    rc = O.lib().orc_step(C.byref(p), C.byref(e), pa.ctypes.data_as(fp), ea.ctypes.data_as(fp), 1,
                          obs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r), C.byref(d))
    return rc, np.array(e.Pp[:] + e.Pv[:] + e.Ep[:] + e.Ev[:])


def find_abs():
    """the circular and the parabolic speed at R = (42164000, 0, 0), V along y"""
    R = [42164000.0, 0.0, 0.0]
    out = []
    for want, v0 in ((-4, np.sqrt(MU / R[0])), (-5, np.sqrt(2 * MU / R[0]))):
        for k in range(-2000, 2001):
            V = [0.0, ulps(v0, k), 0.0]
            if codes(R, V) == [want, want]:
                rc_c, _ = O.danger_zone(R, V, R_CW + [2000, 2000, 1000], V_CW + [1.71, 1.14, 1.3], 320.0, 0)
                rc_t, _ = O.danger_zone(R_CW + [2000, 2000, 1000], V_CW + [1.71, 1.14, 1.3], R, V, 320.0, 0)
                if rc_c == want and rc_t == want:
                    out.append((R, V))
                    break
        else:
            raise SystemExit(f"no exact {want} state found")
    return out


def find_parabolic_step(p, kin, craft, direction, cw, lo, hi, span=14, want_rc=-5):
    """kin with the velocity of `craft` (0 pursuer, 1 evader) replaced by the
    first ulp neighbour of s * direction whose POST-step absolute state is
    exactly parabolic."""
    o = 3 + 6 * craft
    direction = np.asarray(direction, np.float64)

    def post_en(s):
        k = np.array(kin, np.float64)
        k[o:o + 3] = s * direction
        _, post = step(p, k)
        return branch(cw[0] + post[o - 3:o], cw[1] + post[o:o + 3], SQUARES[1])[1]

    assert post_en(lo) > 0 > post_en(hi)
    while np.nextafter(lo, np.inf) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if post_en(mid) > 0 else (lo, mid)
    base = lo * direction
    axes = [a for a in range(3) if direction[a] != 0.0]
    offs = [(i, j) for i in range(-span, span + 1) for j in (range(-span, span + 1) if len(axes) > 1 else [0])]
    if len(axes) == 1:
        offs = [(i, 0) for i in range(-400, 401)]
    offs.sort(key=lambda ij: (abs(ij[0]) + abs(ij[1]), ij))
    tried = hits = 0
    first = None
    for i, j in offs:
        v = base.copy()
        for a, m in zip(axes, (i, j)):
            v[a] = ulps(v[a], m)
        k = np.array(kin, np.float64)
        k[o:o + 3] = v
        rc, post = step(p, k)
        tried += 1
        if rc == want_rc and codes(cw[0] + post[o - 3:o], cw[1] + post[o:o + 3]) == [-5, -5]:
            hits += 1
            if first is None:
                first = k
    print(f"  craft {craft}, direction {direction.tolist()}: {hits} of {tried} ulp neighbours are parabolic "
          "after the step")
    return first


def find_any_direction(p, kin, craft, cw, want_rc=-5):
    """the alt set's velocities are coarse (its positions move by exact
    amounts), so one neighbourhood can miss the zero: try a few directions"""
    for d in ([0.6, 0.8, 0.0], [0.8, 0.6, 0.0], [0.28, 0.96, 0.0], [0.96, 0.28, 0.0], [-0.6, 0.8, 0.0],
              [0.352, 0.936, 0.0], [-0.28, 0.96, 0.0], [-0.8, 0.6, 0.0], [0.1, 0.99, 0.0], [-0.1, 0.99, 0.0],
              [0.45, 0.89, 0.0], [-0.45, 0.89, 0.0], [0.7, 0.71, 0.0], [-0.7, 0.71, 0.0]):
        k = find_parabolic_step(p, kin, craft, d, cw, 500.0, 8000.0, want_rc=want_rc)
        if k is not None:
            return k
    raise SystemExit("no parabolic post-step state found")


def main():
    (Rc, Vc), (Rp, Vp) = find_abs()
    print("circular  V =", Vc, "\nparabolic V =", Vp)
    for R, V in ((Rc, Vc), (Rp, Vp)):        # the offset round trip of set_state / satenv_rd_orbits
        assert np.array_equal(R_CW + (np.array(R) - R_CW), R) and np.array_equal(V_CW + (np.array(V) - V_CW), V)

    p0 = params()
    cw0 = (R_CW, V_CW)
    u = V_CW / np.linalg.norm(V_CW)
    clean0 = np.array(P_RESET + PV0 + E_RESET + EV0)
    k_c = find_parabolic_step(p0, clean0, 0, u, cw0, 1000.0, 1500.0)
    k_t = find_parabolic_step(p0, clean0, 1, u, cw0, 1000.0, 1500.0)
    k_b = k_c.copy()
    k_b[9:12] = k_t[9:12]

    # parameter set 1: the circular absolute state is where a craft that starts at (18000, 0, 0)
    # ... drifting at `rest` arrives after one step (cw_omega 0: a straight line, exact for these values)
    rest = [0.25, 0.5, -0.25]
    arrive = np.array(E_RESET) + 100.0 * np.array(rest)
    alt = (np.array(Rc) - arrive, np.array(Vc) - rest)
    assert np.array_equal(alt[0] + arrive, Rc) and np.array_equal(alt[1] + rest, Vc)
    p1 = params(alt)
    clean1 = np.array(P_RESET + PV0 + E_RESET + EV0)
    k_cc = np.array(E_RESET + rest + P_RESET + EV0)              # the chaser arrives on the circular state
    k_tc = np.array(P_RESET + PV0 + E_RESET + rest)              # the target does
    k_pc = find_any_direction(p1, k_tc, 0, alt)   # parabolic chaser, circular target
    k_cp = find_any_direction(p1, k_cc, 1, alt, want_rc=-4)   # (the chaser's code comes first)   # circular chaser, parabolic target

    names = ["chaser_parabolic", "target_parabolic", "both_parabolic", "chaser_circular", "target_circular",
             "chaser_parabolic_target_circular", "chaser_circular_target_parabolic"]
    kin = np.stack([k_c, k_t, k_b, k_cc, k_tc, k_pc, k_cp])
    code = np.array([-5, -5, -5, -4, -4, -5, -4], np.int32)
    sets = np.array([0, 0, 0, 1, 1, 1, 1], np.int32)
    rng = np.random.default_rng(5)
    for name, k, c, s in zip(names, kin, code, sets):
        p = p1 if s else p0
        pa = rng.uniform(-1.6, 1.6, 3)
        got = [step(p, k, flag=0, dz=1, pa=pa)[0],        # Flag 0, pursuer frozen: its action is zeroed
               step(p, k, flag=0, dz=0, dis=np.inf)[0],   # Flag 0, both move (zero actions)
               step(p, k, flag=1, dz=1)[0], step(p, k, flag=1, dz=0)[0],
               step(p, k, flag=2, dz=1)[0]]
        print(f"  {name}: orc_step -> {got}")
        assert got == [c, c, c, c, 0], (name, got)
    for s, k in ((0, clean0), (1, clean1)):
        assert step(p1 if s else p0, k)[0] == 0
    np.savez_compressed(os.path.join(HERE, "error_states.npz"), mu=MU, abs_R=np.array([Rc, Rp]),
                        abs_V=np.array([Vc, Vp]), abs_code=np.array([-4, -5], np.int32), step_kin=kin,
                        step_code=code, step_set=sets, step_names=np.array(names), clean_kin=np.stack([clean0, clean1]),
                        alt_R_cw=alt[0], alt_V_cw=alt[1])
    print("error_states.npz written")


if __name__ == "__main__":
    main()
