"""Shared cases of test_env_errors_cpu.py / test_env_errors_gpu.py: envs whose
step records a device error code (include/satenv.h: -4 circular, -5 parabolic,
-6 RK45 step too small / non-finite state) and envs with non-finite state or
actions.  Not a test module.

The degenerate states are tests/golden/error_states.npz (capture_error_states.py:
found by search, proven against the oracle).  An env is `planted` by writing a
fixture row into its state planes, with planes dz = 1 and dis = 50000 (<
d_range: under Flag 0 the pursuer is frozen and its action zeroed,
environment.py:91-97, so the row is hit whatever the pursuer's action) and
zero actions for whoever moves.

Run as a program it is the child process of the non-finite cases:
    python env_error_cases.py <cpu|cuda> <propagator> <out.npz>
steps every non-finite case on every schedule of the device and saves what it
saw; the parent asserts.  A step that never returns is the parent's time limit.
"""
import os
import sys

import numpy as np

N = 130
LANES = (0, 31, 63, 64, 129)           # first lane, wave interior, last lane of a wave, first of the next, last env
D_CAPTURE = 15000.0
# the device schedules of test_step_kernels_agree_bitwise_ragged; the host build has one
SCHEDULES = ((2, 64), (2, 32), (2, 16), (1, 64), (0, 64))
ERR_CIRCULAR, ERR_PARABOLIC, ERR_STEP = -4, -5, -6


def fixtures():
    from conftest import golden
    return golden("error_states")


def schedules(device):
    return (None,) if device == "cpu" else SCHEDULES


def make_env(device, pset=0, flag=0, fx=None, schedule=None, **kw):
    """N envs on the host build (2 threads) or the GPU; pset 1: the fixture's
    alternate parameters (its CW point, RK4 with cw_omega 0)."""
    from satrl.env import VecSatellites
    kw.setdefault("max_episode_steps", 1000)
    if pset == 1:
        kw.update(R_cw=fx["alt_R_cw"], V_cw=fx["alt_V_cw"], cw_omega=0.0, propagator=1)
    if device == "cpu":
        kw["threads"] = 2
    env = VecSatellites(N, device=device, d_capture=D_CAPTURE, Flag=flag, **kw)
    if schedule is not None:
        env.set_step_kernel(*schedule)
    return env


def clean_launch(fx, pset, flag, seed=3):
    """State planes and actions of N clean, distinct envs around the fixture's
    clean row: (f64 [15][N], i32 [3][N], pa [N][3], ea [N][3], count [N])."""
    from satrl.env import pack_bits
    rng = np.random.default_rng(seed)
    f = np.zeros((15, N))
    f[0:12] = fx["clean_kin"][pset][:, None]
    f[0:3] += rng.uniform(-20000.0, 20000.0, (3, N))
    f[6:9] += rng.uniform(-5000.0, 5000.0, (3, N))
    f[3:6] += rng.uniform(-1.0, 1.0, (3, N))
    f[9:12] += rng.uniform(-1.0, 1.0, (3, N))
    f[12] = f[13] = 320.0
    lanes = np.arange(N)
    f[14] = np.where(lanes % 2 == 0, 50000.0, np.inf)        # every gating arm among the clean envs
    i32 = np.zeros((3, N), np.int32)
    i32[0] = lanes % 3
    i32[2] = pack_bits(0, 0, 0, flag)
    pa = rng.uniform(-1.6, 1.6, (N, 3)).astype(np.float32)
    ea = rng.uniform(-1.6, 1.6, (N, 3)).astype(np.float32)
    return f, i32, pa, ea, np.full(N, 5, np.int32)


def plant(f, i32, pa, ea, lane, kin, flag):
    """fixture row `kin` into env `lane` of a launch (in place)"""
    f[0:12, lane] = kin
    f[14, lane] = 50000.0
    i32[0, lane] = 1
    ea[lane] = 0.0
    if flag != 0:                       # Flag 1 with dz != 0: both move; Flag 0: the pursuer is frozen, any action
        pa[lane] = 0.0


def step_once(env, f, i32, pa, ea, count):
    """set_state + one satenv_step: everything the launch wrote, as numpy"""
    import torch
    dev = env.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    env.set_state(t(f), t(i32))
    obs = torch.empty((N, 18), dtype=torch.float32, device=dev)
    obs64 = torch.empty((N, 18), dtype=torch.float64, device=dev)
    _, r, d = env.step(t(pa), t(ea), t(count), obs_out=obs, obs64_out=obs64)
    fa, ia = env.get_state()
    return {"obs": obs.cpu().numpy(), "obs64": obs64.cpu().numpy(), "reward": r.cpu().numpy(),
            "done": d.cpu().numpy(), "f64": fa.cpu().numpy(), "i32": ia.cpu().numpy()}


OUT_KEYS = ("obs", "obs64", "reward", "done", "f64", "i32")


def other_lanes_bitwise(a, b, lanes):
    """every output of every env outside `lanes` has the same bits in a and b"""
    keep = np.ones(N, bool)
    keep[list(lanes)] = False
    for k in OUT_KEYS:
        x, y = a[k], b[k]
        if k in ("f64", "i32"):
            x, y = x.T, y.T
        x, y = np.ascontiguousarray(x[keep]), np.ascontiguousarray(y[keep])
        assert x.tobytes() == y.tobytes(), k


def reward_count0(k, pa, p_zero, dis_prev, flag, d_capture=D_CAPTURE):
    """The non-terminal reward of environment.py:161-175, :251 with a
    danger-zone count of 0, restated in f64 from
    the post-step kinematics k, the clipped pursuer action and dis before the
    step.  Imports nothing from the product."""
    k = np.asarray(k, np.float64)
    Pp, Pv, Ep, Ev = k[0:3], k[3:6], k[6:9], k[9:12]
    rel = Pp - Ep
    dis = np.sqrt(rel @ rel)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = lambda a, b: (a / np.sqrt(a @ a)) @ (b / np.sqrt(b @ b))   # noqa: E731
        r = 1.0 if dis < dis_prev else -1.0                               # :161-164
        r += -1.0 if d_capture <= dis <= 4 * d_capture else -2.0
        r += -1.0                                                         # dangerous_zone == 0
        r += 1 * cos(Pp, Ep) + 0.6 * cos(Pv, Ev) + 0.2 * cos(rel, Pv)     # reward_of_action3, 1, 2
        a = np.asarray(pa, np.float32)
        if not p_zero and (a != 0).all():                                 # reward_of_action4, :388
            ua = (a / np.sqrt((a.astype(np.float64) ** 2).sum()).astype(np.float32)).astype(np.float64)
            r += 2 * -((rel / dis) @ ua)
    return r if flag == 0 else -r


def oracle_step(O, fx, pset, kin, flag, dz=1, dis=50000.0, pa=(0, 0, 0), ea=(0, 0, 0), count=5):
    """orc_step of one env from pre-step kinematics: (rc, f64 [15] after, bits after)"""
    import ctypes as C
    from satrl.env import pack_bits
    p = O.params(d_capture=D_CAPTURE, max_episode_steps=1000)
    if pset == 1:
        p.R_cw[:], p.V_cw[:] = fx["alt_R_cw"].tolist(), fx["alt_V_cw"].tolist()
        p.cw_omega, p.propagator, p.rk4_substeps = 0.0, 1, 10
    e = O.OrcEnv()
    O.lib().orc_env_init(C.byref(e))
    kin = [float(x) for x in kin]
    e.Pp[:], e.Pv[:], e.Ep[:], e.Ev[:] = kin[0:3], kin[3:6], kin[6:9], kin[9:12]
    e.fuel_c = e.fuel_t = 320.0
    e.dis, e.dz, e.vel_int, e.flag = float(dis), int(dz), 0, int(flag)
    pa, ea = np.array(pa, np.float32), np.array(ea, np.float32)
    obs, r, d = np.zeros(18), C.c_double(0), C.c_int32(0)
    fp = C.POINTER(C.c_float)
    rc = O.lib().orc_step(C.byref(p), C.byref(e), pa.ctypes.data_as(fp), ea.ctypes.data_as(fp), int(count),
                          obs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r), C.byref(d))
    after = np.array(e.Pp[:] + e.Pv[:] + e.Ep[:] + e.Ev[:] + [e.fuel_c, e.fuel_t, e.dis])
    return rc, after, pack_bits(e.fuel_c_mode, e.fuel_t_mode, e.vel_int, e.flag)


def check_error_lanes(device, schedule, O, fx, row, flag):
    """Fixture row `row` planted at LANES of an otherwise clean launch: the
    word, its stickiness, what the error lanes write, and that nobody else
    notices.  Returns the planted launch's outputs (the GPU tests compare
    them with the host build's)."""
    pset, code, kin = int(fx["step_set"][row]), int(fx["step_code"][row]), fx["step_kin"][row]
    what = (device, schedule, str(fx["step_names"][row]), flag)
    f0, i0, pa0, ea0, cnt = clean_launch(fx, pset, flag)
    env = make_env(device, pset, flag, fx, schedule)
    assert env.check_errors() == 0                               # a fresh handle
    clean = step_once(env, f0, i0, pa0, ea0, cnt)
    assert env.check_errors() == 0, what
    f, i32, pa, ea = f0.copy(), i0.copy(), pa0.copy(), ea0.copy()
    for lane in LANES:
        plant(f, i32, pa, ea, lane, kin, flag)
    env = make_env(device, pset, flag, fx, schedule)
    got = step_once(env, f, i32, pa, ea, cnt)
    assert env.check_errors() == code, what
    other_lanes_bitwise(got, clean, LANES)
    for lane in LANES:
        rc, after, bits = oracle_step(O, fx, pset, kin, flag, pa=pa[lane], ea=ea[lane])
        assert rc == code
        # the lane finished its step: the oracle's state where it stopped, count 0 stored, not done
        assert got["f64"][:, lane].tobytes() == after.tobytes(), what
        assert got["i32"][:, lane].tolist() == [0, 5, bits], what
        assert got["done"][lane] == 0, what
        k = after[0:12]
        o = np.concatenate([k[0:3] - k[6:9], k[3:6] - k[9:12], k[0:3], k[3:6], k[6:9], k[9:12]])
        assert got["obs64"][lane].tobytes() == o.tobytes(), what
        assert got["obs"][lane].tobytes() == o.astype(np.float32).tobytes(), what
        p_zero = flag != 1                                       # planted dz 1, dis < d_range: the pursuer is frozen
        rel = kin[0:3] - kin[6:9]
        want = reward_count0(k, np.clip(pa[lane], np.float32(-1.6), np.float32(1.6)), p_zero, np.sqrt(rel @ rel), flag)
        r = got["reward"][lane]
        print(f"{what} lane {lane}: reward {r!r}, restated {want!r}")
        assert (np.isnan(r) and np.isnan(want)) or abs(r - want) <= 1e-12 * abs(want), (what, lane, r, want)
    # sticky across a later clean step of the same handle
    step_once(env, f0, i0, pa0, ea0, cnt)
    assert env.check_errors() == code, what
    # Flag 2 steps the same states without a danger-zone count: nothing to record
    from satrl.env import pack_bits
    env2 = make_env(device, pset, 2, fx, schedule)
    i2 = i32.copy()
    i2[2] = pack_bits(0, 0, 0, 2)
    out2 = step_once(env2, f, i2, pa, ea, cnt)
    assert env2.check_errors() == 0, what
    assert not out2["done"].any() and (out2["reward"] == 0).all(), what
    return got


def dz_planted(fx):
    """dz_cases.npz with the absolute fixture states planted as the chaser
    (rows 0, 63) and as the target (rows 64, last)"""
    from conftest import golden
    d = golden("dz_cases")
    Xs = np.ascontiguousarray(d["X"], np.float64).copy()
    n = len(Xs)
    rows = {0: (0, 0), 63: (1, 0), 64: (0, 1), n - 1: (1, 1)}     # row -> (fixture, chaser / target)
    want = {}
    for r, (k, craft) in rows.items():
        Xs[r, 6 * craft:6 * craft + 3] = fx["abs_R"][k]
        Xs[r, 6 * craft + 3:6 * craft + 6] = fx["abs_V"][k]
        want[r] = int(fx["abs_code"][k])
    return d, Xs, want


# ---------------------------------------------------------------------------
# non-finite cases
# ---------------------------------------------------------------------------
BAD = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
# where the value goes: a state plane, or a component of an agent's action
SPOTS = {"pos": ("f64", 1), "vel": ("f64", 4), "fuel_c": ("f64", 12), "pa": ("pa", 2), "ea": ("ea", 0)}


def nonfinite_cases():
    """(name, spot, value name, lane): the lanes cycle through LANES"""
    out = []
    for s in SPOTS:
        for v in BAD:
            out.append((f"{s}_{v}", s, v, LANES[len(out) % len(LANES)]))
    return out


def expected_word(spot, vname, propagator):
    """What the error word must read after the poisoned launch.  Propagators 0
    and 1 have no code for a non-finite state (their loops have fixed trip
    counts).  Under propagator 2 cw_rk45 returns -6 for a non-finite state: a
    non-finite kinematic scalar, or a NaN action of an agent that moves (both
    do: Flag 0, dz 0).  An infinite action is not non-finite once executed --
    np.clip(a, -1.6, 1.6) makes it +-1.6 (environment.py:86-87) -- and fuel is
    not part of the propagated state."""
    if propagator != 2:
        return 0
    if spot in ("pos", "vel"):
        return ERR_STEP
    if spot in ("pa", "ea") and vname == "nan":
        return ERR_STEP
    return 0


def poison(f, i32, pa, ea, spot, vname, lane):
    where, idx = SPOTS[spot]
    f[14, lane] = np.inf                 # Flag 0, dz 0: both agents move
    i32[0, lane] = 0
    if where == "f64":
        f[idx, lane] = BAD[vname]
    elif where == "pa":
        pa[lane, idx] = BAD[vname]
    else:
        ea[lane, idx] = BAD[vname]


def rk45_variants(device):
    """Propagator 2 launches step_kernel_split<AUTORESET, RK45, DRAW, NOISE,
    MEAS>: the handle climbs the ladder when a reset distribution, actuation
    noise or observation noise was enabled once (cleared again here, so every
    rung computes the same bits).  The host build has one instantiation."""
    return ("plain",) if device == "cpu" else ("plain", "draw", "noise", "meas")


def climb(env, variant):
    if variant in ("draw", "noise", "meas"):
        lo = np.zeros(12)
        env.set_reset_dist(lo, lo + 1.0, seed=1)
        env.clear_reset_dist()
    if variant in ("noise", "meas"):
        env.set_act_noise((0.5, 0.5), (0.5, 0.5), seed=1)
        env.clear_act_noise()
    if variant == "meas":
        env.set_obs_noise((1.0, 1.0), (1.0, 1.0), seed=1)
        env.clear_obs_noise()


def child(device, propagator, out_path):
    """every non-finite case on every schedule: the poisoned and the clean
    launch of satenv_step, and three autoreset steps with max_episode_steps 3"""
    import time
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    fx = fixtures()
    out = {}
    variants = rk45_variants(device) if propagator == 2 else ("plain",)
    # propagator 2 has one schedule (the split kernel) whatever set_step_kernel says
    scheds = schedules(device) if propagator != 2 else schedules(device)[:1]
    t0 = time.perf_counter()
    for si, sched in enumerate(scheds):
        for variant in variants:
            tag = f"s{si}_{variant}"
            f0, i0, pa0, ea0, cnt = clean_launch(fx, 0, 0)
            env = make_env(device, 0, 0, fx, sched, propagator=propagator)
            climb(env, variant)
            clean = step_once(env, f0, i0, pa0, ea0, cnt)
            out[f"{tag}_clean_word"] = env.check_errors()
            for k in OUT_KEYS:
                out[f"{tag}_clean_{k}"] = clean[k]
            for name, spot, vname, lane in nonfinite_cases():
                print(f"[{time.perf_counter() - t0:6.2f}s] {device} propagator {propagator} schedule {sched} "
                      f"{variant}: {name} in lane {lane}", flush=True)
                f, i32, pa, ea = f0.copy(), i0.copy(), pa0.copy(), ea0.copy()
                poison(f, i32, pa, ea, spot, vname, lane)
                env = make_env(device, 0, 0, fx, sched, propagator=propagator)
                climb(env, variant)
                got = step_once(env, f, i32, pa, ea, cnt)
                out[f"{tag}_{name}_word"] = env.check_errors()
                for k in OUT_KEYS:
                    out[f"{tag}_{name}_{k}"] = got[k]
                # the poisoned env runs into its step limit and is reset in-kernel
                env = make_env(device, 0, 0, fx, sched, propagator=propagator, max_episode_steps=3)
                climb(env, variant)
                t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)   # noqa: E731
                env.set_state(t(f), t(i32 * np.array([[1], [0], [1]], np.int32)))        # counts 0
                dones = []
                for s in range(3):
                    _, _, d = env.step_autoreset(t(pa if s == 0 else pa0), t(ea if s == 0 else ea0), stats=False)
                    dones.append(d.cpu().numpy().copy())
                out[f"{tag}_{name}_ar_done"] = np.stack(dones)
                out[f"{tag}_{name}_ar_f64"] = env.get_state()[0].cpu().numpy()
                out[f"{tag}_{name}_ar_word"] = env.check_errors()
    if device != "cpu":
        torch.cuda.synchronize()
    out["seconds"] = time.perf_counter() - t0
    np.savez(out_path, **out)
    print(f"done in {out['seconds']:.2f} s", flush=True)


def run_child(device, propagator, out_path, limit):
    """child() in a fresh process under a time limit; returns (npz, seconds)"""
    import subprocess
    import time
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), device, str(propagator), str(out_path)],
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        log = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode()
        raise AssertionError(f"the {device} step at propagator {propagator} did not return within {limit} s; the "
                             f"child's last lines:\n" + "\n".join(log.splitlines()[-3:])) from None
    dt = time.perf_counter() - t0
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    print(f"{device} propagator {propagator}: the child took {dt:.1f} s (its steps {p.stdout.splitlines()[-1]}); "
          f"the limit is {limit} s")
    return np.load(out_path), dt


def check_nonfinite(z, device, propagator):
    """the assertions on one child's record that need no second device"""
    variants = rk45_variants(device) if propagator == 2 else ("plain",)
    scheds = schedules(device) if propagator != 2 else schedules(device)[:1]
    for si in range(len(scheds)):
        for variant in variants:
            tag = f"s{si}_{variant}"
            assert int(z[f"{tag}_clean_word"]) == 0
            clean = {k: z[f"{tag}_clean_{k}"] for k in OUT_KEYS}
            for name, spot, vname, lane in nonfinite_cases():
                what = (device, propagator, tag, name)
                got = {k: z[f"{tag}_{name}_{k}"] for k in OUT_KEYS}
                assert int(z[f"{tag}_{name}_word"]) == expected_word(spot, vname, propagator), what
                other_lanes_bitwise(got, clean, [lane])
                assert int(z[f"{tag}_{name}_ar_word"]) == expected_word(spot, vname, propagator), what
                done = z[f"{tag}_{name}_ar_done"]
                assert done[2, lane] == 1 and not done[:2, lane].any(), what       # ended by its count, not sooner
                assert np.isfinite(z[f"{tag}_{name}_ar_f64"][0:12, lane]).all(), what


if __name__ == "__main__":
    HERE = os.path.dirname(os.path.abspath(__file__))
    ROOT = os.path.dirname(HERE)
    for p in (HERE, ROOT, os.path.join(ROOT, "ppo-rl-satellite_amd"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    child(sys.argv[1], int(sys.argv[2]), sys.argv[3])
