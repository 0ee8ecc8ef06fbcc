"""Environment front-ends over the HIP C-ABI (include/satenv.h).

* ``VecSatellites`` -- N environments resident in HBM, torch device tensors in
  and out; the engine's rollout path.
* ``satellites``    -- drop-in for the reference class
  (qiaobeibei/PPO-RL-Satellite environment.py:8-413): same constructor
  keywords, ``reset(Flag)`` / ``step(pursuer_action, escaper_action,
  epsiode_count)`` signatures, numpy outputs with the reference's dtypes and
  the attributes its callers read (``observation_space``, ``action_space``,
  ``d_capture`` ...).  It runs one env on the GPU kernel.

Both run on the host build of the same env ABI (include/satenv_cpu.h: the
step source compiled by g++, OpenMP over envs) when asked with
device="cpu" -- BASELINE.json configs[0], CPPO_main on a machine without a
GPU.  Nothing falls back to it: without a GPU the default device raises.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import ACT_DIM, OBS_DIM, SATENV_F64_PLANES, SATENV_I32_PLANES, check, ptr, require_cpu, require_cuda, stream_ptr

PYINT, I64, F32, F64 = 0, 1, 2, 3
STATE_F64 = ["Pp0", "Pp1", "Pp2", "Pv0", "Pv1", "Pv2", "Ep0", "Ep1", "Ep2", "Ev0", "Ev1", "Ev2",
             "fuel_c", "fuel_t", "dis"]
STATE_I32 = ["dz", "episode_count", "bits"]


ERROR_NAMES = {-4: "SATENV_ERR_ORBIT_CIRCULAR", -5: "SATENV_ERR_ORBIT_PARABOLIC", -6: "SATENV_ERR_STEP_TOO_SMALL"}


class EnvError(RuntimeError):
    """A step recorded a device error code (include/satenv.h): an env's orbit
    had no 6-element set (-4 circular, -5 parabolic: the reference crashes
    there) or propagator 2's RK45 stopped (-6: step too small, or a non-finite
    state).  `code` is what VecSatellites.check_errors() returned; the word is
    sticky, so the handle keeps reporting it."""

    def __init__(self, code, where=""):
        self.code = int(code)
        name = ERROR_NAMES.get(self.code, "unknown code")
        super().__init__(f"{where + ': ' if where else ''}the env step recorded error {self.code} ({name}); the "
                         "lane took a danger-zone count of 0 (-4 / -5) or kept its state unpropagated (-6), so "
                         "what was collected since the last check is not the reference's")


def default_params(**overrides) -> _lib.SatenvParams:
    p = _lib.SatenvParams()
    check(_lib.lib().satenv_default_params(C.byref(p)), "satenv_default_params")
    names = {f[0] for f in _lib.SatenvParams._fields_}
    for k, v in overrides.items():
        if k not in names:
            raise TypeError(f"unknown satenv parameter {k!r} (include/satenv.h satenv_params)")
        if k in ("R_cw", "V_cw", "stm", "init_kin"):
            getattr(p, k)[:] = [float(x) for x in np.asarray(v, dtype=np.float64).ravel()]
        else:
            setattr(p, k, v)
    return p


def stm(t: float = 100.0) -> np.ndarray:
    out = (C.c_double * 36)()
    check(_lib.lib().satenv_stm(float(t), out), "satenv_stm")
    return np.array(out[:]).reshape(6, 6)


def rk4_j2(rv, h, steps, out=None):
    """RK4 two-body + J2 propagation of 轨道外推-龙格库塔算法.py (km, km/s) for a
    batch of states rv [n][6] (f64, CUDA): `steps` steps of h seconds on the
    satenv_rk4_j2 kernel (one lane per state, SoA planes internally)."""
    n = rv.shape[0]
    _lib.require_cuda(rv, torch.float64, (n, 6), "rv")
    soa = rv.t().contiguous()
    check(_lib.lib().satenv_rk4_j2(n, ptr(soa), float(h), int(steps), ptr(soa), stream_ptr()), "satenv_rk4_j2")
    res = soa.t()
    if out is None:
        return res.contiguous()
    out.copy_(res)
    return out


def reset_constants() -> np.ndarray:
    """The 12 kinematic scalars of the reference's reset (environment.py:67-71)."""
    d = _lib.SatenvResetDist()
    check(_lib.lib().satenv_default_reset_dist(C.byref(d)), "satenv_default_reset_dist")
    return np.array(d.lo[:])


def reset_box(spread):
    """args_param.reset_spread -> (lo, hi) f64 [12], or None for None: a
    12-sequence gives half-widths around the reset's constants, a dict
    {"lo": ..., "hi": ...} the box itself."""
    if spread is None:
        return None
    if isinstance(spread, dict):
        lo, hi = (np.asarray(spread[k], dtype=np.float64).ravel() for k in ("lo", "hi"))
    else:
        half = np.asarray(spread, dtype=np.float64).ravel()
        if half.shape != (12,) or not (half >= 0).all():
            raise ValueError("reset_spread: 12 non-negative half-widths (Pp, Pv, Ep, Ev) or a dict of lo and hi")
        c = reset_constants()
        lo, hi = c - half, c + half
    if lo.shape != (12,) or hi.shape != (12,):
        raise ValueError("reset_spread: lo and hi are 12 scalars each")
    return lo, hi


def act_noise_spec(spec):
    """args_param.act_noise -> ((mag, dir) of the pursuer, (mag, dir) of the
    evader) as floats, or None for None: a pair (mag, dir) holds for both
    agents, a dict {"pursuer": (mag, dir), "evader": (mag, dir)} for the agents
    it names (the other one is exact).  mag: half-width of the relative thrust
    magnitude error, at most 1; dir: half-width of the pointing error as a
    fraction of the commanded |a| (include/satenv.h satenv_act_noise)."""
    if spec is None:
        return None

    def pair(v, who):
        try:
            mag, dire = (float(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError(f"act_noise: {who} is a pair (mag, dir) of numbers, got {v!r}") from None
        if not (math.isfinite(mag) and math.isfinite(dire) and mag >= 0.0 and dire >= 0.0):
            raise ValueError(f"act_noise: {who}'s half-widths must be finite and >= 0, got {v!r}")
        if mag > 1.0:
            raise ValueError(f"act_noise: {who}'s mag must not exceed 1 (the thrust must not flip), got {mag}")
        return mag, dire

    if isinstance(spec, dict):
        unknown = set(spec) - {"pursuer", "evader"}
        if unknown:
            raise ValueError(f"act_noise: keys are 'pursuer' and 'evader', got {sorted(map(str, unknown))}")
        return tuple(pair(spec[k], k) if k in spec else (0.0, 0.0) for k in ("pursuer", "evader"))
    both = pair(spec, "the spec")
    return both, both


OBS_NOISE_KEYS = ("bias_pos", "bias_vel", "pos", "vel")


def obs_noise_craft(c, who="the craft"):
    """One tracked craft of an obs_noise spec -> its half-widths (bias_pos,
    bias_vel, pos, vel) as floats: a pair (pos, vel) is the error redrawn at
    every track refresh, a dict names any of bias_pos, bias_vel (held for a
    whole episode), pos, vel (missing = 0).  Metres and m/s."""
    if isinstance(c, dict):
        unknown = set(c) - set(OBS_NOISE_KEYS)
        if unknown:
            raise ValueError(f"obs_noise: {who}'s keys are {', '.join(OBS_NOISE_KEYS)}, "
                             f"got {sorted(map(str, unknown))}")
        named = {k: c.get(k, 0.0) for k in OBS_NOISE_KEYS}
    else:
        try:
            pos, vel = c
        except (TypeError, ValueError):
            raise ValueError(f"obs_noise: {who} is a pair (pos, vel) or a dict, got {c!r}") from None
        named = {"bias_pos": 0.0, "bias_vel": 0.0, "pos": pos, "vel": vel}
    out = []
    for k in OBS_NOISE_KEYS:
        try:
            v = float(named[k])
        except (TypeError, ValueError):
            raise ValueError(f"obs_noise: {who}'s {k} is a number, got {named[k]!r}") from None
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"obs_noise: {who}'s {k} must be finite and >= 0, got {named[k]!r}")
        out.append(v)
    return tuple(out)


def obs_noise_spec(spec):
    """args_param.obs_noise -> (the pursuer's (bias_pos, bias_vel, pos, vel),
    the evader's, hold), or None for None.  A pair (pos, vel) holds for both
    tracked craft with hold 1; a dict {"pursuer": c, "evader": c, "hold": h}
    names the craft it perturbs (the other one is tracked exactly), c as in
    obs_noise_craft, and the number of steps h >= 1 a redrawn error is held
    (include/satenv.h satenv_obs_noise)."""
    if spec is None:
        return None
    if isinstance(spec, dict):
        unknown = set(spec) - {"pursuer", "evader", "hold"}
        if unknown:
            raise ValueError(f"obs_noise: keys are 'pursuer', 'evader' and 'hold', got {sorted(map(str, unknown))}")
        hold = spec.get("hold", 1)
        if isinstance(hold, bool) or not isinstance(hold, (int, np.integer)) or not 1 <= int(hold) < 2 ** 31:
            raise ValueError(f"obs_noise: hold is an int >= 1, got {hold!r}")
        zero = (0.0, 0.0, 0.0, 0.0)
        return tuple(obs_noise_craft(spec[k], k) if k in spec else zero for k in ("pursuer", "evader")) + (int(hold),)
    both = obs_noise_craft(spec, "the spec")
    return both, both, 1


def _num_mode(v) -> int:
    if isinstance(v, np.float32):
        return F32
    if isinstance(v, (np.floating, float)):
        return F64
    if isinstance(v, np.integer):
        return I64
    return PYINT


class Box:
    """Minimal stand-in for ``gym.spaces.Box`` (environment.py:57): shape/low/high/dtype."""

    def __init__(self, low, high, shape, dtype=np.float32):
        self.low, self.high, self.dtype = np.asarray(low), np.asarray(high), dtype
        self.shape = tuple(shape)


class Discrete:
    def __init__(self, n):
        self.n = n


def _spaces():
    # environment.py:51-62
    position_low = np.array([-500000, -500000, -500000, -10000000, -10000000, -10000000, -10000000, -10000000,
                             -10000000])
    velocity_low = np.array([-10000, -10000, -10000, -50000, -50000, -50000, -50000, -50000, -50000])
    low = np.concatenate((position_low, velocity_low))
    obs = Box(low=low, high=-low, shape=(OBS_DIM,), dtype=np.float32)
    act = np.array([[-1.6, 1.6], [-1.6, 1.6], [-1.6, 1.6]])
    return obs, act, Discrete(5)


class VecSatellites:
    """``num_envs`` reference environments stepped by one HIP kernel launch.

    Tensors are device tensors on ``device`` (actions f32 [N,3]); every call
    is asynchronous on the current torch stream.  device="cpu": the host
    build (satenv_cpu_*, synchronous, `threads` OpenMP threads, 0 = all)."""

    def __init__(self, num_envs: int, device=None, d_capture: float = 100000.0, d_range: float = 100000.0,
                 max_episode_steps: int = 1000, Flag: int = 0, fuel_c=320, fuel_t=320, threads: int = 0, **params):
        self.host = device is not None and torch.device(device).type == "cpu"
        if not self.host and not torch.cuda.is_available():
            raise _lib.NativeError("VecSatellites needs a HIP device (MI355X); the host build runs only when asked "
                                   "for with device='cpu'")
        if self.host:
            self.device = torch.device("cpu")
        else:
            self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._api = "satenv_cpu_" if self.host else "satenv_"
        self._req = require_cpu if self.host else require_cuda
        self.num_envs = int(num_envs)
        self._p = default_params(d_capture=float(d_capture), d_range=float(d_range),
                                 max_episode_steps=int(max_episode_steps), flag=int(Flag), fuel_c0=float(fuel_c),
                                 fuel_t0=float(fuel_t), fuel_c0_mode=_num_mode(fuel_c),
                                 fuel_t0_mode=_num_mode(fuel_t), **params)
        h = C.c_void_p()
        if self.host:
            check(self._fn("create")(C.byref(h), self.num_envs, C.byref(self._p), int(threads)), "satenv_cpu_create")
        else:
            with torch.cuda.device(self.device):
                check(_lib.lib().satenv_create(C.byref(h), self.num_envs, C.byref(self._p), self.device.index or 0),
                      "satenv_create")
        self._h = h
        self.observation_space, self.action_space, self.action_space_beta = _spaces()
        self.stats = torch.zeros(4, dtype=torch.float64, device=self.device)
        self.draws = False               # set_reset_dist was called: the handle launches the drawing step kernels
        self.noisy = False               # set_act_noise was called: ... the step kernels with the actuation noise
        self.measures = False            # set_obs_noise was called: ... and with the tracking errors on the rows

    def _fn(self, name):
        return getattr(_lib.lib(), self._api + name)

    def _sp(self):
        return None if self.host else stream_ptr()

    # -- parameters -----------------------------------------------------------
    def _push_params(self):
        check(self._fn("set_params")(self._h, C.byref(self._p)), self._api + "set_params")

    def set_params(self, **fields):
        """Update satenv_params fields (e.g. propagator=2) and push them."""
        for k, v in fields.items():
            if not hasattr(self._p, k):
                raise AttributeError(f"satenv_params has no field {k!r}")
            setattr(self._p, k, v)
        self._push_params()

    @property
    def d_capture(self):
        return self._p.d_capture

    @d_capture.setter
    def d_capture(self, v):          # CPPO_main.py:98 "env.d_capture = d_capture"
        self._p.d_capture = float(v)
        self._push_params()

    @property
    def max_episode_steps(self):
        return self._p.max_episode_steps

    @max_episode_steps.setter
    def max_episode_steps(self, v):
        self._p.max_episode_steps = int(v)
        self._push_params()

    @property
    def d_range(self):
        return self._p.d_range

    @d_range.setter
    def d_range(self, v):
        self._p.d_range = float(v)
        self._push_params()

    def set_step_kernel(self, kind: int = 2, wide_envs: int = 64):
        """Which step kernel the device build launches (satenv_set_step_kernel):
        2 the wide kernel (default), 1 the four-solve split kernel, 0 one lane
        per env; every one computes the same bits."""
        if self.host:
            raise _lib.NativeError("the host build has one step loop")
        check(_lib.lib().satenv_set_step_kernel(self._h, int(kind), int(wide_envs)), "satenv_set_step_kernel")

    # -- API -----------------------------------------------------------------
    def reset(self, Flag: int = 0, mask=None, obs_out=None, obs64_out=None):
        """environment.py:66-79 for all envs (or those with mask != 0). Returns obs f32 [N,18]."""
        n = self.num_envs
        if obs_out is None and obs64_out is None:
            obs_out = torch.empty((n, OBS_DIM), dtype=torch.float32, device=self.device)
        if mask is not None:
            self._req(mask, torch.uint8, (n,), "mask")
        check(self._fn("reset")(self._h, int(Flag), ptr(mask), ptr(obs_out), ptr(obs64_out), self._sp()),
              self._api + "reset")
        return obs_out if obs_out is not None else obs64_out

    def step(self, pursuer_action, escaper_action, epsiode_count=None, obs_out=None, obs64_out=None,
             reward_out=None, done_out=None):
        """environment.py:81-255 for all envs, no automatic reset.

        Returns (obs f32 [N,18] or obs64, reward f64 [N], done u8 [N])."""
        n = self.num_envs
        self._req(pursuer_action, torch.float32, (n, ACT_DIM), "pursuer_action")
        self._req(escaper_action, torch.float32, (n, ACT_DIM), "escaper_action")
        if epsiode_count is not None:
            self._req(epsiode_count, torch.int32, (n,), "epsiode_count")
        if obs_out is None and obs64_out is None:
            obs_out = torch.empty((n, OBS_DIM), dtype=torch.float32, device=self.device)
        if reward_out is None:
            reward_out = torch.empty(n, dtype=torch.float64, device=self.device)
        if done_out is None:
            done_out = torch.empty(n, dtype=torch.uint8, device=self.device)
        check(self._fn("step")(self._h, ptr(pursuer_action), ptr(escaper_action), ptr(epsiode_count), ptr(obs_out),
                               ptr(obs64_out), ptr(reward_out), ptr(done_out), self._sp()), self._api + "step")
        return (obs_out if obs_out is not None else obs64_out), reward_out, done_out

    def step_autoreset(self, pursuer_action, escaper_action, obs_out=None, reward_out=None, done_out=None,
                       stats=True):
        """One step of the CPPO_main.py:119-153 loop for all envs: device episode
        counters, done envs reset in-kernel (obs_out = post-reset obs).
        Returns (obs f32 [N,18], reward f32 [N], done u8 [N])."""
        n = self.num_envs
        if obs_out is None:
            obs_out = torch.empty((n, OBS_DIM), dtype=torch.float32, device=self.device)
        if reward_out is None:
            reward_out = torch.empty(n, dtype=torch.float32, device=self.device)
        if done_out is None:
            done_out = torch.empty(n, dtype=torch.uint8, device=self.device)
        if self.host:
            self._req(pursuer_action, torch.float32, (n, ACT_DIM), "pursuer_action")
            self._req(escaper_action, torch.float32, (n, ACT_DIM), "escaper_action")
        check(self._fn("step_autoreset")(self._h, ptr(pursuer_action), ptr(escaper_action), ptr(obs_out),
                                         ptr(reward_out), ptr(done_out), ptr(self.stats) if stats else None,
                                         self._sp()), self._api + "step_autoreset")
        return obs_out, reward_out, done_out

    def get_state(self):
        n = self.num_envs
        f = torch.empty((SATENV_F64_PLANES, n), dtype=torch.float64, device=self.device)
        i = torch.empty((SATENV_I32_PLANES, n), dtype=torch.int32, device=self.device)
        check(self._fn("get_state")(self._h, ptr(f), ptr(i), self._sp()), self._api + "get_state")
        return f, i

    def set_state(self, f64_planes=None, i32_planes=None):
        n = self.num_envs
        if f64_planes is not None:
            self._req(f64_planes, torch.float64, (SATENV_F64_PLANES, n), "f64_planes")
        if i32_planes is not None:
            self._req(i32_planes, torch.int32, (SATENV_I32_PLANES, n), "i32_planes")
        check(self._fn("set_state")(self._h, ptr(f64_planes), ptr(i32_planes), self._sp()), self._api + "set_state")

    # -- randomised episode starts (include/satenv.h satenv_reset_dist) ---------
    def _get_dist(self):
        d = _lib.SatenvResetDist()
        check(self._fn("get_reset_dist")(self._h, C.byref(d)), self._api + "get_reset_dist")
        return d

    def _set_dist(self, d):
        check(self._fn("set_reset_dist")(self._h, C.byref(d), self._sp()), self._api + "set_reset_dist")

    def set_reset_dist(self, lo, hi, seed, env_offset: int = 0):
        """From now on every reset of env i -- reset() and the autoreset inside
        step_autoreset -- starts from a point drawn uniformly from the box
        [lo, hi] (12 scalars: Pp, Pv, Ep, Ev), a function of (seed, env_offset
        + i, the env's episode index) alone.  Stream-ordered: graphs captured
        earlier see it on their next replay -- except graphs captured before
        this handle's first set_reset_dist (`draws` still False), which hold
        the step kernel without the draw and must be captured again.  There
        is no rejection: a start inside d_capture is captured on its first step."""
        d = _lib.SatenvResetDist()
        lo, hi = (np.asarray(x, dtype=np.float64).ravel() for x in (lo, hi))
        if lo.shape != (12,) or hi.shape != (12,):
            raise ValueError("lo and hi are 12 scalars each: Pp[3], Pv[3], Ep[3], Ev[3]")
        d.lo[:], d.hi[:] = lo.tolist(), hi.tolist()
        d.seed, d.env_offset, d.enabled = int(seed) & (2 ** 64 - 1), int(env_offset), 1
        self._set_dist(d)
        self.draws = True

    def clear_reset_dist(self):
        """Back to the reference's fixed reset (the episode indices keep counting)."""
        d = self._get_dist()
        d.enabled = 0
        self._set_dist(d)

    @property
    def reset_dist(self):
        """None while resets are the reference's, else a dict: lo, hi (f64 [12]), seed, env_offset."""
        d = self._get_dist()
        if not d.enabled:
            return None
        return {"lo": np.array(d.lo[:]), "hi": np.array(d.hi[:]), "seed": int(d.seed), "env_offset": int(d.env_offset)}

    # -- actuation noise (include/satenv.h satenv_act_noise) ---------------------
    def _get_noise(self):
        d = _lib.SatenvActNoise()
        check(self._fn("get_act_noise")(self._h, C.byref(d)), self._api + "get_act_noise")
        return d

    def _set_noise(self, d):
        check(self._fn("set_act_noise")(self._h, C.byref(d), self._sp()), self._api + "set_act_noise")

    def set_act_noise(self, pursuer=(0.0, 0.0), evader=(0.0, 0.0), seed=0, env_offset: int = 0):
        """From now on every step executes, for each agent, its clipped action
        with a thrust magnitude error of relative half-width mag (<= 1) and a
        pointing error of half-width dir * |a|, pursuer=(mag, dir) and
        evader=(mag, dir): a function of (seed, env_offset + i, the env's
        episode index, the step count) alone.  The caller's action tensors
        are not written.  Stream-ordered: graphs captured earlier see it on
        their next replay -- except graphs captured before this handle's first
        set_act_noise (`noisy` still False), which hold the step kernel
        without the noise and must be captured again."""
        d = _lib.SatenvActNoise()
        (d.mag[0], d.dir[0]), (d.mag[1], d.dir[1]) = ((float(x) for x in pursuer), (float(x) for x in evader))
        d.seed, d.env_offset, d.enabled = int(seed) & (2 ** 64 - 1), int(env_offset), 1
        self._set_noise(d)
        self.noisy = True

    def clear_act_noise(self):
        """Back to exact execution of every action."""
        d = self._get_noise()
        d.enabled = 0
        self._set_noise(d)

    def act_noise(self):
        """None while actions are executed exactly, else a dict: pursuer, evader
        ((mag, dir) each), seed, env_offset."""
        d = self._get_noise()
        if not d.enabled:
            return None
        return {"pursuer": (d.mag[0], d.dir[0]), "evader": (d.mag[1], d.dir[1]), "seed": int(d.seed),
                "env_offset": int(d.env_offset)}

    # -- tracking errors on the observations (include/satenv.h satenv_obs_noise) --
    def _get_obs_noise(self):
        d = _lib.SatenvObsNoise()
        check(self._fn("get_obs_noise")(self._h, C.byref(d)), self._api + "get_obs_noise")
        return d

    def _set_obs_noise(self, d):
        check(self._fn("set_obs_noise")(self._h, C.byref(d), self._sp()), self._api + "set_obs_noise")

    def set_obs_noise(self, pursuer=(0.0, 0.0), evader=(0.0, 0.0), hold: int = 1, seed=0, env_offset: int = 0):
        """From now on every f32 observation row the env writes (step,
        step_autoreset, reset) is write_obs of the MEASURED kinematics: each
        scalar of tracked craft pursuer / evader off by a bias held for the
        whole episode plus an error redrawn every `hold` steps, bounded
        uniforms of the half-widths given per craft as (pos, vel) or as a dict
        with keys among bias_pos, bias_vel, pos, vel (obs_noise_craft) -- a
        function of (seed, env_offset + i, the env's episode index, the step
        count) alone.  Both agents read the same row.  The state, rewards,
        dones, stats and obs64_out stay the truth.  Stream-ordered: graphs
        captured earlier see it on their next replay -- except graphs captured
        before this handle's first set_obs_noise (`measures` still False),
        which hold the kernels without the measurement and must be captured
        again."""
        d = _lib.SatenvObsNoise()
        for g, c in enumerate((pursuer, evader)):
            d.bias_pos[g], d.bias_vel[g], d.pos[g], d.vel[g] = obs_noise_craft(c, ("pursuer", "evader")[g])
        d.hold = int(hold)
        d.seed, d.env_offset, d.enabled = int(seed) & (2 ** 64 - 1), int(env_offset), 1
        self._set_obs_noise(d)
        self.measures = True

    def clear_obs_noise(self):
        """Back to exact observations."""
        d = self._get_obs_noise()
        d.enabled = 0
        self._set_obs_noise(d)

    def obs_noise(self):
        """None while observations are exact, else a dict: pursuer, evader (each
        a dict of bias_pos, bias_vel, pos, vel), hold, seed, env_offset."""
        d = self._get_obs_noise()
        if not d.enabled:
            return None
        craft = [{"bias_pos": d.bias_pos[g], "bias_vel": d.bias_vel[g], "pos": d.pos[g], "vel": d.vel[g]}
                 for g in (0, 1)]
        return {"pursuer": craft[0], "evader": craft[1], "hold": int(d.hold), "seed": int(d.seed),
                "env_offset": int(d.env_offset)}

    def episode_index(self):
        """int32 [N]: how many resets each env has had (0 at construction)."""
        out = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        check(self._fn("get_episode_index")(self._h, ptr(out), self._sp()), self._api + "get_episode_index")
        return out

    def set_episode_index(self, t=None):
        """Set the per-env episode indices (int32 [N]; None: zeros)."""
        if t is not None:
            self._req(t, torch.int32, (self.num_envs,), "episode index")
        check(self._fn("set_episode_index")(self._h, ptr(t), self._sp()), self._api + "set_episode_index")

    def episode_return(self):
        """float64 [N]: the running return of every env's episode in flight
        (the plane get_state leaves out; it feeds stats[1] when the episode ends)."""
        out = torch.empty(self.num_envs, dtype=torch.float64, device=self.device)
        check(self._fn("get_episode_return")(self._h, ptr(out), self._sp()), self._api + "get_episode_return")
        return out

    def set_episode_return(self, t=None):
        """Set the per-env running returns (float64 [N]; None: zeros)."""
        if t is not None:
            self._req(t, torch.float64, (self.num_envs,), "episode return")
        check(self._fn("set_episode_return")(self._h, ptr(t), self._sp()), self._api + "set_episode_return")

    # -- the whole state (satrl/checkpoint.py) -----------------------------------
    def full_state(self):
        """Everything a handle carries from one step to the next, as CPU numpy
        arrays: the 15 f64 and 3 i32 planes of get_state, the running episode
        returns, the episode indices and `stats`.  The reset distribution, the
        actuation noise and the observation noise are configuration and are
        not part of it."""
        f, i = self.get_state()
        return {"f64": f.cpu().numpy(), "i32": i.cpu().numpy(), "ep_return": self.episode_return().cpu().numpy(),
                "episode_index": self.episode_index().cpu().numpy(), "stats": self.stats.cpu().numpy().copy()}

    def load_full_state(self, d):
        """Restore full_state(), in place and stream-ordered: graphs captured
        over this handle and over `stats` stay valid."""
        n = self.num_envs
        want = {"f64": (np.float64, (SATENV_F64_PLANES, n)), "i32": (np.int32, (SATENV_I32_PLANES, n)),
                "ep_return": (np.float64, (n,)), "episode_index": (np.int32, (n,)), "stats": (np.float64, (4,))}
        t = {}
        for k, (dt, shape) in want.items():
            a = np.ascontiguousarray(d[k])
            if a.dtype != dt or a.shape != shape:
                raise ValueError(f"env state {k!r}: {a.dtype} {a.shape} for {np.dtype(dt)} {shape}")
            t[k] = torch.from_numpy(a).to(self.device)
        self.set_state(t["f64"], t["i32"])
        self.set_episode_return(t["ep_return"])
        self.set_episode_index(t["episode_index"])
        self.stats.copy_(t["stats"])

    def check_errors(self) -> int:
        st = C.c_int32(0)
        check(self._fn("check")(self._h, C.byref(st)), self._api + "check")
        return st.value

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_bits(fuel_c_mode, fuel_t_mode, vel_int, flag):
    return (int(fuel_c_mode) & 3) | ((int(fuel_t_mode) & 3) << 2) | ((int(vel_int) & 1) << 4) | ((int(flag) & 3) << 5)


def unpack_bits(b):
    b = int(b)
    return dict(fuel_c_mode=b & 3, fuel_t_mode=(b >> 2) & 3, vel_int=(b >> 4) & 1, flag=(b >> 5) & 3)


def _typed(v, mode):
    return [int(v), np.int64(v), np.float32(v), np.float64(v)][mode]


class satellites:  # noqa: N801  (reference class name)
    """Drop-in for ``environment.satellites`` (environment.py:8), Flag 0/1/2.

    Same keywords as environment.py:26-28; ``args.max_episode_steps`` is
    required as in environment.py:46.  State lives on the GPU; the public
    attributes are read back on access.  Flag 2 (environment.py:257-315):
    the kernel steps the state (no danger-zone update, reward 0), the
    ellipse_params come from the reachable-domain grid and ellipse-fit
    kernels (satrl.reachable), and the env's network_method_train takes its
    step on the CPU like the reference's.
    """

    def __init__(self, Pursuer_position=np.array([2000, 2000, 1000]), Pursuer_vector=np.array([1.71, 1.14, 1.3]),
                 Escaper_position=np.array([1000, 2000, 0]), Escaper_vector=np.array([1.71, 1.14, 1.3]),
                 M=0.4, dis_safe=1000, d_capture=100000, Flag=0, fuel_c=320, fuel_t=320, d_range=100000,
                 args=None, device=None):
        max_ep = args.max_episode_steps          # AttributeError on args=None, as environment.py:46
        kin = np.concatenate([np.asarray(Pursuer_position, np.float64), np.asarray(Pursuer_vector, np.float64),
                              np.asarray(Escaper_position, np.float64), np.asarray(Escaper_vector, np.float64)])
        self._v = VecSatellites(1, device=device, d_capture=d_capture, d_range=d_range, max_episode_steps=max_ep,
                                Flag=Flag, fuel_c=fuel_c, fuel_t=fuel_t, init_kin=kin)
        self.dis_dafe = dis_safe
        self.M = M
        self.burn_reward = 0
        self.win_reward = 100
        self.ellipse_params = []
        self.observation_space, self.action_space, self.action_space_beta = _spaces()
        # environment.py:49 builds the ellipse-fitting trainer, whose ImprovedNN()
        # (real_time_data_process.py:129) draws its default init from torch's
        # global CPU generator: draw the same numbers, so agents constructed
        # after a seeded env get the reference's weights
        from .surrogate import network_method_train
        self.trian_elliptical_fitting = network_method_train(pretrain=False,
                                                             save_dir=getattr(args, "ellipse_save_dir", None))
        dev = self._v.device
        self._pa = torch.empty((1, ACT_DIM), dtype=torch.float32, device=dev)
        self._ea = torch.empty((1, ACT_DIM), dtype=torch.float32, device=dev)
        self._cnt = torch.empty(1, dtype=torch.int32, device=dev)
        self._obs = torch.empty((1, OBS_DIM), dtype=torch.float64, device=dev)
        self._r = torch.empty(1, dtype=torch.float64, device=dev)
        self._d = torch.empty(1, dtype=torch.uint8, device=dev)

    # reference attributes ------------------------------------------------------
    d_capture = property(lambda s: s._v.d_capture, lambda s, v: setattr(s._v, "d_capture", v))
    d_range = property(lambda s: s._v.d_range, lambda s, v: setattr(s._v, "d_range", v))
    max_episode_steps = property(lambda s: s._v.max_episode_steps,
                                 lambda s, v: setattr(s._v, "max_episode_steps", v))

    def _state(self):
        f, i = self._v.get_state()
        return f[:, 0].cpu().numpy(), i[:, 0].cpu().numpy()

    def _set(self, fi=None, ii=None):
        f, i = self._v.get_state()
        if fi:
            for k, v in fi.items():
                f[k, 0] = v
        if ii:
            for k, v in ii.items():
                i[k, 0] = v
        self._v.set_state(f, i)

    def _kin(self, lo):
        f, i = self._state()
        vel_int = unpack_bits(i[2])["vel_int"]
        arr = f[lo:lo + 3].copy()
        return arr.astype(np.int64) if vel_int else arr

    Pursuer_position = property(lambda s: s._kin(0))
    Pursuer_vector = property(lambda s: s._kin(3))
    Escaper_position = property(lambda s: s._kin(6))
    Escaper_vector = property(lambda s: s._kin(9))

    @property
    def fuel_c(self):
        f, i = self._state()
        return _typed(f[12], unpack_bits(i[2])["fuel_c_mode"])

    @fuel_c.setter
    def fuel_c(self, v):
        f, i = self._v.get_state()
        b = unpack_bits(int(i[2, 0]))
        f[12, 0] = float(v)
        i[2, 0] = pack_bits(_num_mode(v), b["fuel_t_mode"], b["vel_int"], b["flag"])
        self._v.set_state(f, i)

    @property
    def fuel_t(self):
        f, i = self._state()
        return _typed(f[13], unpack_bits(i[2])["fuel_t_mode"])

    @property
    def dis(self):
        return float(self._state()[0][14])

    @property
    def dangerous_zone(self):
        return int(self._state()[1][0])

    @property
    def Flag(self):
        return unpack_bits(self._state()[1][2])["flag"]

    # API ------------------------------------------------------------------------
    def reset(self, Flag):
        """environment.py:66-79: returns the int64 observation."""
        if Flag not in (0, 1, 2):
            raise ValueError(f"Flag must be 0, 1 or 2 (environment.py:36), got {Flag!r}")
        self._v.reset(Flag, obs64_out=self._obs)
        return self._obs[0].cpu().numpy().astype(np.int64)

    def step(self, pursuer_action, escaper_action, epsiode_count):
        """environment.py:81-255.  Actions are taken as float32 (the dtype
        PPO_continuous.choose_action returns)."""
        self._pa.copy_(torch.as_tensor(np.asarray(pursuer_action, dtype=np.float32).reshape(1, ACT_DIM)))
        self._ea.copy_(torch.as_tensor(np.asarray(escaper_action, dtype=np.float32).reshape(1, ACT_DIM)))
        self._cnt.fill_(int(epsiode_count))
        self._v.step(self._pa, self._ea, self._cnt, obs_out=None, obs64_out=self._obs, reward_out=self._r,
                     done_out=self._d)
        obs = self._obs[0].cpu().numpy().copy()      # a fresh array per step (on device="cpu" .cpu() aliases)
        r = float(self._r.item())
        done = bool(self._d.item())
        if done:
            r = int(r)          # terminal rewards are python ints in the reference
        if self.Flag == 2:
            self._flag2_fit()
            r = 0               # environment.py:298-315 return the literal 0
        return obs, r, done

    def _flag2_fit(self):
        """environment.py:293-301: ellipse_params = numerical_method_process(
        R0_c, V0_c, fuel_c) on the GPU grid + fit kernels, then one step of
        the env's ellipse-fitting network."""
        from . import reachable as RD
        if self._v.host:
            raise _lib.NativeError("Flag 2's reachable-domain grid and ellipse fit run on the GPU kernels; the host "
                                   "build steps Flag 0/1 only")
        orbits, status = RD.env_orbits(self._v)
        if int(status.item()) != 0:
            # real_time_data_process.py:109 -> RD_single_pulse.py:32 indexes data[5] of a 4/5-element list
            raise IndexError("list index out of range (the pursuer's orbit has no 6-element set, "
                             f"satenv code {int(status.item())})")
        ell, _ = RD.reachable_ellipses(orbits, RD.params["N1"], RD.params["N2"], RD.params["N3"])
        self.ellipse_params = ell[0].cpu().numpy()
        R0_c, V0_c = self.relative_state_to_absolute_state(self.Pursuer_position, self.Pursuer_vector)
        self.trian_elliptical_fitting.train(R0_c, V0_c, self.fuel_c, self.ellipse_params)

    @staticmethod
    def relative_state_to_absolute_state(R0, V0):
        """environment.py:334-343."""
        assert isinstance(R0, np.ndarray) and isinstance(V0, np.ndarray)
        return np.array([27098000, 32306000, 0]) + R0, np.array([-2350, 1970, 0]) + V0
