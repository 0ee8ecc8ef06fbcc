"""Policy evaluation of the vectorised engine.

``VecEvaluator`` runs the trainer's two policies on an env handle of its own
and records, for every env, the FIRST episode after a fresh start: return,
length, outcome (captured / timed out), final and closest distance and the
commanded delta-v of both craft.  It is the vectorised counterpart of the
reference's ``PPO_continuous.evaluate`` (the mean action,
ppo_continuous.py:168-174) and ``test_network`` (one episode on a fresh env,
CPPO_main.py:233-282).

One step is [obs_normalize (with obs_norm)] -> satrl_policy_eval ->
satenv_step without autoreset -> satrl_episode_record, captured in hipGraph
chunks like the training rollout.  Envs whose episode is over go on being
stepped and are ignored by the record; the host reads the count of running
envs once per chunk and stops at 0.

Nothing of the trainer is written: not its env, buffers, step counters,
generators, learners or running statistics (the observation statistics are
read).  Under data parallelism every rank evaluates its own envs, with the
global env id (trainer.env_offset + i) in the noise key; reducing the
results across ranks is left to the caller.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import norm as _norm
from .env import OBS_NOISE_KEYS, VecSatellites, _typed, act_noise_spec, obs_noise_spec
from .ppo import REC_F64, REC_I32, episode_record, episode_record_reset, policy_eval, policy_eval_scripted
from .scripted import ScriptedLaw

# the default noise seed of an evaluation is args.seed ^ EVAL_SEED_XOR: another
# Philox key than the training rollout's, the same one on every call
EVAL_SEED_XOR = 0x5EEDE7A1
AGENTS = ("pursuer", "evader")
STREAMS = ("policy_input", "obs", "obs64", "pursuer_action", "evader_action", "reward", "done")


def det_mask_of(deterministic, flag):
    """Bit a (0 pursuer, 1 evader) set: agent a acts with its mean."""
    learner = 1 << (0 if flag == 0 else 1)
    if isinstance(deterministic, str):
        named = {"learner": learner, "both": 3, "none": 0, "pursuer": 1, "evader": 2}
        if deterministic not in named:
            raise ValueError(f"deterministic must be 'learner', 'both', 'none' or a set of {AGENTS}, "
                             f"got {deterministic!r}")
        return named[deterministic]
    mask = 0
    for a in deterministic:
        if a not in AGENTS:
            raise ValueError(f"deterministic names agents {AGENTS}, got {a!r}")
        mask |= 1 << AGENTS.index(a)
    return mask


def capture_reward_of(params, flag):
    """The terminal reward literal of a capture under `flag` (the env writes a
    capture's and a timeout's reward as exact literals, so reward ==
    capture_reward on a done step classifies the episode exactly)."""
    if flag == 0:
        cap, out = float(params.win_reward), float(params.burn_reward)
    elif flag == 1:
        cap, out = -150.0, float(params.win_reward)
    else:
        raise ValueError("evaluation runs under Flag 0 (pursuer learns) or Flag 1 (evader learns)")
    if cap == out:
        raise ValueError(f"Flag {flag}: a capture and a timeout both pay {cap}; the outcome cannot be told from "
                         "the terminal reward")
    return cap


def _env_like(env, num_envs):
    """A fresh handle of num_envs envs with env's satenv_params."""
    p = env._p
    arrays = {k: list(getattr(p, k)) for k in ("R_cw", "V_cw", "stm", "init_kin")}
    scalars = {k: getattr(p, k) for k in ("win_reward", "burn_reward", "mu", "cw_omega", "propagator", "rk4_substeps")}
    return VecSatellites(num_envs, device=env.device, d_capture=p.d_capture, d_range=p.d_range,
                         max_episode_steps=p.max_episode_steps, Flag=p.flag, fuel_c=_typed(p.fuel_c0, p.fuel_c0_mode),
                         fuel_t=_typed(p.fuel_t0, p.fuel_t0_mode), **arrays, **scalars)


class EvalResult:
    """Per-env records of one evaluation (device tensors, [num_envs]):
    ``ret`` (f64 sum of rewards in step order), ``final_dis``, ``min_dis``,
    ``dv_p``, ``dv_e`` (f64), ``length``, ``outcome`` (i32; 0 still running
    when the evaluation stopped, 1 captured, 2 timed out).  ``steps``: the
    env steps run.  ``streams`` (record=True): the per-step tensors
    [steps, num_envs, ...] named in STREAMS -- ``obs`` / ``obs64`` / ``reward``
    / ``done`` are step t's outputs, ``policy_input`` and the actions its
    inputs.  ``start`` (f64 [12, num_envs]): the kinematics Pp Pv Ep Ev each
    recorded episode began from."""

    def __init__(self, rec_f64, rec_i32, steps, flag, det_mask, seed, streams=None, start=None):
        for k, name in enumerate(REC_F64):
            setattr(self, name, rec_f64[k])
        for k, name in enumerate(REC_I32):
            setattr(self, name, rec_i32[k])
        self.steps, self.flag, self.det_mask, self.seed, self.streams = steps, flag, det_mask, seed, streams
        self.start = start

    def summary(self):
        """Host statistics.  ``episodes``: finished episodes, ``unfinished``:
        envs still running when the evaluation stopped (max_steps); every
        other entry is over the finished episodes only (NaN when there are
        none): ``capture_rate``, ``mean_return``, ``std_return`` (population
        std), ``mean_length``, ``mean_final_dis``, ``mean_min_dis``."""
        outcome = self.outcome.cpu().numpy()
        fin = outcome != 0
        n = int(fin.sum())

        def mean(t):
            return float(t.cpu().numpy()[fin].astype(np.float64).mean()) if n else float("nan")

        return {"episodes": n, "unfinished": int(outcome.size - n),
                "capture_rate": float((outcome == 1).sum()) / n if n else float("nan"),
                "mean_return": mean(self.ret),
                "std_return": float(self.ret.cpu().numpy()[fin].std()) if n else float("nan"),
                "mean_length": mean(self.length), "mean_final_dis": mean(self.final_dis),
                "mean_min_dis": mean(self.min_dis)}


class VecEvaluator:
    """Evaluation of ``trainer``'s policies on ``num_envs`` envs of its own
    (default: the trainer's N) with the trainer's env parameters.  ``seed``
    keys the sampling agents' noise (default args.seed ^ EVAL_SEED_XOR) and,
    where the trainer's env draws randomised starts, the evaluator's draws
    from the same box; likewise the actuation noise (evaluate(act_noise=...))
    and the observation noise (evaluate(obs_noise=...))."""

    MAX_GRAPHS = 16

    def __init__(self, trainer, num_envs=None, seed=None):
        tr = self.trainer = trainer
        self.N = int(tr.N if num_envs is None else num_envs)
        self.seed = int(tr.seed ^ EVAL_SEED_XOR if seed is None else seed)
        self.device = dev = tr.device
        self.env = _env_like(tr.env, self.N)
        self._state0 = self.env.get_state()              # as the constructor leaves it: fuel 320, dis = inf
        N = self.N
        self.obs_raw = torch.zeros((N, 18), dtype=torch.float32, device=dev)
        self.policy_input = torch.zeros((N, 18), dtype=torch.float32, device=dev) if tr.obs_norm else self.obs_raw
        self.obs64 = torch.zeros((N, 18), dtype=torch.float64, device=dev)
        self.pa = torch.zeros((N, 3), dtype=torch.float32, device=dev)
        self.ea = torch.zeros((N, 3), dtype=torch.float32, device=dev)
        self.rew = torch.zeros(N, dtype=torch.float64, device=dev)
        self.done = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.rec_f64 = torch.zeros((len(REC_F64), N), dtype=torch.float64, device=dev)
        self.rec_i32 = torch.zeros((len(REC_I32), N), dtype=torch.int32, device=dev)
        self.alive = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step_base = torch.zeros(1, dtype=torch.int64, device=dev)   # the evaluator's own Philox step offset
        self._no_mask = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._chunk_streams = None
        self._graphs = {}
        self._laws = {}
        self._pool = None
        self._warm = False

    # -- one step -------------------------------------------------------------------------
    def _step(self, k, det_mask, seed, cap, rec=None, opponent=None):
        """Step k of a chunk (Philox step k + *step_base); rec: the chunk's stream buffers;
        opponent: the frozen agent's pool slot that acts in its place (None: its live parameters)."""
        tr = self.trainer
        P0, P1 = tr.pursuer.P, tr.evader.P
        if isinstance(opponent, ScriptedLaw):    # the frozen agent's law on the raw row, the learner's MLP alone
            if tr.obs_norm:
                _norm.obs_normalize(self.obs_raw, tr.obs_stats, tr.obs_clip, self.policy_input)
            learner_act, law_act = (self.pa, self.ea) if tr.flag == 0 else (self.ea, self.pa)
            policy_eval_scripted(tr.learner.H, self.policy_input, self.obs_raw, tr.learner.P, tr.flag, 1.6,
                                 (det_mask >> tr.flag) & 1, seed, tr.env_offset, k, learner_act, opponent, law_act,
                                 step_base=self.step_base)
            self._after_policy(k, cap, rec)
            return
        if opponent is not None:
            if tr.flag == 0:
                P1 = tr.pools["evader"].slot(opponent)
            else:
                P0 = tr.pools["pursuer"].slot(opponent)
        if tr.obs_norm:                          # the trainer's current statistics, read only
            _norm.obs_normalize(self.obs_raw, tr.obs_stats, tr.obs_clip, self.policy_input)
        policy_eval(tr.pursuer.H, self.policy_input, P0, P1, 1.6, det_mask, seed, tr.env_offset, k,
                    self.pa, self.ea, step_base=self.step_base)
        self._after_policy(k, cap, rec)

    def _after_policy(self, k, cap, rec):
        """The rest of step k once both actions are in pa / ea: env step and record."""
        if rec is not None:
            rec["policy_input"][k].copy_(self.policy_input)
            rec["pursuer_action"][k].copy_(self.pa)
            rec["evader_action"][k].copy_(self.ea)
        self.env.step(self.pa, self.ea, None, obs_out=self.obs_raw, obs64_out=self.obs64, reward_out=self.rew,
                      done_out=self.done)
        episode_record(self.rew, self.done, self.obs64, self.pa, self.ea, cap, self.rec_f64, self.rec_i32, self.alive)
        if rec is not None:
            rec["obs"][k].copy_(self.obs_raw)
            rec["obs64"][k].copy_(self.obs64)
            rec["reward"][k].copy_(self.rew)
            rec["done"][k].copy_(self.done)

    def _stream_buffers(self, steps):
        N, dev = self.N, self.device
        shapes = {"policy_input": ((18,), torch.float32), "obs": ((18,), torch.float32), "obs64": ((18,), torch.float64),
                  "pursuer_action": ((3,), torch.float32), "evader_action": ((3,), torch.float32),
                  "reward": ((), torch.float64), "done": ((), torch.uint8)}
        return {k: torch.zeros((steps, N) + s, dtype=dt, device=dev) for k, (s, dt) in shapes.items()}

    def _graph(self, n, flag, det_mask, seed, cap, rec, opponent=None):
        """The captured chunk of n steps.  The env parameters, the noise seed
        and the opponent slot's pointer (a scripted law's block: the law's
        identity, not its values, which the kernel reads at every launch) are
        launch arguments, so they are part of the key."""
        okey = ("law", id(opponent)) if isinstance(opponent, ScriptedLaw) else opponent
        key = (flag, n, det_mask, seed, rec is not None, bytes(self.env._p), okey)
        if key not in self._graphs:
            if len(self._graphs) >= self.MAX_GRAPHS:
                self._graphs.clear()
                self._laws.clear()
            if isinstance(opponent, ScriptedLaw):
                self._laws[id(opponent)] = opponent          # keeps the block (and the id) alive with its graphs
            s = torch.cuda.Stream(device=self.device)
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            with torch.cuda.graph(g, pool=self._pool, stream=s):
                for k in range(n):
                    self._step(k, det_mask, seed, cap, rec, opponent)
            self._graphs[key] = g
        return self._graphs[key]

    # -- one evaluation -------------------------------------------------------------------
    def evaluate(self, deterministic="learner", max_steps=None, states=None, seed=None, record=False, opponent=None,
                 act_noise="inherit", obs_noise="inherit"):
        tr = self.trainer
        if isinstance(obs_noise, str):
            if obs_noise != "inherit":
                raise ValueError(f"obs_noise is 'inherit', None or a spec (args_param obs_noise), got {obs_noise!r}")
            now = tr.env.obs_noise()             # the trainer's half-widths and hold as they are now
            track = None if now is None else obs_noise_spec({k: now[k] for k in ("pursuer", "evader", "hold")})
        else:
            track = obs_noise_spec(obs_noise)
        if isinstance(act_noise, str):
            if act_noise != "inherit":
                raise ValueError(f"act_noise is 'inherit', None or a spec (args_param act_noise), got {act_noise!r}")
            now = tr.env.act_noise()             # the trainer's half-widths as they are now
            noise = None if now is None else (now["pursuer"], now["evader"])
        else:
            noise = act_noise_spec(act_noise)
        flag = int(tr.flag)
        det_mask = det_mask_of(deterministic, flag)
        seed = self.seed if seed is None else int(seed)
        env = self.env
        # the trainer's env parameters as they are now
        C.memmove(C.byref(env._p), C.byref(tr.env._p), C.sizeof(env._p))
        env._push_params()
        cap = capture_reward_of(env._p, flag)
        max_steps = int(env.max_episode_steps if max_steps is None else max_steps)
        if max_steps <= 0:
            raise ValueError("max_steps must be positive")
        use_graphs = bool(tr.use_graphs)
        chunk = max(1, min(int(tr.args.rollout_graph_chunk), max_steps))
        with torch.cuda.device(self.device):
            if use_graphs and not self._warm:
                # one eager step so that lazy initialisation happens before the first capture
                # (the state is set below)
                self._step(0, det_mask, seed, cap)
                torch.cuda.synchronize()
                self._warm = True
            # the trainer's reset box as it is now, under the evaluation seed and from episode index
            # 0: the same scenarios on every call
            box = tr.env.reset_dist
            if box is None:
                env.clear_reset_dist()
            else:
                env.set_reset_dist(box["lo"], box["hi"], seed, env_offset=tr.env_offset)
            # the actuation noise under the evaluation seed too: the same errors on every call
            if noise is None:
                env.clear_act_noise()
            else:
                if not env.noisy:                # this handle's first noise: its graphs hold the step kernel without it
                    self._graphs.clear()
                    self._laws.clear()
                env.set_act_noise(noise[0], noise[1], seed, env_offset=tr.env_offset)
            # ... and the observation noise, before the reset below writes the first row
            if track is None:
                env.clear_obs_noise()
            else:
                if not env.measures:             # likewise: its graphs hold the step kernel without the measurement
                    self._graphs.clear()
                    self._laws.clear()
                env.set_obs_noise(*(dict(zip(OBS_NOISE_KEYS, c)) for c in track[:2]), hold=track[2], seed=seed,
                                  env_offset=tr.env_offset)
            env.set_episode_index(None)
            if states is None:
                env.set_state(*self._state0)
                env.reset(flag, obs_out=self.obs_raw)
            else:
                env.set_state(*states)           # the caller's scenarios: no reset, the obs of the state as it is
                env.reset(flag, mask=self._no_mask, obs_out=self.obs_raw)
            start = env.get_state()[0][:12].clone()
            episode_record_reset(self.rec_f64, self.rec_i32, self.alive)
            rec = None
            out = self._stream_buffers(max_steps) if record else None
            if record:
                if self._chunk_streams is None or self._chunk_streams["done"].shape[0] < chunk:
                    self._chunk_streams = self._stream_buffers(chunk)
                    self._graphs = {k: g for k, g in self._graphs.items() if not k[4]}
                rec = self._chunk_streams
            t = 0
            while t < max_steps:
                n = min(chunk, max_steps - t)
                self.step_base.fill_(t)
                if use_graphs:
                    self._graph(n, flag, det_mask, seed, cap, rec, opponent).replay()
                else:
                    for k in range(n):
                        self._step(k, det_mask, seed, cap, rec, opponent)
                if record:
                    for name in STREAMS:
                        out[name][t:t + n].copy_(rec[name][:n])
                t += n
                if int(self.alive.item()) == 0:  # the one host read per chunk
                    break
            if record:
                out = {k: v[:t] for k, v in out.items()}
            return EvalResult(self.rec_f64.clone(), self.rec_i32.clone(), t, flag, det_mask, seed, out, start)
