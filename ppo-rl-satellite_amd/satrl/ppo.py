"""Gaussian PPO on PyTorch-ROCm + HIP rollout kernels.

Reference: qiaobeibei/PPO-RL-Satellite ppo_continuous.py.
  * ``Actor_Gaussian`` / ``Critic``       ppo_continuous.py:61-134 (same layer
    names, init, activations and checkpoint file names)
  * ``PPO_continuous``                     ppo_continuous.py:136-258, drop-in:
    choose_action / evaluate / update / lr_decay / save / load_checkpoint
  * ``PPOLearner``                          the batched engine used by the
    vectorised trainer: HIP Gaussian sampling, HIP GAE scan, and a
    hipGraph-captured minibatch step (actor and critic losses, backward,
    grad-norm clip, Adam) replayed over device-resident permutations.

The ``Actor_Beta`` policy (ppo_continuous.py:14-59) is outside the hot path
(policy_dist defaults to "Gaussian", CPPO_main.py:17).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import dist as _dist
from . import rccl as _rccl
from ._lib import check, ptr, stream_ptr

LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))
ENT_CONST = 0.5 + 0.5 * math.log(2 * math.pi)


def orthogonal_init(layer, gain=1.0):
    """ppo_continuous.py:10-12."""
    nn.init.orthogonal_(layer.weight, gain=gain)
    nn.init.constant_(layer.bias, 0)


class Actor_Gaussian(nn.Module):  # noqa: N801
    """ppo_continuous.py:61-101."""

    def __init__(self, args, agent_idx):
        super().__init__()
        self.agent_name = "agent_%s" % agent_idx
        self.chkpt_file = os.path.join(args.chkpt_dir, self.agent_name + "_actor_Gaussian")
        self.max_action = args.max_action
        self.fc1 = nn.Linear(args.state_dim, args.hidden_width)
        self.fc2 = nn.Linear(args.hidden_width, args.hidden_width)
        self.mean_layer = nn.Linear(args.hidden_width, args.action_dim)
        self.log_std = nn.Parameter(torch.zeros(1, args.action_dim))
        self.activate_func = [nn.ReLU(), nn.Tanh()][args.use_tanh]
        if args.use_orthogonal_init:
            orthogonal_init(self.fc1)
            orthogonal_init(self.fc2)
            orthogonal_init(self.mean_layer, gain=0.01)

    def forward(self, s):
        s = self.activate_func(self.fc1(s))
        s = self.activate_func(self.fc2(s))
        return self.max_action * torch.tanh(self.mean_layer(s))

    def get_dist(self, s):
        mean = self.forward(s)
        std = torch.exp(self.log_std.expand_as(mean))
        return torch.distributions.Normal(mean, std, validate_args=False)

    def save_checkpoint(self):
        torch.save({k: v.detach().cpu().clone() for k, v in self.state_dict().items()}, self.chkpt_file)

    def load_checkpoint(self):
        self.load_state_dict(torch.load(self.chkpt_file, weights_only=True, map_location="cpu"))


class Critic(nn.Module):
    """ppo_continuous.py:103-134."""

    def __init__(self, args, agent_idx):
        super().__init__()
        self.agent_name = "agent_%s" % agent_idx
        self.chkpt_file = os.path.join(args.chkpt_dir, self.agent_name + "_critic")
        self.fc1 = nn.Linear(args.state_dim, args.hidden_width)
        self.fc2 = nn.Linear(args.hidden_width, args.hidden_width)
        self.fc3 = nn.Linear(args.hidden_width, 1)
        self.activate_func = [nn.ReLU(), nn.Tanh()][args.use_tanh]
        if args.use_orthogonal_init:
            orthogonal_init(self.fc1)
            orthogonal_init(self.fc2)
            orthogonal_init(self.fc3)

    def forward(self, s):
        s = self.activate_func(self.fc1(s))
        s = self.activate_func(self.fc2(s))
        return self.fc3(s)

    def save_checkpoint(self):
        torch.save({k: v.detach().cpu().clone() for k, v in self.state_dict().items()}, self.chkpt_file)

    def load_checkpoint(self):
        self.load_state_dict(torch.load(self.chkpt_file, weights_only=True, map_location="cpu"))


# ---------------------------------------------------------------------------
# HIP kernels (include/satrl_rollout.h)
# ---------------------------------------------------------------------------
def gae(rew, done, values, gamma, lamda, adv_out=None, vt_out=None):
    """ppo_continuous.py:198-208 as a per-env reverse scan.

    rew f32 [T,N], done u8 [T,N], values f32 [T+1,N] -> adv, v_target f32 [T,N].
    A flat reference buffer of B transitions is the case N = 1."""
    T, N = rew.shape
    _lib.require_cuda(rew, torch.float32, (T, N), "rew")
    _lib.require_cuda(done, torch.uint8, (T, N), "done")
    _lib.require_cuda(values, torch.float32, (T + 1, N), "values")
    adv_out = torch.empty_like(rew) if adv_out is None else adv_out
    vt_out = torch.empty_like(rew) if vt_out is None else vt_out
    check(_lib.lib().satrl_gae(T, N, ptr(rew), ptr(done), ptr(values), float(gamma), float(lamda), ptr(adv_out),
                               ptr(vt_out), stream_ptr()), "satrl_gae")
    return adv_out, vt_out


def gaussian_sample(mean, log_std, max_action, seed, agent, env_offset, step, act_out=None, logp_out=None,
                    step_base=None):
    """choose_action (ppo_continuous.py:184-188) for a batch, counter-based RNG."""
    N = mean.shape[0]
    _lib.require_cuda(mean, torch.float32, (N, 3), "mean")
    log_std = log_std.reshape(-1)
    _lib.require_cuda(log_std, torch.float32, (3,), "log_std")
    act_out = torch.empty_like(mean) if act_out is None else act_out
    logp_out = torch.empty_like(mean) if logp_out is None else logp_out
    check(_lib.lib().satrl_gaussian_sample(N, ptr(mean), ptr(log_std), float(max_action), int(seed) & (2**64 - 1),
                                           int(agent), int(env_offset), int(step), ptr(step_base), ptr(act_out),
                                           ptr(logp_out), stream_ptr()), "satrl_gaussian_sample")
    return act_out, logp_out


def policy_act(H, obs, P0, P1, max_action, seed, env_offset, step, act0, logp0, act1=None, logp1=None,
               step_base=None):
    """Both agents' choose_action for a batch of observations on the fused
    MLP kernel (satrl_policy_act): P0/P1 are the pursuer's / evader's flat
    parameter buffers (PPOLearner.P), agent ids 0 / 1 in the noise key."""
    N = obs.shape[0]
    _lib.require_cuda(obs, torch.float32, (N, 18), "obs")
    for t, nm in ((act0, "act0"), (logp0, "logp0")) + (((act1, "act1"), (logp1, "logp1")) if P1 is not None else ()):
        _lib.require_cuda(t, torch.float32, (N, 3), nm)
    check(_lib.lib().satrl_policy_act(int(H), N, ptr(obs), ptr(P0), ptr(P1), float(max_action),
                                      int(seed) & (2**64 - 1), int(env_offset), int(step), ptr(step_base), ptr(act0),
                                      ptr(logp0), ptr(act1), ptr(logp1), stream_ptr()), "satrl_policy_act")


def policy_act_pool(H, obs, P0, P1, max_action, seed, env_offset, step, act0, logp0, act1, logp1, pool_agent, pool,
                    member, step_base=None):
    """policy_act with an opponent pool (satrl_policy_act_pool): agent
    pool_agent (0 | 1) acts, per 32-row block b, with row member[b] of pool
    f32 [K, stride] where 0 <= member[b] < K, and with its live parameters for
    every other value.  pool and member (i32 [ceil(N / 32)], device) are read
    at every launch."""
    N = obs.shape[0]
    _lib.require_cuda(obs, torch.float32, (N, 18), "obs")
    for t, nm in ((act0, "act0"), (logp0, "logp0"), (act1, "act1"), (logp1, "logp1")):
        _lib.require_cuda(t, torch.float32, (N, 3), nm)
    if pool.dim() != 2:
        raise ValueError(f"pool must be [K, stride], got {tuple(pool.shape)}")
    K, stride = pool.shape
    _lib.require_cuda(pool, torch.float32, (K, stride), "pool")
    _lib.require_cuda(member, torch.int32, ((N + 31) // 32,), "member")
    check(_lib.lib().satrl_policy_act_pool(int(H), N, ptr(obs), ptr(P0), ptr(P1), float(max_action),
                                           int(seed) & (2**64 - 1), int(env_offset), int(step), ptr(step_base),
                                           ptr(act0), ptr(logp0), ptr(act1), ptr(logp1), int(pool_agent), ptr(pool),
                                           int(stride), int(K), ptr(member), stream_ptr()), "satrl_policy_act_pool")


def policy_act_league(H, obs, obs_law, P0, P1, max_action, seed, env_offset, step, act0, logp0, act1, logp1,
                      pool_agent, pool, member, laws, J=None, step_base=None):
    """policy_act_pool with a law table (satrl_policy_act_league): block b of
    agent pool_agent acts with row member[b] of pool where 0 <= member[b] < K,
    with law member[b] - K of `laws` (f64 [rows >= J, 58] on the device, a
    satrl.scripted.LawTable's storage; J defaults to its rows) over the raw
    observation obs_law where K <= member[b] < K + J, writing +0.0 log-probs,
    and with its live parameters for every other value.  pool, member and laws
    are read at every launch."""
    N = obs.shape[0]
    _lib.require_cuda(obs, torch.float32, (N, 18), "obs")
    _lib.require_cuda(obs_law, torch.float32, (N, 18), "obs_law")
    for t, nm in ((act0, "act0"), (logp0, "logp0"), (act1, "act1"), (logp1, "logp1")):
        _lib.require_cuda(t, torch.float32, (N, 3), nm)
    if pool.dim() != 2:
        raise ValueError(f"pool must be [K, stride], got {tuple(pool.shape)}")
    K, stride = pool.shape
    _lib.require_cuda(pool, torch.float32, (K, stride), "pool")
    _lib.require_cuda(member, torch.int32, ((N + 31) // 32,), "member")
    if not torch.is_tensor(laws):
        laws = laws.storage                                # a LawTable
    if laws.dim() != 2:
        raise ValueError(f"laws must be [J, 58], got {tuple(laws.shape)}")
    _lib.require_cuda(laws, torch.float64, (laws.shape[0], 58), "laws")
    J = laws.shape[0] if J is None else int(J)
    if J > laws.shape[0]:
        raise ValueError(f"J = {J} laws of a table of {laws.shape[0]} rows")
    check(_lib.lib().satrl_policy_act_league(int(H), N, ptr(obs), ptr(P0), ptr(P1), float(max_action),
                                             int(seed) & (2**64 - 1), int(env_offset), int(step), ptr(step_base),
                                             ptr(act0), ptr(logp0), ptr(act1), ptr(logp1), int(pool_agent), ptr(pool),
                                             int(stride), int(K), ptr(member), ptr(obs_law), ptr(laws), J,
                                             stream_ptr()), "satrl_policy_act_league")


def _law_block(law, device):
    """The device block (f64 [58]) of a satrl.scripted.ScriptedLaw, or the tensor itself."""
    blk = law.block(device) if hasattr(law, "block") else law
    return _lib.require_cuda(blk, torch.float64, (58,), "law")


def policy_act_scripted(H, obs, obs_law, P, agent, max_action, seed, env_offset, step, act, logp, law, act_scripted,
                        step_base=None):
    """policy_act for one learning agent against a scripted one
    (satrl_policy_act_scripted): agent `agent` (0 | 1) acts with P on obs, bit
    for bit its rows of policy_act; the other agent's actions act_scripted are
    `law` (a ScriptedLaw or its device block, read at every launch) over the
    raw observation obs_law, which may be obs."""
    N = obs.shape[0]
    _lib.require_cuda(obs, torch.float32, (N, 18), "obs")
    _lib.require_cuda(obs_law, torch.float32, (N, 18), "obs_law")
    for t, nm in ((act, "act"), (logp, "logp"), (act_scripted, "act_scripted")):
        _lib.require_cuda(t, torch.float32, (N, 3), nm)
    if agent not in (0, 1):
        raise ValueError(f"agent is 0 (pursuer) or 1 (evader), got {agent!r}")
    check(_lib.lib().satrl_policy_act_scripted(int(H), N, ptr(obs), ptr(obs_law), ptr(P), int(agent),
                                               float(max_action), int(seed) & (2**64 - 1), int(env_offset), int(step),
                                               ptr(step_base), ptr(act), ptr(logp), ptr(_law_block(law, obs.device)),
                                               ptr(act_scripted), stream_ptr()), "satrl_policy_act_scripted")


def policy_eval_scripted(H, obs, obs_law, P, agent, max_action, det, seed, env_offset, step, act, law, act_scripted,
                         step_base=None):
    """policy_eval for one network agent against a scripted one
    (satrl_policy_eval_scripted): det 1, agent `agent` acts with its mean;
    det 0, with policy_act's sample."""
    N = obs.shape[0]
    _lib.require_cuda(obs, torch.float32, (N, 18), "obs")
    _lib.require_cuda(obs_law, torch.float32, (N, 18), "obs_law")
    for t, nm in ((act, "act"), (act_scripted, "act_scripted")):
        _lib.require_cuda(t, torch.float32, (N, 3), nm)
    if agent not in (0, 1):
        raise ValueError(f"agent is 0 (pursuer) or 1 (evader), got {agent!r}")
    if det not in (0, 1):
        raise ValueError(f"det is 0 or 1, got {det!r}")
    check(_lib.lib().satrl_policy_eval_scripted(int(H), N, ptr(obs), ptr(obs_law), ptr(P), int(agent),
                                                float(max_action), int(det), int(seed) & (2**64 - 1), int(env_offset),
                                                int(step), ptr(step_base), ptr(act), ptr(_law_block(law, obs.device)),
                                                ptr(act_scripted), stream_ptr()), "satrl_policy_eval_scripted")


def policy_eval(H, obs, P0, P1, max_action, det_mask, seed, env_offset, step, act0, act1=None, step_base=None):
    """Both agents' actions without log-probs (satrl_policy_eval): agent a
    with bit 1 << a of det_mask set acts with the mean (PPO_continuous.evaluate),
    the other one with policy_act's sample for the same noise key."""
    N = obs.shape[0]
    _lib.require_cuda(obs, torch.float32, (N, 18), "obs")
    for t, nm in ((act0, "act0"),) + (((act1, "act1"),) if P1 is not None else ()):
        _lib.require_cuda(t, torch.float32, (N, 3), nm)
    check(_lib.lib().satrl_policy_eval(int(H), N, ptr(obs), ptr(P0), ptr(P1), float(max_action), int(det_mask),
                                       int(seed) & (2**64 - 1), int(env_offset), int(step), ptr(step_base), ptr(act0),
                                       ptr(act1), stream_ptr()), "satrl_policy_eval")


REC_F64 = ["ret", "final_dis", "min_dis", "dv_p", "dv_e"]
REC_I32 = ["length", "outcome"]


def episode_record_reset(rec_f64, rec_i32, alive):
    """Episode records as before any step (satrl_episode_record_reset)."""
    N = rec_f64.shape[1]
    _lib.require_cuda(rec_f64, torch.float64, (len(REC_F64), N), "rec_f64")
    _lib.require_cuda(rec_i32, torch.int32, (len(REC_I32), N), "rec_i32")
    _lib.require_cuda(alive, torch.int32, (1,), "alive")
    check(_lib.lib().satrl_episode_record_reset(N, ptr(rec_f64), ptr(rec_i32), ptr(alive), stream_ptr()),
          "satrl_episode_record_reset")


def episode_record(reward, done, obs64, pa, ea, capture_reward, rec_f64, rec_i32, alive):
    """One env step into the records of every env's first episode
    (satrl_episode_record): reward f64 [N], done u8 [N], obs64 f64 [N,18] of
    VecSatellites.step, pa / ea f32 [N,3] the actions it was given."""
    N = reward.shape[0]
    _lib.require_cuda(reward, torch.float64, (N,), "reward")
    _lib.require_cuda(done, torch.uint8, (N,), "done")
    _lib.require_cuda(obs64, torch.float64, (N, 18), "obs64")
    _lib.require_cuda(pa, torch.float32, (N, 3), "pa")
    _lib.require_cuda(ea, torch.float32, (N, 3), "ea")
    _lib.require_cuda(rec_f64, torch.float64, (len(REC_F64), N), "rec_f64")
    _lib.require_cuda(rec_i32, torch.int32, (len(REC_I32), N), "rec_i32")
    _lib.require_cuda(alive, torch.int32, (1,), "alive")
    check(_lib.lib().satrl_episode_record(N, ptr(reward), ptr(done), ptr(obs64), ptr(pa), ptr(ea),
                                          float(capture_reward), ptr(rec_f64), ptr(rec_i32), ptr(alive),
                                          stream_ptr()), "satrl_episode_record")


def policy_value(H, obs, P, v_out):
    """critic(obs) on the fused MLP kernel (satrl_policy_value)."""
    N = obs.shape[0]
    _lib.require_cuda(obs, torch.float32, (N, 18), "obs")
    check(_lib.lib().satrl_policy_value(int(H), N, ptr(obs), ptr(P), ptr(v_out), stream_ptr()), "satrl_policy_value")
    return v_out


DIAG_SLOTS = ["rows", "surr", "kl", "log_ratio", "clipped", "ratio_max", "verr2", "verr", "vt", "vt2"]
DIAG_MAX_SLOT = DIAG_SLOTS.index("ratio_max")               # the one slot that is a max, not a sum


def diagnostics_scratch(n):
    """f64 elements of ppo_diagnostics' scratch for n rows (satrl_ppo_diagnostics_scratch)."""
    k = int(_lib.lib().satrl_ppo_diagnostics_scratch(int(n)))
    if k <= 0:
        raise ValueError(f"satrl_ppo_diagnostics_scratch({n}) failed")
    return k


def ppo_diagnostics(H, src, idx, P, epsilon, max_action, sums, scratch, rows_out=None):
    """The update-diagnostics sums (satrl_ppo_diagnostics, include/satrl_ppo.h)
    of the flat parameters P over rows src[idx] of the packed table (idx None:
    every row of src) into sums f64 [10] (DIAG_SLOTS); rows_out (optional) f32
    [n, 4] receives ratio, log ratio, v, 0 per row.  Asynchronous."""
    _lib.require_cuda(src, torch.float32, (src.shape[0], 32), "src")
    n = src.shape[0]
    if idx is not None:
        n = idx.numel()
        _lib.require_cuda(idx, torch.int64, (n,), "idx")
    _lib.require_cuda(P, torch.float32, None, "P")
    _lib.require_cuda(sums, torch.float64, (len(DIAG_SLOTS),), "sums")
    _lib.require_cuda(scratch, torch.float64, None, "scratch")
    if rows_out is not None:
        _lib.require_cuda(rows_out, torch.float32, None, "rows_out")
        if rows_out.dim() != 2 or rows_out.shape[0] < n or rows_out.shape[1] != 4:
            raise _lib.NativeError(f"rows_out shape {tuple(rows_out.shape)} holds fewer than {n} rows of 4")
    check(_lib.lib().satrl_ppo_diagnostics(int(H), n, ptr(src), ptr(idx), ptr(P), float(epsilon), float(max_action),
                                           ptr(sums), ptr(scratch), scratch.numel(), ptr(rows_out), stream_ptr()),
          "satrl_ppo_diagnostics")
    return sums


def reduce_diagnostics_sums(sums, pg):
    """The diagnostics sums of every rank's rows as one set (a new tensor,
    equal bits on every rank): the additive slots summed, the max slot maxed."""
    if pg is None:
        return sums.clone()
    out = _dist.sum_(sums, pg)
    out[DIAG_MAX_SLOT] = _dist.max_(sums[DIAG_MAX_SLOT:DIAG_MAX_SLOT + 1], pg)[0]
    return out


class UpdateDiagnostics:
    """What an update did, from the sums of satrl_ppo_diagnostics (a pure
    function of them: no GPU).  Every field is over the whole set of rows the
    sums cover, under the parameters at the time of the call:
      rows, policy_loss (-mean min(surr1, surr2)), entropy (state-independent:
      from log_std), actor_loss (policy_loss - entropy_coef * entropy),
      value_loss (mean (v - vt)^2, mse_loss), approx_kl (mean (ratio - 1) -
      log ratio), mean_log_ratio, clip_fraction, ratio_max,
      explained_variance_after (1 - Var(vt - v) / Var(vt), population
      variances; NaN when Var(vt) = 0)."""

    FIELDS = ("rows", "policy_loss", "entropy", "actor_loss", "value_loss", "approx_kl", "mean_log_ratio",
              "clip_fraction", "ratio_max", "explained_variance_after")

    def __init__(self, sums, **fields):
        self.sums = sums
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    @classmethod
    def from_sums(cls, sums, log_std, entropy_coef):
        sums = np.array(sums, dtype=np.float64).reshape(-1)
        if sums.shape[0] != len(DIAG_SLOTS):
            raise ValueError(f"{len(DIAG_SLOTS)} sums expected, got {sums.shape[0]}")
        s = {k: float(v) for k, v in zip(DIAG_SLOTS, sums)}
        n = s["rows"]
        if not n > 0:
            raise ValueError("diagnostics over no rows")
        entropy = float(sum(float(x) for x in np.asarray(log_std, dtype=np.float64).reshape(-1))) + 3 * ENT_CONST
        policy_loss = -s["surr"] / n
        var_vt = s["vt2"] / n - (s["vt"] / n) ** 2
        var_err = s["verr2"] / n - (s["verr"] / n) ** 2
        return cls(sums, rows=int(n), policy_loss=policy_loss, entropy=entropy,
                   actor_loss=policy_loss - float(entropy_coef) * entropy, value_loss=s["verr2"] / n,
                   approx_kl=s["kl"] / n, mean_log_ratio=s["log_ratio"] / n, clip_fraction=s["clipped"] / n,
                   ratio_max=s["ratio_max"],
                   explained_variance_after=1.0 - var_err / var_vt if var_vt > 0 else float("nan"))

    def as_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def __repr__(self):
        return "UpdateDiagnostics(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.FIELDS) + ")"


def moments(x, out=None):
    out = torch.zeros(2, dtype=torch.float64, device=x.device) if out is None else out
    x = x.reshape(-1)
    # the fixed-order form: the advantage moments and explained variance of a run and
    # of its resumed copy are the same bits (satrl_moments' atomics are not)
    need = int(_lib.lib().satrl_moments_scratch(x.numel()))
    scratch = torch.empty(max(need, 0), dtype=torch.float64, device=x.device)
    check(_lib.lib().satrl_moments_ordered(x.numel(), ptr(x), ptr(out), ptr(scratch), scratch.numel(), stream_ptr()),
          "satrl_moments_ordered")
    return out


# ---------------------------------------------------------------------------
# fused minibatch step (ppo_continuous.py:213-239), include/satrl_ppo.h
# ---------------------------------------------------------------------------
OFF_NAMES = ["W2", "W1", "b2", "W3a", "b3a", "ls", "W3c", "b3c", "total"]


def ppo_layout(H):
    off = (C.c_int64 * 9)()
    check(_lib.lib().satrl_ppo_layout(int(H), off), "satrl_ppo_layout")
    return dict(zip(OFF_NAMES, [int(v) for v in off]))


def w2x_floats(H):
    """f32 elements of the fc2 operand image (satrl_ppo_w2x_floats)."""
    n = int(_lib.lib().satrl_ppo_w2x_floats(int(H)))
    if n <= 0:
        raise ValueError(f"hidden width {H} not supported")
    return n


def w2x_image(W2, H):
    """Host statement of satrl_ppo_w2x_sync: the fc2 operand image of the two
    nets' fc2.weight W2 (flat [2*H*H] f32), the f32 fc2.weight^T per net."""
    return W2.reshape(2, H, H).transpose(1, 2).contiguous().reshape(-1)


def w2x_decode(img, H):
    """fc2.weight^T per net [2, H, H] f32 from an operand image."""
    return img.view(2, H, H)


def rowpass_exchange_check(stream=None, timeout_s=None):
    """satrl_ppo_rowpass_error (include/satrl_ppo.h): waits for the stream (at
    most timeout_s of host time, default the DP watchdog's deadline
    SATRL_DP_TIMEOUT_S: a stream stuck behind a dead peer's collective raises
    NativeError instead of hanging); raises RuntimeError if a column-split
    short rowpass launch timed out waiting for the other workgroups of its
    group (its outputs, hence this update, are invalid), after the library has
    re-armed the exchange state."""
    L = _lib.lib()
    e = C.c_int(0)
    t = _dist.dp_timeout_s() if timeout_s is None else float(timeout_s)
    check(L.satrl_ppo_rowpass_error(C.byref(e), t, stream_ptr(stream)), "satrl_ppo_rowpass_error")
    if e.value:
        raise RuntimeError("satrl_ppo_rowpass_kx: a column-split exchange (its workgroups were not resident "
                           "together) or an LDS hand-off of the 32-row kernel timed out; the update is invalid")


def step_plan(H, mb, net=-1):
    """satrl_ppo_step_plan (include/satrl_ppo.h): the library's plan of the
    minibatch step for (H, mb, net) as a _lib.StepPlan -- which kernels run
    (step, rowpass: _lib.STEP_* / _lib.RP_*), this minibatch's row blocks and
    splits, whether its rowpass can set the error word, and the capacity of
    every buffer.  Host arithmetic only, no device call."""
    plan = _lib.StepPlan()
    if _lib.lib().satrl_ppo_step_plan(int(H), int(mb), int(net), C.byref(plan)) != 0:
        raise ValueError(f"satrl_ppo_step_plan: no minibatch step for H {H}, mb {mb}, net {net}")
    return plan


def _update_plans(H, mb, B):
    """The plans of the minibatches an update of B rows in minibatches of mb
    steps: the full minibatch min(mb, B) and the ragged tail (none where the
    library has no step: an empty update, an unsupported width)."""
    mb = min(int(mb), int(B))
    plans = []
    for m in ((mb, int(B) % mb) if mb > 0 else ()):
        plan = _lib.StepPlan()
        if m > 0 and _lib.lib().satrl_ppo_step_plan(int(H), m, -1, C.byref(plan)) == 0:
            plans.append(plan)
    return plans


def uses_column_split(H, mb, B):
    """True when an update of B rows in minibatches of mb may run the
    column-split short rowpass (the plan of its full or ragged-tail minibatch
    says so: H = 256 up to the kernel's row limit)."""
    return any(p.rowpass == _lib.RP_CS for p in _update_plans(H, mb, B))


def rowpass_sync(mode=None):
    """satrl_ppo_rowpass_sync (include/satrl_ppo.h), a development switch:
    how the phases of the 32-row H = 256 k-packed rowpass wait for each other,
    0 workgroup barriers, 1 per-chunk LDS hand-offs (bitwise the same
    outputs).  Sets the process-wide mode (None: only queries) and returns the
    previous one; a captured graph keeps the form it was captured with."""
    prev = _lib.lib().satrl_ppo_rowpass_sync(-1 if mode is None else int(mode))
    if prev < 0:
        raise ValueError(f"rowpass_sync: mode {mode!r} is not 0 or 1")
    return prev


def rowpass_dskip(mode=None):
    """satrl_ppo_rowpass_dskip (described in include/satrl_ppo.h; exported by
    the library but outside the declared ABI and _lib's table, so bound here),
    a development switch:
    whether a wave of the 32-row H = 256 k-packed rowpass (either sync form)
    may skip phase D where a saturated fc1 makes its product unused, 0 never
    (phase D always runs), 1 the product default (bitwise the same outputs).
    Sets the process-wide mode (None: only queries) and returns the previous
    one; a captured graph keeps the mode it was captured with."""
    try:
        fn = _lib.lib().satrl_ppo_rowpass_dskip
    except AttributeError as e:
        raise _lib.NativeError(f"{_lib.LIB_PATH} has no satrl_ppo_rowpass_dskip: it was not built from this tree") from e
    fn.argtypes, fn.restype = [C.c_int], C.c_int
    prev = fn(-1 if mode is None else int(mode))
    if prev < 0:
        raise ValueError(f"rowpass_dskip: mode {mode!r} is not 0 or 1")
    return prev


def uses_handoff(H, mb, B):
    """True when an update of B rows in minibatches of mb runs the hand-off
    form of the 32-row rowpass (the plan of its full or ragged-tail minibatch
    says so: H = 256 above the 16-row range while rowpass_sync() == 1).  Its
    bounded waits report through the column split's error word."""
    return any(p.rowpass == _lib.RP_WG32_HANDOFF for p in _update_plans(H, mb, B))


class FusedMinibatch:
    """One PPO minibatch step for actor + critic on shared rows:
    satrl_ppo_rowpass (gather, MLP forward/backward on f32 MFMA, losses),
    satrl_ppo_dw2 (the dW2 weight gradient, split-K), satrl_ppo_reduce and
    satrl_ppo_adam, both nets per launch.  The actor and
    critic steps share nothing but the rows (ppo_continuous.py:216-239 runs
    two independent optimisers); with ``split_chains`` they run as two
    per-net chains on two streams (the critic on a side stream, fork/join per
    group).  Under data parallelism both nets' gradients travel in one
    all-reduce.  Groups of ``group`` minibatches are captured into a hipGraph
    and replayed over [group, mb] blocks of a device permutation."""

    def __init__(self, learner, mb, group, use_graph=True, split_chains=False):
        self.L = learner
        self.mb = int(mb)
        self.group = int(group)
        self.use_graph = use_graph
        # dW2 (the fc2 weight gradient dZ2^T H1), hand-written at every width.
        # Which step runs, and the size of every buffer, is the library's plan
        # for this minibatch size (satrl_ppo_step_plan):
        # STEP_FUSED (H = 64, configs[1]): the rowpass multiplies each block's
        # dW2 partial out of LDS itself (satrl_ppo_rowpass_dw2), bitwise the
        # dw2_kernel's one-chunk splits, so a minibatch step is three launches;
        # STEP_KX (H = 256): the rowpass writes H1 / dZ2 as k-packed bf16 planes
        # and dW2 runs on the split-bf16 MFMA from them (satrl_ppo_rowpass_kx /
        # satrl_ppo_dw2_kx_w1), for every minibatch size;
        # STEP_ROWS (H = 128): f32 rows and dw2_kernel (satrl_ppo_dw2)
        H, dev = learner.H, learner.device
        plan = step_plan(H, self.mb)
        self.step_kind = plan.step
        self.fused_dw2 = plan.step == _lib.STEP_FUSED
        self.kx_on = plan.step == _lib.STEP_KX
        # two concurrent per-net chains: measured no faster than one fused chain at
        # H = 256 / 64, mb = 4096 on MI355X (the chains run in lockstep), so off by default
        self.split = bool(split_chains) and learner.pg is None
        self.nwg, self.nblk = plan.slab_blocks, plan.norm_blocks
        self.S = plan.splits
        f32 = dict(dtype=torch.float32, device=dev)
        # f32 H1 / dZ2 rows: satrl_ppo_rowpass (the roofline's rowpass timing,
        # tests) and the H = 128 dW2; the H = 256 step hands them over as planes
        self.H1 = torch.empty(plan.rows_floats, **f32)
        self.dZ2 = torch.empty(plan.rows_floats, **f32)
        self.kx_elems = plan.kx_elems
        if self.kx_on:
            self.H1x = torch.empty(self.kx_elems, dtype=torch.int16, device=dev)
            self.dZ2x = torch.empty(self.kx_elems, dtype=torch.int16, device=dev)
        self.ptail = torch.empty(plan.ptail_floats, **f32)
        self.pw1 = torch.empty(plan.pw1_floats, **f32)
        # sized for the largest split count any minibatch size up to mb can
        # produce, so a ragged tail minibatch whose S exceeds the full
        # minibatch's never writes past the slabs (the launch guard below
        # compares against this capacity)
        self.p2_splits = plan.max_splits
        self.p2 = torch.empty(plan.p2_floats, **f32)
        self.nsq = torch.zeros((2, 2 * self.nblk), dtype=torch.float64, device=dev)   # one per chain
        self.idx = torch.zeros((self.group, self.mb), dtype=torch.int64, device=dev)
        # the rows of one group of minibatches, gathered contiguously once per
        # group (one index_select) so rowpass reads them without an index hop
        self.stage = torch.empty((self.group * self.mb, 32), **f32)
        self.side = torch.cuda.Stream(device=dev) if self.split and torch.cuda.is_available() else None
        self.graph = None
        self._src_ptr = None
        # graph replays walk the epoch's permutation through a device group
        # counter (satrl_ppo_stage / satrl_ppo_group_advance): no host copy
        # or host round trip between groups
        self.perm_buf = None
        self.grp = torch.zeros(1, dtype=torch.int64, device=dev)
        if learner.pg is not None and _dist.world_size(learner.pg) > 1 and torch.cuda.is_available():
            # every rank's first step of this shape starts together (a rank
            # still setting up must not run into the peer all-reduce's bounded
            # wait)
            import torch.distributed as dist
            torch.cuda.synchronize()
            dist.barrier(group=learner.pg)

    def rowpass(self, src, idx, mb=None, net=-1):
        """satrl_ppo_rowpass alone (a pure function of src, idx and the
        parameters: bench.py times it on its own for the roofline).  idx None:
        rows 0..mb-1 of src.  net -1: both nets in one launch."""
        L = self.L
        H = L.H
        mb = self.mb if mb is None else int(mb)
        n = 2 * mb * H
        H1, dZ2 = self.H1[:n], self.dZ2[:n]
        check(_lib.lib().satrl_ppo_rowpass(H, mb, int(net), ptr(src), None if idx is None else ptr(idx), ptr(L.P),
                                           ptr(L.W2T), float(L.epsilon), float(L.entropy_coef), float(L.max_action),
                                           ptr(H1), ptr(dZ2), ptr(self.ptail), ptr(self.pw1), stream_ptr()),
                  "satrl_ppo_rowpass")
        return H1, dZ2

    def kx(self, mb):
        """True when a minibatch of mb rows takes the k-packed split-bf16 dW2
        path (H = 256, every minibatch size)."""
        return self.kx_on

    def rowpass_kx(self, src, idx, mb=None, net=-1):
        """satrl_ppo_rowpass_kx: the rowpass with H1 / dZ2 written as k-packed
        bf16 planes into self.H1x / self.dZ2x (the dW2 operands)."""
        L = self.L
        mb = self.mb if mb is None else int(mb)
        check(_lib.lib().satrl_ppo_rowpass_kx(L.H, mb, int(net), ptr(src), None if idx is None else ptr(idx),
                                              ptr(L.P), ptr(L.W2T), float(L.epsilon), float(L.entropy_coef),
                                              float(L.max_action), ptr(self.H1x), ptr(self.dZ2x), self.H1x.numel(),
                                              ptr(self.ptail), ptr(self.pw1), stream_ptr()), "satrl_ppo_rowpass_kx")

    def dw2_kx(self, mb, S, net=-1):
        """satrl_ppo_dw2_kx: the dW2 split-K slabs from the k-packed planes."""
        check(_lib.lib().satrl_ppo_dw2_kx(self.L.H, int(mb), int(net), int(S), ptr(self.H1x), ptr(self.dZ2x),
                                          self.H1x.numel(), ptr(self.p2), self.p2.numel(), stream_ptr()),
              "satrl_ppo_dw2_kx")

    def dw2_kx_w1(self, mb, S, net, mode, nsq):
        """satrl_ppo_dw2_kx_w1: dw2_kx with the reduce's W1 / tail regions
        (G, and their norm pairs with mode 3) in the same launch; the reduce
        that follows takes mode bit 4 (the W2 region only)."""
        check(_lib.lib().satrl_ppo_dw2_kx_w1(self.L.H, int(mb), int(net), int(S), ptr(self.H1x), ptr(self.dZ2x),
                                             self.H1x.numel(), ptr(self.p2), self.p2.numel(), int(mode), ptr(self.pw1),
                                             ptr(self.ptail), ptr(self.L.G), ptr(nsq), stream_ptr()),
              "satrl_ppo_dw2_kx_w1")

    def rowpass_dw2(self, src, idx, mb=None, net=-1):
        """satrl_ppo_rowpass_dw2 (H = 64): the rowpass with each block's dW2
        partial written as split-K slab of p2 (no H1 / dZ2 stores)."""
        L = self.L
        mb = self.mb if mb is None else int(mb)
        check(_lib.lib().satrl_ppo_rowpass_dw2(L.H, mb, int(net), ptr(src), None if idx is None else ptr(idx),
                                               ptr(L.P), ptr(L.W2T), float(L.epsilon), float(L.entropy_coef),
                                               float(L.max_action), ptr(self.p2), self.p2.numel(), ptr(self.ptail),
                                               ptr(self.pw1), stream_ptr()), "satrl_ppo_rowpass_dw2")

    def rowpass_ratio(self, src, idx, ratio, mb=None, net=-1):
        """satrl_ppo_rowpass_ratio: satrl_ppo_rowpass that also writes the
        actor's probability ratio exp(logp - logp_old) per row into `ratio`."""
        L = self.L
        H = L.H
        mb = self.mb if mb is None else int(mb)
        n = 2 * mb * H
        _lib.require_cuda(ratio, torch.float32, (mb,), "ratio")
        check(_lib.lib().satrl_ppo_rowpass_ratio(H, mb, int(net), ptr(src), None if idx is None else ptr(idx),
                                                 ptr(L.P), ptr(L.W2T), float(L.epsilon), float(L.entropy_coef),
                                                 float(L.max_action), ptr(self.H1[:n]), ptr(self.dZ2[:n]),
                                                 ptr(self.ptail), ptr(self.pw1), ptr(ratio), stream_ptr()),
              "satrl_ppo_rowpass_ratio")
        return ratio

    def step_kernel_flops(self, mb=None):
        """Algorithmic FLOPs of the step's first launch: the rowpass, plus the
        dW2 product (2 H^2 per row and net) where it is fused in (H = 64)."""
        mb = self.mb if mb is None else int(mb)
        H = self.L.H
        return self.rowpass_flops(H, mb) + (2 * 2 * H * H * mb if self.fused_dw2 else 0)

    @staticmethod
    def rowpass_flops(H, mb):
        """Algorithmic FLOPs of one rowpass launch over both nets (DESIGN.md
        "Roofline"): per row and net fc1 forward + [dW1|db1] (2*18*H + H
        each), fc2 forward and dH1 (2*H*H each); output layers forward /
        backward (actor 3 outputs x 3 products, critic 1 x 3)."""
        per_row = 2 * (2 * (2 * 18 * H + H) + 2 * (2 * H * H)) + 2 * 3 * 3 * H + 2 * 1 * 3 * H
        return per_row * mb

    def max_splits(self, H):
        """Upper bound of splits(H, m) over every m <= mb (the plan's p2 capacity)."""
        return step_plan(H, self.mb).max_splits

    def splits(self, H, mb):
        """split-K ways of the dW2 product for a minibatch of mb rows (both
        nets' count: a one-net chain of split mode uses the same)."""
        return step_plan(H, mb).splits

    def _dw2(self, H1, dZ2, mb, S, net):
        """dW2 = dZ2^T @ H1 split-K S ways into the slabs p2 [2][S][H][H] (f32 rows)."""
        check(_lib.lib().satrl_ppo_dw2(self.L.H, mb, net, S, ptr(H1), ptr(dZ2), ptr(self.p2), self.p2.numel(),
                                       stream_ptr()), "satrl_ppo_dw2")

    def _net_step(self, src, idx, mb, net, events=None, skip_rowpass=False):
        """One minibatch step of one chain.  Bench-only knobs: `events` (a pair
        of torch.cuda.Event) recorded around the rowpass launch; skip_rowpass
        runs the rest of the chain on the last H1/dZ2/slabs (timing only)."""
        L = self.L
        H = L.H
        S = self.S if mb == self.mb else self.splits(H, mb)
        if S > self.p2_splits:
            raise _lib.NativeError(f"dW2 split count {S} exceeds the slab capacity {self.p2_splits}")
        lib, sp = _lib.lib(), stream_ptr()
        nsq = self.nsq[max(net, 0)]
        if events is not None:
            events[0].record()
        kind = self.step_kind
        H1 = dZ2 = None                                    # (f32 rows: STEP_ROWS only)
        if skip_rowpass:
            n = 2 * mb * H
            H1, dZ2 = self.H1[:n], self.dZ2[:n]
        elif kind == _lib.STEP_KX:
            self.rowpass_kx(src, idx, mb, net)
        elif kind == _lib.STEP_FUSED:
            self.rowpass_dw2(src, idx, mb, net)
        else:
            H1, dZ2 = self.rowpass(src, idx, mb, net)
        if events is not None:
            events[1].record()
        # the slabs summed into G; alone also the norms and the step counters,
        # which under data parallelism follow the all-reduce (reduce_dp)
        dp = L.pg is not None
        mode = 1 if dp else 3
        nsq_r, steps_r = (None, None) if dp else (nsq, L.steps)
        if kind == _lib.STEP_KX:
            # the reduce's W1 / tail regions ride in the dW2 launch, the reduce sums the W2 region
            self.dw2_kx_w1(mb, S, net, mode, nsq_r)
            mode |= 4
        elif kind == _lib.STEP_ROWS:
            self._dw2(H1, dZ2, mb, S, net)
        check(lib.satrl_ppo_reduce(H, mb, net, S, mode, ptr(self.p2), self.p2.numel(), ptr(self.pw1), ptr(self.ptail),
                                   ptr(L.G), ptr(nsq_r), ptr(steps_r), sp), "satrl_ppo_reduce")
        if dp:
            # one bucket, both nets: SUM over the ranks, then G /= world and the norms in one launch
            if L.peer is not None and net < 0:
                L.peer.all_reduce_dp_(H, mb, L.G, nsq, L.steps)              # peer kernel, reduce_dp fused
            elif L.comm is not None:
                L.comm.all_reduce_sum_(L.G)                                   # RCCL on this stream (capturable)
            else:
                _dist.sum_inplace_(L.G, L.pg)                                 # c10d (gloo in the CPU tests)
            if L.peer is None or net >= 0:
                check(lib.satrl_ppo_reduce_dp(H, mb, net, _dist.world_size(L.pg), ptr(L.G), ptr(nsq), ptr(L.steps),
                                              sp), "satrl_ppo_reduce_dp")
        check(lib.satrl_ppo_adam(H, mb, net, ptr(nsq), ptr(L.steps), ptr(L.bct), L.bct.shape[0], ptr(L.lr),
                                 float(L.beta1), float(L.beta2), float(L.adam_eps), 0.5, int(bool(L.use_grad_clip)),
                                 ptr(L.G), ptr(L.P), ptr(L.M), ptr(L.V), ptr(L.W2T), sp), "satrl_ppo_adam")

    def _chains(self, fn):
        """fn(net) for the actor on the current stream and the critic on the
        side stream (fork/join), or fn(-1) once when not split."""
        if not self.split:
            fn(-1)
            return
        cur = torch.cuda.current_stream()
        self.side.wait_stream(cur)
        fn(0)
        with torch.cuda.stream(self.side):
            fn(1)
        cur.wait_stream(self.side)

    def step(self, src, idx, mb=None, events=None, skip_rowpass=False):
        mb = self.mb if mb is None else int(mb)
        if events is not None or skip_rowpass:
            self._net_step(src, idx, mb, -1, events, skip_rowpass)
            return
        self._chains(lambda net: self._net_step(src, idx, mb, net))

    def _group(self, src, ng):
        """ng minibatches whose indices are in self.idx[:ng]: one gather of
        their rows into self.stage, then ng steps per chain on contiguous rows."""
        mb = self.mb
        torch.index_select(src, 0, self.idx[:ng].view(-1), out=self.stage[:ng * mb])

        def chain(net):
            for k in range(ng):
                self._net_step(self.stage[k * mb:(k + 1) * mb], None, mb, net)
        self._chains(chain)

    def _group_dev(self, src):
        """One graph group: stage the rows of the next `group` minibatches of
        self.perm_buf (offset grp[0]), step them, advance grp."""
        mb, G = self.mb, self.group
        check(_lib.lib().satrl_ppo_stage(G * mb, ptr(src), ptr(self.perm_buf), ptr(self.grp), ptr(self.stage),
                                         stream_ptr()), "satrl_ppo_stage")

        def chain(net):
            for k in range(G):
                self._net_step(self.stage[k * mb:(k + 1) * mb], None, mb, net)
        self._chains(chain)
        check(_lib.lib().satrl_ppo_group_advance(ptr(self.grp), stream_ptr()), "satrl_ppo_group_advance")

    def _capture(self, src):
        if self.L.comm is not None:
            self.L.comm.warm(self.L.G)        # RCCL connects lazily: never inside the capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._group_dev(src)
        self._src_ptr = src.data_ptr()

    def run(self, src, perm):
        """All minibatches of one epoch (BatchSampler drop_last=False order)."""
        B = perm.numel()
        mb, G = self.mb, self.group
        nfull = B // mb
        graphable = self.use_graph and torch.cuda.is_available() and (self.L.pg is None or self.L.comm is not None
                                                                       or self.L.peer is not None)
        k = 0
        if graphable and nfull >= G:
            if self.perm_buf is None or self.perm_buf.numel() < B:
                self.perm_buf = torch.empty(B, dtype=torch.int64, device=perm.device)
                self.graph = None
            if perm.data_ptr() != self.perm_buf.data_ptr():
                self.perm_buf[:B].copy_(perm)
            if self.graph is None or self._src_ptr != src.data_ptr():
                self._capture(src)
            self.grp.zero_()
            comm, peer = self.L.comm, self.L.peer
            inflight = []
            for _ in range(nfull // G):
                self.graph.replay()
                if comm is not None or peer is not None:
                    # watchdog between replays: at most two replays queued ahead
                    # of the host.  RCCL: the oldest is waited for with the
                    # deadline while ncclCommGetAsyncError is polled
                    # (rccl.Comm.wait_event); peer: the oldest is polled against
                    # a host deadline, then the error word is read on a side
                    # stream (the queued replays keep running), so a lost rank
                    # stops the update there
                    ev = torch.cuda.Event()
                    ev.record()
                    inflight.append(ev)
                    if len(inflight) > 2:
                        if comm is not None:
                            comm.wait_event(inflight.pop(0), _dist.dp_timeout_s())
                        else:
                            peer.wait_event(inflight.pop(0))
            k = (nfull // G) * G
        while k < nfull:                      # the rest of the full minibatches, eagerly
            ng = min(G, nfull - k)
            self.idx[:ng].copy_(perm[k * mb:(k + ng) * mb].view(ng, mb))
            self._group(src, ng)
            k += ng
        if B % mb:
            tail = perm[nfull * mb:].contiguous()
            self.step(src, tail, mb=tail.numel())


def adam_bias_table(beta1=0.9, beta2=0.999):
    """{1 - beta1**k, sqrt(1 - beta2**k)} in python-float math, as
    torch.optim.Adam._single_tensor_adam computes them per step; rows up to
    the step where both are exactly 1.0."""
    rows = [(0.0, 0.0)]
    k = 1
    while True:
        b1 = 1 - beta1 ** k
        b2 = math.sqrt(1 - beta2 ** k)
        rows.append((b1, b2))
        if b1 == 1.0 and b2 == 1.0:
            break
        k += 1
    return torch.tensor(rows, dtype=torch.float64)


def _bind(module, name, view):
    """Make module.<name> a Parameter that aliases ``view`` (flat storage)."""
    module._parameters[name] = nn.Parameter(view, requires_grad=False)


class PPOLearner:
    """Actor/critic pair whose parameters, gradients and Adam moments live in
    flat device buffers (include/satrl_ppo.h layout); the nn.Module
    parameters are views into ``P`` so every forward pass (rollout, values,
    evaluate) reads the weights the fused update writes."""

    def __init__(self, args, agent_idx, device=None, pg=None, graph_group=16, use_graph=True):
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.args = args
        self.H = int(args.hidden_width)
        if not args.use_tanh:
            raise NotImplementedError("the fused update implements the tanh networks (use_tanh=True, CPPO_main.py:38)")
        self.max_action = float(args.max_action)
        self.batch_size = args.batch_size
        self.mini_batch_size = args.mini_batch_size
        self.max_train_steps = args.max_train_steps
        self.lr_a, self.lr_c = args.lr_a, args.lr_c
        self.gamma, self.lamda = args.gamma, args.lamda
        self.epsilon = args.epsilon
        self.K_epochs = args.K_epochs
        self.entropy_coef = args.entropy_coef
        self.use_grad_clip = args.use_grad_clip
        self.use_lr_decay = args.use_lr_decay
        self.use_adv_norm = args.use_adv_norm
        self.beta1, self.beta2 = 0.9, 0.999                  # torch.optim.Adam defaults
        self.adam_eps = 1e-5 if args.set_adam_eps else 1e-8  # ppo_continuous.py:161-166
        self.pg = pg
        # RCCL communicator for the in-graph gradient all-reduce (None without a
        # process group, or on gloo: the c10d all-reduce then runs eagerly)
        mode = getattr(args, "allreduce", "rccl")
        if mode not in ("rccl", "peer"):
            raise ValueError("allreduce must be 'rccl' or 'peer'")
        on_gpus = pg is not None and self.device.type == "cuda"
        self.comm = _rccl.for_group(pg, self.device) if on_gpus and mode == "rccl" else None
        self.peer = None
        if on_gpus and mode == "peer":
            from .peer import PeerComm
            self.peer = PeerComm(pg, ppo_layout(int(args.hidden_width))["total"], self.device, int(args.hidden_width))
        self.graph_group = graph_group
        self.use_graph = use_graph
        # CPU init with the reference's RNG consumption order (actor, then critic)
        actor = Actor_Gaussian(args, agent_idx)
        critic = Critic(args, agent_idx)
        self.off = ppo_layout(self.H)
        H, o = self.H, self.off
        f32 = dict(dtype=torch.float32, device=self.device)
        self.P = torch.zeros(o["total"], **f32)
        self.G = torch.zeros(o["total"], **f32)
        self.M = torch.zeros(o["total"], **f32)
        self.V = torch.zeros(o["total"], **f32)
        self.steps = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.bct = adam_bias_table(self.beta1, self.beta2).to(self.device)
        self.lr = torch.tensor([float(self.lr_a), float(self.lr_c)], **f32)
        self.actor = actor.to(self.device)
        self.critic = critic.to(self.device)
        P = self.P
        self.W2v = P[o["W2"]:o["W2"] + 2 * H * H].view(2, H, H)
        # the fc2 operand image the rowpass reads (the f32 fc2.weight^T; satrl_ppo.h)
        self.W2T = torch.zeros(w2x_floats(H), **f32)
        self.GW2v = self.G[o["W2"]:o["W2"] + 2 * H * H].view(2, H, H)
        W1 = P[o["W1"]:o["W1"] + 2 * H * 20].view(2, H, 20)
        self.GW1v = self.G[o["W1"]:o["W1"] + 2 * H * 20].view(2, H, 20)
        b2 = P[o["b2"]:o["b2"] + 2 * H].view(2, H)
        views = {
            (self.actor.fc1, "weight"): W1[0, :, :18], (self.actor.fc1, "bias"): W1[0, :, 18],
            (self.critic.fc1, "weight"): W1[1, :, :18], (self.critic.fc1, "bias"): W1[1, :, 18],
            (self.actor.fc2, "weight"): self.W2v[0], (self.actor.fc2, "bias"): b2[0],
            (self.critic.fc2, "weight"): self.W2v[1], (self.critic.fc2, "bias"): b2[1],
            (self.actor.mean_layer, "weight"): P[o["W3a"]:o["W3a"] + 3 * H].view(3, H),
            (self.actor.mean_layer, "bias"): P[o["b3a"]:o["b3a"] + 3],
            (self.actor, "log_std"): P[o["ls"]:o["ls"] + 3].view(1, 3),
            (self.critic.fc3, "weight"): P[o["W3c"]:o["W3c"] + H].view(1, H),
            (self.critic.fc3, "bias"): P[o["b3c"]:o["b3c"] + 1],
        }
        with torch.no_grad():
            for (mod, name), view in views.items():
                view.copy_(getattr(mod, name).detach())
                _bind(mod, name, view)
        self._steppers = {}
        self._diag = None                                    # diagnostics(): (sums, scratch), on first use

    # -- lr ---------------------------------------------------------------------
    def lr_decay(self, total_steps):
        """ppo_continuous.py:244-250.  The reference's total_steps is an
        episode index below max_train_steps (its loop stops there,
        CPPO_main.py:110); the vectorised engine counts finished episodes over
        all envs and ranks, which can pass the budget inside an iteration, so
        the progress fraction is clamped to [0, 1] and lr never goes negative
        (identical to the reference wherever the reference runs)."""
        frac = min(max(float(total_steps) / self.max_train_steps, 0.0), 1.0)
        lr_a_now = self.lr_a * (1 - frac)
        lr_c_now = self.lr_c * (1 - frac)
        self.lr.copy_(torch.tensor([lr_a_now, lr_c_now], dtype=torch.float32))

    @property
    def lr_now(self):
        v = self.lr.cpu().tolist()
        return v[0], v[1]

    def param_groups(self):
        """(actor params, critic params) as tensors, reference order."""
        return list(self.actor.parameters()), list(self.critic.parameters())

    def flat_views(self, buf):
        """{"actor.fc1.weight": view, ...} of a flat buffer (P, G, M or V)."""
        H, o = self.H, self.off
        W1 = buf[o["W1"]:o["W1"] + 2 * H * 20].view(2, H, 20)
        W2 = buf[o["W2"]:o["W2"] + 2 * H * H].view(2, H, H)
        b2 = buf[o["b2"]:o["b2"] + 2 * H].view(2, H)
        return {"actor.fc1.weight": W1[0, :, :18], "actor.fc1.bias": W1[0, :, 18],
                "actor.fc2.weight": W2[0], "actor.fc2.bias": b2[0],
                "actor.mean_layer.weight": buf[o["W3a"]:o["W3a"] + 3 * H].view(3, H),
                "actor.mean_layer.bias": buf[o["b3a"]:o["b3a"] + 3],
                "actor.log_std": buf[o["ls"]:o["ls"] + 3].view(1, 3),
                "critic.fc1.weight": W1[1, :, :18], "critic.fc1.bias": W1[1, :, 18],
                "critic.fc2.weight": W2[1], "critic.fc2.bias": b2[1],
                "critic.fc3.weight": buf[o["W3c"]:o["W3c"] + H].view(1, H),
                "critic.fc3.bias": buf[o["b3c"]:o["b3c"] + 1]}

    # -- update -----------------------------------------------------------------
    def sync_w2t(self):
        """Refresh the fc2 operand image from P (Adam keeps it current during an
        update; this covers loads / external writes between updates)."""
        if self.device.type == "cuda":
            check(_lib.lib().satrl_ppo_w2x_sync(self.H, -1, ptr(self.P), ptr(self.W2T), stream_ptr()),
                  "satrl_ppo_w2x_sync")
        else:
            self.W2T.copy_(w2x_image(self.P[:2 * self.H * self.H], self.H))

    # -- the whole state (satrl/checkpoint.py) --------------------------------------
    def state(self):
        """What an update carries to the next, as CPU numpy arrays: the flat
        parameters P, Adam's moments M and V and step counts (f64 [2]) and the
        decayed learning rates (f32 [2]).  G and every scratch buffer are
        rewritten before they are read."""
        return {"H": self.H, "P": self.P.cpu().numpy(), "M": self.M.cpu().numpy(), "V": self.V.cpu().numpy(),
                "steps": self.steps.cpu().numpy(), "lr": self.lr.cpu().numpy()}

    def load_state(self, d):
        """Restore state(), in place: the module parameters (views into P), the
        captured update graphs and every plan's buffers stay valid; the fc2
        operand image is refreshed from the new P."""
        if int(np.asarray(d["H"])) != self.H:
            raise ValueError(f"a learner state of hidden width {int(np.asarray(d['H']))} for a learner of {self.H}")
        for k, buf in (("P", self.P), ("M", self.M), ("V", self.V), ("steps", self.steps), ("lr", self.lr)):
            a = torch.from_numpy(np.ascontiguousarray(d[k]))
            if a.dtype != buf.dtype or tuple(a.shape) != tuple(buf.shape):
                raise ValueError(f"learner state {k!r}: {a.dtype} {tuple(a.shape)} for {buf.dtype} "
                                 f"{tuple(buf.shape)}")
            buf.copy_(a)
        self.sync_w2t()

    def w2t_f32(self):
        """fc2.weight^T per net [2, H, H] f32 from the operand image."""
        return w2x_decode(self.W2T, self.H)

    def stepper(self, mb):
        if mb not in self._steppers:
            self._steppers[mb] = FusedMinibatch(self, mb, self.graph_group, use_graph=self.use_graph)
        return self._steppers[mb]

    def normalize_adv(self, adv):
        """ppo_continuous.py:209-210 (unbiased std); global over the process group."""
        if not self.use_adv_norm:
            return adv
        if self.pg is None:
            return (adv - adv.mean()) / (adv.std() + 1e-5)
        cnt = torch.tensor([float(adv.numel())], dtype=torch.float64, device=adv.device)
        mean, std = _dist.global_mean_std(torch.cat([moments(adv), cnt]), self.pg)
        return (adv - mean.float()) / (std.float() + 1e-5)

    def diagnostics_sums(self, src, idx=None, rows_out=None):
        """satrl_ppo_diagnostics of the current parameters over src[idx] (idx
        None: every row): the f64 [10] device sums (DIAG_SLOTS), a buffer of
        the learner's own that the next call overwrites.  No host sync."""
        n = src.shape[0] if idx is None else idx.numel()
        need = diagnostics_scratch(n)
        if self._diag is None or self._diag[1].numel() < need:
            f64 = dict(dtype=torch.float64, device=self.device)
            self._diag = (torch.zeros(len(DIAG_SLOTS), **f64), torch.empty(need, **f64))
        sums, scratch = self._diag
        return ppo_diagnostics(self.H, src, idx, self.P, self.epsilon, self.max_action, sums, scratch, rows_out)

    def diagnostics_from(self, sums):
        """UpdateDiagnostics of host or device sums under the current log_std."""
        if torch.is_tensor(sums):
            sums = sums.cpu().numpy()
        o = self.off["ls"]
        return UpdateDiagnostics.from_sums(sums, self.P[o:o + 3].cpu().numpy(), self.entropy_coef)

    def diagnostics(self, src, idx=None, rows_out=None):
        """What the current parameters make of the packed rows src[idx] (idx
        None: every row) as an UpdateDiagnostics: the forward pass is the fused
        update's own (satrl_ppo_diagnostics), nothing of the learner changes.
        rows_out (optional) f32 [n, 4] receives ratio, log ratio, v, 0 per row.
        Reads the ten sums back (one host sync)."""
        return self.diagnostics_from(self.diagnostics_sums(src, idx, rows_out))

    def update_packed(self, src, total_steps, perms=None, generator=None, after_epoch=None):
        """K epochs of minibatch steps over the packed table src [B, 32]
        (adv already normalised), then lr decay (ppo_continuous.py:212-242).
        after_epoch (optional): after_epoch(ep, perm) runs after epoch ep's
        minibatches; a true return ends the epoch loop there (the permutations
        of the epochs not run are then never drawn).  The checks and the lr
        decay below run either way."""
        B = src.shape[0]
        self.sync_w2t()
        st = self.stepper(min(self.mini_batch_size, B))
        for ep in range(self.K_epochs):
            if perms is None:
                perm = torch.randperm(B, device=self.device, generator=generator)
            else:
                perm = perms(ep) if callable(perms) else perms[ep]     # a callable draws each epoch's order lazily
            st.run(src, perm)
            if after_epoch is not None and after_epoch(ep, perm):
                break
        if self.peer is not None:
            self.peer.check()                # a peer's value never arrived: the update is invalid
        if any(p.error_word for p in _update_plans(self.H, self.mini_batch_size, B)):
            rowpass_exchange_check()         # (a kernel's bounded wait ran out; bounded by the DP deadline)
        if self.use_lr_decay:
            self.lr_decay(total_steps)

    @staticmethod
    def pack(s, a, logp, adv, vt, out=None):
        B = s.shape[0]
        out = torch.empty((B, 32), dtype=torch.float32, device=s.device) if out is None else out
        out[:, 0:18] = s
        out[:, 18:21] = a
        out[:, 21:24] = logp
        out[:, 24] = adv.reshape(-1)
        out[:, 25] = vt.reshape(-1)
        out[:, 26:] = 0
        return out


class HostLearner:
    """The N = 1 drop-in's agent on host cores (device="cpu"; BASELINE.json
    configs[0]: CPPO_main.py on CPU, no GPU).  The networks are the same
    nn.Modules, stepped by torch's CPU autograd, clip_grad_norm_ and Adam in
    the order of ppo_continuous.py:212-239 (actor step, then critic step, per
    minibatch); the vectorised engine never uses it (its update is the HIP
    minibatch step of PPOLearner)."""

    def __init__(self, args, agent_idx):
        self.device = torch.device("cpu")
        self.actor = Actor_Gaussian(args, agent_idx)
        self.critic = Critic(args, agent_idx)
        self.lr_a, self.lr_c = args.lr_a, args.lr_c
        self.max_train_steps = args.max_train_steps
        self.K_epochs, self.epsilon, self.entropy_coef = args.K_epochs, args.epsilon, args.entropy_coef
        self.use_grad_clip, self.use_lr_decay, self.use_adv_norm = (args.use_grad_clip, args.use_lr_decay,
                                                                   args.use_adv_norm)
        kw = {"eps": 1e-5} if args.set_adam_eps else {}                  # ppo_continuous.py:161-166
        self.opts = (torch.optim.Adam(self.actor.parameters(), lr=self.lr_a, **kw),
                     torch.optim.Adam(self.critic.parameters(), lr=self.lr_c, **kw))

    def normalize_adv(self, adv):
        return (adv - adv.mean()) / (adv.std() + 1e-5) if self.use_adv_norm else adv

    def lr_decay(self, total_steps):
        frac = min(max(float(total_steps) / self.max_train_steps, 0.0), 1.0)    # as PPOLearner.lr_decay
        for opt, lr in zip(self.opts, (self.lr_a, self.lr_c)):
            for g in opt.param_groups:
                g["lr"] = lr * (1 - frac)

    @property
    def lr_now(self):
        return tuple(opt.param_groups[0]["lr"] for opt in self.opts)

    def _minibatch(self, rows):
        # contiguous column blocks, as the reference's s[index], a[index] ... are
        s, a, lp_old, adv, vt = (rows[:, lo:hi].contiguous() for lo, hi in ((0, 18), (18, 21), (21, 24), (24, 25),
                                                                             (25, 26)))
        dist = self.actor.get_dist(s)
        ent = dist.entropy().sum(1, keepdim=True)
        ratio = torch.exp(dist.log_prob(a).sum(1, keepdim=True) - lp_old.sum(1, keepdim=True))
        loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - self.epsilon, 1 + self.epsilon) * adv)
        losses = ((loss - self.entropy_coef * ent).mean(), lambda: F.mse_loss(vt, self.critic(s)))
        for k, (net, opt) in enumerate(zip((self.actor, self.critic), self.opts)):
            opt.zero_grad()
            (losses[0] if k == 0 else losses[1]()).backward()
            if self.use_grad_clip:
                torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
            opt.step()

    def update_packed(self, src, total_steps, perms):
        """K epochs over the packed rows [B, 32] in the given minibatch orders."""
        mb = self.mini_batch_size
        for ep in range(self.K_epochs):
            perm = perms[ep]
            for k in range(0, perm.numel(), mb):
                self._minibatch(src[perm[k:k + mb]])
        if self.use_lr_decay:
            self.lr_decay(total_steps)


def _gae_host(r, vs, vs_, dw, done, gamma, lamda):
    """ppo_continuous.py:198-208 on host arrays: f32 deltas, then the reverse
    scan with numpy-scalar arithmetic (f32, python floats weak) as the
    reference's loop runs it."""
    deltas = (r + gamma * (1.0 - dw) * vs_ - vs).reshape(-1).numpy()
    d = done.reshape(-1).numpy()
    adv = np.empty_like(deltas)
    g = 0
    for t in range(len(deltas) - 1, -1, -1):
        g = deltas[t] + gamma * lamda * g * (1.0 - d[t])
        adv[t] = g
    adv = torch.from_numpy(adv)
    return adv, adv + vs.reshape(-1)


class PPO_continuous:  # noqa: N801
    """Drop-in for ppo_continuous.PPO_continuous (ppo_continuous.py:136-258).

    Networks and optimizer live on the GPU.  ``choose_action`` draws its
    noise from torch's global CPU generator exactly as the reference's
    ``Normal.sample()`` does, and ``update`` draws its minibatch permutations
    from the same generator (BatchSampler(SubsetRandomSampler), drop_last
    False), so seeding and indexing match the reference bit for bit.
    """

    def __init__(self, args, agent_idx, device=None):
        if args.policy_dist != "Gaussian":
            raise NotImplementedError("only the Gaussian policy (CPPO_main.py:17 default) is on the hot path")
        self.policy_dist = args.policy_dist
        dev = device if device is not None else getattr(args, "device", None)
        if dev is not None and torch.device(dev).type == "cpu":
            self.L = HostLearner(args, agent_idx)          # device="cpu" only when asked (configs[0])
            self.L.mini_batch_size = args.mini_batch_size
        else:
            self.L = PPOLearner(args, agent_idx, device=device, graph_group=4)
        self.actor, self.critic = self.L.actor, self.L.critic
        self.max_action = args.max_action
        self.batch_size = args.batch_size
        self.mini_batch_size = args.mini_batch_size
        self.K_epochs = args.K_epochs
        self.gamma, self.lamda = args.gamma, args.lamda

    def _obs(self, s):
        return torch.as_tensor(np.asarray(s), dtype=torch.float32).reshape(1, -1).to(self.L.device)

    def evaluate(self, s):
        """ppo_continuous.py:168-174 (mean action)."""
        with torch.no_grad():
            return self.actor(self._obs(s)).cpu().numpy().flatten()

    def choose_action(self, s):
        """ppo_continuous.py:176-189."""
        with torch.no_grad():
            mean = self.actor(self._obs(s)).cpu()
            std = torch.exp(self.actor.log_std.detach().cpu().expand_as(mean))
            dist = torch.distributions.Normal(mean, std)
            a = dist.sample()
            a = torch.clamp(a, -self.max_action, self.max_action)
            a_logprob = dist.log_prob(a)
        return a.numpy().flatten(), a_logprob.numpy().flatten()

    def update(self, replay_buffer, total_steps):
        """ppo_continuous.py:191-242 on a flat ReplayBuffer."""
        from torch.utils.data.sampler import BatchSampler, SubsetRandomSampler
        dev = self.L.device
        s, a, a_logprob, r, s_, dw, done = [t.to(dev) for t in replay_buffer.numpy_to_tensor()]
        B = s.shape[0]
        with torch.no_grad():
            vs = self.critic(s)
            vs_ = self.critic(s_)
            gae_fn = _gae_host if isinstance(self.L, HostLearner) else _gae_explicit
            adv, v_target = gae_fn(r.reshape(-1), vs.reshape(-1), vs_.reshape(-1), dw.reshape(-1),
                                   done.reshape(-1), self.gamma, self.lamda)
            adv = adv.reshape(-1, 1)
            v_target = v_target.reshape(-1, 1)
            adv = self.L.normalize_adv(adv)
        src = PPOLearner.pack(s, a, a_logprob, adv, v_target)
        perms = []
        for _ in range(self.K_epochs):
            idx = [i for batch in BatchSampler(SubsetRandomSampler(range(B)), self.mini_batch_size, False)
                   for i in batch]
            perms.append(torch.tensor(idx, dtype=torch.int64, device=dev))
        self.L.update_packed(src, total_steps, perms=perms)

    def lr_decay(self, total_steps):
        self.L.lr_decay(total_steps)

    def save_checkpoint(self):
        self.actor.save_checkpoint()
        self.critic.save_checkpoint()

    def load_checkpoint(self):
        self.actor.load_checkpoint()
        self.critic.load_checkpoint()


def _gae_explicit(r, vs, vs_, dw, done, gamma, lamda):
    """General flat-buffer GAE with separate V(s') (dw != done boundaries):
    runs the HIP scan on a one-column buffer whose deltas already carry V(s')."""
    B = r.shape[0]
    # delta_t = r + g(1-dw)V(s') - V(s): feed r' = r + g(1-dw)V(s') - V(s) + V(s) ... keep the
    # reference order by computing deltas here, then scanning with V == 0.
    deltas = r + gamma * (1.0 - dw) * vs_ - vs
    zeros = torch.zeros(B + 1, 1, dtype=torch.float32, device=r.device)
    adv, _ = gae(deltas.reshape(B, 1).contiguous(), done.reshape(B, 1).to(torch.uint8).contiguous(), zeros,
                 gamma, lamda)
    adv = adv.reshape(-1)
    return adv, adv + vs
