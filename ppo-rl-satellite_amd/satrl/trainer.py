"""Training loops.

* ``args_param`` -- CPPO_main.py:13-65 config surface (every reference
  keyword, same defaults) plus the engine's keywords (num_envs, horizon,
  seed, rollout_graph_chunk, update_graph_group).
* ``train_pursuer_network`` / ``train_evader_network`` / ``test_network`` --
  CPPO_main.py:94-282 semantics over the drop-in N=1 classes.
* ``VecTrainer`` -- the vectorised engine: N envs x T steps per iteration,
  collected by hipGraph-captured chunks of [actor fwd -> HIP sample (x2
  agents) -> HIP env step], then critic values, HIP GAE scan, global
  advantage normalisation, and the graph-captured minibatch update.
  One process per GPU; with a process group the envs are sharded by global
  env id (Philox noise keyed by it, so rollouts do not depend on sharding)
  and gradients are averaged with RCCL.  Opt-in (reset_spread): every episode
  starts from a point drawn from a box, per env and episode.  Opt-in (obs_norm, reward_scaling):
  running observation normalisation and reward scaling, satrl/norm.py.
  ``VecTrainer.evaluate`` measures the current policies on a fresh env handle
  without touching any training state, satrl/evaluate.py.  Opt-in
  (diagnostics, target_kl): per-update loss / KL / clip-fraction figures in
  ``VecTrainer.diagnostics`` and the KL early stop of an update's epochs.
  Opt-in (opponent_pool): the frozen agent of a rollout acts, per 32-env
  block, with the live opponent or a stored earlier one, satrl/pool.py.
  ``VecTrainer.save_checkpoint`` / ``load_checkpoint`` (and ``train(...,
  checkpoint_every=k, checkpoint_path=p)``) write and read the whole state
  between two iterations: a fresh process continues with the bits of the
  run that never stopped, satrl/checkpoint.py.  Opt-in (scripted_opponent):
  an agent acts, whenever it is the frozen one, with a linear guidance law
  instead of its network, satrl/scripted.py.  Opt-in (league_laws,
  opponent_weighting): league play on top of the pool -- per 32-env block
  the live opponent, a stored one or one of several laws in one launch,
  per-member results tallied from the rollout itself (``league_table``) and
  stored opponents drawn by them (PFSP), DESIGN.md 3.2.3.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from . import dist as _dist
from . import norm as _norm
from . import pool as _pool
from . import scripted as _scripted
from .buffer import ReplayBuffer, RolloutBuffer
from .env import OBS_NOISE_KEYS, EnvError, VecSatellites, act_noise_spec, obs_noise_spec
from .ppo import (PPO_continuous, PPOLearner, gae, gaussian_sample, moments, policy_act, policy_act_league,
                  policy_act_pool, policy_act_scripted, policy_value, reduce_diagnostics_sums)


class args_param:  # noqa: N801
    """CPPO_main.py:13-65 (same keywords and defaults) + engine keywords."""

    def __init__(self, max_train_steps=int(3e6), evaluate_freq=5e3, save_freq=20, policy_dist="Gaussian",
                 batch_size=2048, mini_batch_size=64, hidden_width=256, hidden_width2=128, lr_a=0.0002, lr_c=0.0002,
                 gamma=0.99, lamda=0.95, epsilon=0.1, K_epochs=10, max_episode_steps=1000, use_adv_norm=True,
                 use_state_norm=True, use_reward_norm=False, use_reward_scaling=True, entropy_coef=0.01,
                 use_lr_decay=True, use_grad_clip=True, use_orthogonal_init=True, set_adam_eps=True, use_tanh=True,
                 chkpt_dir="/mnt/datab/home/yuanwenzheng/PICTURE1",
                 num_envs=1, horizon=None, seed=0, rollout_graph_chunk=64, update_graph_group=64, device=None,
                 surrogate=False, dp_minibatch="global", minibatch_sampler=None, allreduce="rccl",
                 obs_norm=False, reward_scaling=False, obs_clip=10.0, obs_norm_calib_steps=64,
                 diagnostics=False, diagnostics_rows=None, target_kl=None, reset_spread=None, reset_seed=None,
                 opponent_pool=0, opponent_latest_prob=0.5, opponent_snapshot_every=None, opponent_seed=None,
                 scripted_opponent=None, league_laws=None, league_law_prob=0.25, opponent_weighting="uniform",
                 pfsp_power=2, act_noise=None, act_noise_seed=None, obs_noise=None, obs_noise_seed=None):
        self.max_train_steps = max_train_steps
        self.evaluate_freq = evaluate_freq
        self.save_freq = save_freq
        self.policy_dist = policy_dist
        self.batch_size = batch_size
        self.mini_batch_size = mini_batch_size
        self.hidden_width = hidden_width
        self.hidden_width2 = hidden_width2
        self.lr_a = lr_a
        self.lr_c = lr_c
        self.gamma = gamma
        self.lamda = lamda
        self.epsilon = epsilon
        self.K_epochs = K_epochs
        self.use_adv_norm = use_adv_norm
        self.use_state_norm = use_state_norm
        self.use_reward_norm = use_reward_norm
        self.use_reward_scaling = use_reward_scaling
        self.entropy_coef = entropy_coef
        self.use_lr_decay = use_lr_decay
        self.use_grad_clip = use_grad_clip
        self.use_orthogonal_init = use_orthogonal_init
        self.set_adam_eps = set_adam_eps
        self.use_tanh = use_tanh
        self.max_episode_steps = max_episode_steps
        self.chkpt_dir = chkpt_dir
        # engine
        self.num_envs = num_envs
        self.horizon = horizon if horizon is not None else max(1, batch_size // max(1, num_envs))
        self.seed = seed
        self.rollout_graph_chunk = rollout_graph_chunk
        self.update_graph_group = update_graph_group
        self.device = device
        # config 5: evaluate the ImprovedNN surrogate (bf16) on every env step into
        # VecTrainer.ellipse_params (environment.py:158); True = the net trained on the
        # reference's golden pairs (satrl/data/improvednn_trained.npz, with its scalers);
        # a path or state_dict loads other weights
        self.surrogate = surrogate
        # data parallelism: "global" -- mini_batch_size is the
        # GLOBAL minibatch, each of W ranks steps mini_batch_size / W of its
        # rows per Adam step (the reference's minibatch semantics,
        # ppo_continuous.py:213); "per_gpu" -- every rank steps
        # mini_batch_size local rows (global minibatch mini_batch_size * W).
        self.dp_minibatch = dp_minibatch
        # minibatch index sampler of the vectorised engine: "uniform" =
        # BatchSampler(SubsetRandomSampler(range(B))) over the local table
        # (the reference's distribution); "stratified" = every minibatch holds
        # mini_batch_size / 8 rows of each of 8 fixed global env blocks, drawn
        # by per-block generators, so W = 1, 2, 4, 8 ranks draw the same
        # global minibatches (None: uniform on one process, stratified under
        # "global" data parallelism)
        self.minibatch_sampler = minibatch_sampler
        # the per-minibatch gradient all-reduce under data parallelism on GPUs:
        # "rccl" (ncclAllReduce + reduce_dp, in the update's graphs) or "peer"
        # (satrl_ppo_allreduce_peer: a two-shot reduce-scatter + all-gather
        # over IPC-mapped buffers, fused with reduce_dp; satrl/peer.py)
        self.allreduce = allreduce
        # running observation normalisation and reward scaling of the vectorised
        # engine (normalization.py's Normalization / RewardScaling, satrl/norm.py).
        # The reference's own use_state_norm / use_reward_norm / use_reward_scaling
        # above stay what they are there: printed and never read.  obs_norm: the
        # policy and the update see clamp((obs - mean) / (std + 1e-8), +-obs_clip)
        # under statistics frozen per iteration, first estimated over
        # obs_norm_calib_steps throw-away steps (0: start from the identity);
        # reward_scaling: GAE reads rew / (std of the running discounted return + 1e-8)
        self.obs_norm = obs_norm
        self.reward_scaling = reward_scaling
        self.obs_clip = obs_clip
        self.obs_norm_calib_steps = obs_norm_calib_steps
        # update diagnostics of the vectorised engine (VecTrainer.diagnostics: policy /
        # value loss, entropy, approximate KL, clip fraction, explained variance),
        # measured by a forward pass over the table after the update's last epoch;
        # diagnostics_rows: over the first that many rows of that epoch's
        # permutation instead of the whole table.  target_kl: measured after
        # every epoch, and the update's remaining epochs are skipped once
        # approx_kl > target_kl (implies diagnostics)
        self.diagnostics = diagnostics
        self.diagnostics_rows = diagnostics_rows
        self.target_kl = target_kl
        # randomised episode starts of the vectorised engine (include/satenv.h
        # satenv_reset_dist): None = the reference's fixed reset; 12 half-widths
        # (Pp, Pv, Ep, Ev; metres and m/s) around the reset's constants, or
        # {"lo": ..., "hi": ...} for the box itself.  Every reset, the in-kernel
        # autoreset included, then draws its start from the box, keyed by
        # (reset_seed, global env id, the env's episode index); reset_seed None = seed
        self.reset_spread = reset_spread
        self.reset_seed = reset_seed
        # actuation noise of the vectorised engine (include/satenv.h satenv_act_noise,
        # DESIGN.md 3.1.2): None = every commanded action is executed exactly; (mag, dir)
        # for both agents, or {"pursuer": (mag, dir), "evader": (mag, dir)} with either key
        # optional.  The env then executes each clipped action with a relative thrust
        # magnitude error in +-mag (mag <= 1) and a pointing error in +-dir * |a| per
        # component, keyed by (act_noise_seed, agent, global env id, the env's episode
        # index, the step count); act_noise_seed None = seed.  The buffer keeps the
        # commanded actions and their log-probs: the error is part of the environment
        act_noise_spec(act_noise)                                        # (raises on a malformed spec)
        self.act_noise = act_noise
        self.act_noise_seed = act_noise_seed
        # observation noise of the vectorised engine (include/satenv.h satenv_obs_noise,
        # DESIGN.md 3.1.3): None = both agents observe the exact state; (pos, vel) for both
        # tracked craft, or {"pursuer": c, "evader": c, "hold": h} with every key optional,
        # c = (pos, vel) or a dict with keys among bias_pos, bias_vel, pos, vel.  Every f32
        # observation row the env writes is then the row of the measured kinematics: each
        # scalar of a tracked craft off by a bias in +-bias_* held for the episode plus an
        # error in +-pos / +-vel redrawn every h steps, keyed by (obs_noise_seed, global env
        # id, the env's episode index, the step count); obs_noise_seed None = seed.  The
        # buffer, obs_norm, scripted laws and frozen opponents all read that one row;
        # rewards, dones and the env's state stay the truth
        obs_noise_spec(obs_noise)                                        # (raises on a malformed spec)
        self.obs_noise = obs_noise
        self.obs_noise_seed = obs_noise_seed
        # opponent pool of the vectorised engine's self-play (satrl/pool.py): per agent
        # a ring of opponent_pool stored parameter sets (0: off, nothing is allocated
        # and the rollout makes the calls it makes without it).  In every iteration
        # each 32-env block plays the live opponent with probability
        # opponent_latest_prob and else a uniformly drawn stored one, keyed by
        # (opponent_seed, iteration, global block); opponent_seed None = seed.  The
        # learner is stored at the end of every self_play phase and, with
        # opponent_snapshot_every = m, after every m-th iteration
        self.opponent_pool = int(opponent_pool)
        self.opponent_latest_prob = float(opponent_latest_prob)
        self.opponent_snapshot_every = None if opponent_snapshot_every is None else int(opponent_snapshot_every)
        self.opponent_seed = opponent_seed
        if self.opponent_pool < 0:
            raise ValueError(f"opponent_pool is the number of stored opponents (0: off), got {opponent_pool}")
        if not 0.0 <= self.opponent_latest_prob <= 1.0:                  # (NaN fails both comparisons)
            raise ValueError(f"opponent_latest_prob must be in [0, 1], got {opponent_latest_prob}")
        if self.opponent_snapshot_every is not None and self.opponent_snapshot_every <= 0:
            raise ValueError(f"opponent_snapshot_every must be positive or None, got {opponent_snapshot_every}")
        # scripted opponents of the vectorised engine (satrl/scripted.py): None, a mapping
        # {"evader": law, "pursuer": law} with either key optional, or a builder's name
        # ("coast", "intercept", "evade") / a ScriptedLaw as shorthand for {"evader": ...}.
        # An agent's law acts whenever that agent is the frozen one, on the raw
        # observation; its network, parameters and Adam state stay live, and set_flag /
        # self_play make it the learner as before
        self.scripted_opponent = _scripted.parse_opponents(scripted_opponent)
        if self.opponent_pool > 0 and self.scripted_opponent:
            raise ValueError("a scripted opponent and an opponent pool on the same agent are not supported "
                             "(opponent_pool stores both agents)")
        # league play of the vectorised engine: on top of the opponent
        # pool, league_laws = {"evader": [law, ...], "pursuer": [...]} (a ScriptedLaw or a
        # builder's name each, at most 8 per agent) are laws the frozen agent may also play,
        # per 32-env block: the live opponent with probability opponent_latest_prob, one of
        # the agent's laws with probability league_law_prob, else a stored one.
        # opponent_weighting "uniform" draws the stored one as the pool does; "pfsp" draws
        # slot k with weight (1 - p_k) ** pfsp_power, p_k the learner's smoothed win rate
        # against it in the rollouts so far (satrl/pool.py pfsp_weights)
        self.league_laws = _scripted.parse_league(league_laws)
        self.league_law_prob = float(league_law_prob)
        self.opponent_weighting = opponent_weighting
        self.pfsp_power = pfsp_power
        if self.league_laws and self.opponent_pool <= 0:
            raise ValueError("league_laws need opponent_pool > 0 (laws are league members beside the stored "
                             "opponents); one law in place of an agent's network is scripted_opponent")
        if not 0.0 <= self.league_law_prob <= 1.0:                       # (NaN fails both comparisons)
            raise ValueError(f"league_law_prob must be in [0, 1], got {league_law_prob}")
        if self.league_laws and self.opponent_latest_prob + self.league_law_prob > 1.0:
            raise ValueError(f"opponent_latest_prob + league_law_prob must not exceed 1, got "
                             f"{opponent_latest_prob} + {league_law_prob}")
        if opponent_weighting not in _scripted.LEAGUE_WEIGHTINGS:
            raise ValueError(f"opponent_weighting is one of {_scripted.LEAGUE_WEIGHTINGS}, got {opponent_weighting!r}")
        if isinstance(pfsp_power, bool) or not isinstance(pfsp_power, int) or pfsp_power <= 0:
            raise ValueError(f"pfsp_power is a positive int, got {pfsp_power!r}")
        if opponent_weighting == "pfsp" and self.opponent_pool <= 0:
            raise ValueError("opponent_weighting='pfsp' needs opponent_pool > 0")
        # set by the train_* functions from the env (CPPO_main.py:99-101)
        self.state_dim = 18
        self.action_dim = 3
        self.max_action = 1.6

    def print_information(self):
        for k, v in vars(self).items():
            print(f"{k}: {v}")


# ---------------------------------------------------------------------------
# reference loops (CPPO_main.py:94-282) on the drop-in N=1 classes
# ---------------------------------------------------------------------------
def _setup(args, env, d_capture):
    env.d_capture = d_capture                               # CPPO_main.py:98
    args.state_dim = env.observation_space.shape[0]
    args.action_dim = env.action_space.shape[0]
    args.max_action = float(env.action_space[0][1])


def _episode_loop(args, env, agents, learner, flag, stored_agent, update_agent, max_episodes, on_done=None):
    replay_buffer = ReplayBuffer(args)
    rewards, mean_rewards = [], []
    pursuer_agent, evader_agent = agents
    for epsiode in range(max_episodes):
        epsiode_reward = 0.0
        epsiode_count = 0
        s = env.reset(flag)
        while True:
            epsiode_count += 1
            pa, plp = pursuer_agent.choose_action(s)
            ea, elp = evader_agent.choose_action(s)
            s_, r, done = env.step(pa, ea, epsiode_count)
            epsiode_reward += r
            dw = bool(done or epsiode_count >= args.max_episode_steps)
            if stored_agent == "pursuer":
                replay_buffer.store(s, pa, plp, r, s_, dw, done)
            else:
                replay_buffer.store(s, ea, elp, r, s_, dw, done)
            s = s_
            if replay_buffer.count == args.batch_size:
                update_agent.update(replay_buffer, epsiode)
                replay_buffer.count = 0
            if done:
                rewards.append(epsiode_reward)
                mean_rewards.append(float(np.mean(rewards)))
                if on_done:
                    on_done(epsiode, epsiode_reward, mean_rewards[-1])
                break
    return rewards, mean_rewards


def train_pursuer_network(args, env, show_picture=False, pre_train=False, d_capture=0, max_episodes=None):
    """CPPO_main.py:94-161."""
    _setup(args, env, d_capture)
    pursuer_agent = PPO_continuous(args, "pursuer")
    evader_agent = PPO_continuous(args, "evader")
    if pre_train:
        pursuer_agent.load_checkpoint()
    n = args.max_train_steps if max_episodes is None else max_episodes
    rewards, means = _episode_loop(args, env, (pursuer_agent, evader_agent), pursuer_agent, 0, "pursuer",
                                   pursuer_agent, n)
    pursuer_agent.save_checkpoint()
    return pursuer_agent


def train_evader_network(args, env, show_picture=False, pre_train=False, d_capture=0, max_episodes=None,
                         fix_update_agent=False):
    """CPPO_main.py:163-230.  The reference updates ``pursuer_agent`` with the
    evader's transitions (CPPO_main.py:215); that is reproduced unless
    ``fix_update_agent`` is set."""
    _setup(args, env, d_capture)
    pursuer_agent = PPO_continuous(args, "pursuer")
    evader_agent = PPO_continuous(args, "evader")
    if pre_train:
        evader_agent.load_checkpoint()
    n = args.max_train_steps if max_episodes is None else max_episodes
    upd = evader_agent if fix_update_agent else pursuer_agent
    _episode_loop(args, env, (pursuer_agent, evader_agent), upd, 1, "evader", upd, n)
    evader_agent.save_checkpoint()
    return evader_agent


def test_network(args, env, show_pictures=False, d_capture=0):
    """CPPO_main.py:233-282; returns the episode return (the reference prints it)."""
    _setup(args, env, d_capture)
    pursuer_agent = PPO_continuous(args, "pursuer")
    evader_agent = PPO_continuous(args, "evader")
    pursuer_agent.load_checkpoint()
    epsiode_reward = 0.0
    epsiode_count = 0
    s = env.reset(0)
    while True:
        epsiode_count += 1
        pa, _ = pursuer_agent.choose_action(s)
        ea, _ = evader_agent.choose_action(s)
        s_, r, done = env.step(pa, ea, epsiode_count)
        epsiode_reward += r
        s = s_
        if done:
            print("当前测试得分为{}".format(epsiode_reward))
            return epsiode_reward


def train_elliptical_network(args, env, epsiodes=200, d_capture=0):
    """CPPO_main.py:284-322: Flag-2 episodes with the trained pursuer and an
    untrained evader acting; each env step fits the reachable-domain
    ellipse (GPU grid + fit kernels) and trains the env's ImprovedNN.  Note
    the reference never resets epsiode_count between episodes (:287, :301),
    so every episode after the first ends at its first step's timeout test."""
    env.d_capture = d_capture
    args.state_dim = env.observation_space.shape[0]
    args.action_dim = env.action_space.shape[0]
    args.max_action = float(env.action_space[0][1])
    pursuer_agent = PPO_continuous(args, "pursuer")
    evader_agent = PPO_continuous(args, "evader")
    pursuer_agent.load_checkpoint()
    epsiode_count = 0
    for _ in range(epsiodes):
        s = env.reset(2)
        while True:
            epsiode_count += 1
            pa, _ = pursuer_agent.choose_action(s)
            ea, _ = evader_agent.choose_action(s)
            if args.policy_dist == "Beta":
                pa = 2 * (pa - 0.5) * args.max_action
                ea = 2 * (ea - 0.5) * args.max_action
            s_, r, done = env.step(pa, ea, epsiode_count)
            s = s_
            if done:
                break


# ---------------------------------------------------------------------------
# vectorised engine
# ---------------------------------------------------------------------------
def stratified_epoch_perm(T, n_local, world, rank, global_mb, gens, strata=8, device=None):
    """One epoch's minibatch order for rank `rank` of `world`.

    The global table is [T, n_local * world] (row t * N_glob + global env),
    cut into `strata` blocks of consecutive global envs; rank r owns blocks
    [r * strata / world, (r + 1) * strata / world).  Block s draws its own
    permutation of its T * N_glob / strata rows from gens[s]; global
    minibatch k is the concatenation over blocks of their k-th chunk of
    global_mb / strata rows (the tail: the leftover rows of every block).  A
    rank returns its blocks' share in LOCAL rows (t * n_local + local env),
    minibatch-major, so every rank steps global_mb / world rows of each
    global minibatch and W = 1, 2, 4, 8 draw the same global minibatches."""
    Ns = n_local * world // strata
    Bs = T * Ns
    c = global_mb // strata
    nfull = Bs // c
    full, tail = [], []
    for s_ in range(rank * (strata // world), (rank + 1) * (strata // world)):
        q = torch.randperm(Bs, device=device, generator=gens[s_])
        t, e = q // Ns, q % Ns + (s_ * Ns - rank * n_local)
        loc = t * n_local + e
        full.append(loc[:nfull * c].view(nfull, c))
        tail.append(loc[nfull * c:])
    return torch.cat([torch.cat(full, 1).reshape(-1)] + tail)


class VecTrainer:
    """N envs x horizon T per iteration on one GPU (one process per GPU)."""

    def __init__(self, args, flag=0, d_capture=15000.0, device=None, pg=None, env_offset=0, use_graphs=True):
        self.args = args
        self.flag = int(flag)
        self.pg = pg
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.N = int(args.num_envs)
        self.T = int(args.horizon)
        self.env_offset = int(env_offset)
        self.seed = int(args.seed)
        self.obs_norm = bool(getattr(args, "obs_norm", False))
        self.reward_scaling = bool(getattr(args, "reward_scaling", False))
        if (self.obs_norm or self.reward_scaling) and pg is not None and (self.N % _norm.SLOT or
                                                                          self.env_offset % _norm.SLOT):
            # every rank holds whole accumulator slots (satrl/norm.py slot_total)
            raise ValueError(f"obs_norm / reward_scaling under data parallelism need num_envs % {_norm.SLOT} == 0 "
                             f"(got num_envs={self.N}, env_offset={self.env_offset})")
        args.state_dim, args.action_dim, args.max_action = 18, 3, 1.6
        self.env = VecSatellites(self.N, device=self.device, d_capture=d_capture,
                                 max_episode_steps=args.max_episode_steps, Flag=self.flag)
        torch.manual_seed(self.seed)                         # same init on every rank
        self.pursuer = PPOLearner(args, "pursuer", self.device, pg=pg, graph_group=args.update_graph_group,
                                  use_graph=use_graphs)
        self.evader = PPOLearner(args, "evader", self.device, pg=pg, graph_group=args.update_graph_group,
                                 use_graph=use_graphs)
        self.learner = self.pursuer if self.flag == 0 else self.evader
        if pg is not None:
            self._broadcast_params()
        self._setup_minibatches(args, pg)
        self.buf = RolloutBuffer(self.T, self.N, self.device)
        self.other_a = torch.zeros((self.N, 3), dtype=torch.float32, device=self.device)
        self.other_lp = torch.zeros((self.N, 3), dtype=torch.float32, device=self.device)
        self.step_base = torch.zeros(1, dtype=torch.int64, device=self.device)   # Philox step offset (u64 bits)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(self.seed * 1000003 + _dist.rank(pg))
        self.use_graphs = use_graphs
        self.chunk = max(1, min(int(args.rollout_graph_chunk), self.T))
        self._graphs = {}
        self._pool = None
        self.iteration_count = 0
        self.rollout_steps = 0
        self.episodes = 0.0
        self._in_iteration = False                           # between collect() and finish_iteration()
        self._loaded = False                                 # load_state_dict() ran: collect()'s warm-up keeps ep_return
        self.evaluations = []                                # train(evaluate_every=...): (iteration, episodes, summary)
        self._evaluators = {}                                # evaluate(): one cached VecEvaluator per num_envs
        tkl = getattr(args, "target_kl", None)
        self.target_kl = None if tkl is None else float(tkl)
        self.diagnostics_on = bool(getattr(args, "diagnostics", False)) or self.target_kl is not None
        rows = getattr(args, "diagnostics_rows", None)
        self.diagnostics_rows = None if rows is None else int(rows)
        if self.diagnostics_rows is not None and not 0 < self.diagnostics_rows <= self.T * self.N:
            raise ValueError(f"diagnostics_rows must be in 1..{self.T * self.N} (the local table), "
                             f"got {self.diagnostics_rows}")
        self.diagnostics = []                                # update(): one dict per update when diagnostics are on
        self.last_diagnostics = None
        self.surrogate = None
        self.ellipse_params = None
        if getattr(args, "surrogate", False):
            from .surrogate import Surrogate
            sd = args.surrogate if isinstance(args.surrogate, (str, dict)) else "trained"
            self.surrogate = Surrogate(device=self.device, seed=self.seed, state_dict=sd)
            self.ellipse_params = torch.zeros((self.N, 10), dtype=torch.float32, device=self.device)
        if self.obs_norm or self.reward_scaling:
            self._setup_norm(args)
        self.pools = None
        self.member = None
        self.last_assignment = None
        if int(getattr(args, "opponent_pool", 0)) > 0:
            self._setup_pools(args)
        self._laws = {}                                      # agent -> ScriptedLaw (satrl/scripted.py)
        for agent, law in dict(getattr(args, "scripted_opponent", None) or {}).items():
            self.set_scripted_opponent(agent, law)
        rs = getattr(args, "reset_seed", None)
        self.reset_seed = self.seed if rs is None else int(rs)
        self.set_reset_spread(getattr(args, "reset_spread", None))
        ans = getattr(args, "act_noise_seed", None)
        self.act_noise_seed = self.seed if ans is None else int(ans)
        self.set_act_noise(getattr(args, "act_noise", None))
        ons = getattr(args, "obs_noise_seed", None)
        self.obs_noise_seed = self.seed if ons is None else int(ons)
        self.set_obs_noise(getattr(args, "obs_noise", None))
        self._reset_obs()
        if self.obs_norm and int(getattr(args, "obs_norm_calib_steps", 64)) > 0:
            self._calibrate_obs_norm(int(args.obs_norm_calib_steps))

    # -- running normalisation (satrl/norm.py) ------------------------------------------
    def _setup_norm(self, args):
        """State of obs_norm / reward_scaling.  The accumulators are per 32-env
        slot (global env id // 32), so that their total does not depend on the
        sharding: under data parallelism every rank holds whole slots."""
        f64 = dict(dtype=torch.float64, device=self.device)
        slots = _norm.num_slots(self.N)
        self._first_slot = self.env_offset // _norm.SLOT if self.pg is not None else 0
        self._global_slots = slots * _dist.world_size(self.pg)
        if self.obs_norm:
            self.obs_clip = float(getattr(args, "obs_clip", 10.0))
            self.obs_rms = _norm.RunningMoments((18,))
            self.obs_raw = torch.zeros((self.N, 18), dtype=torch.float32, device=self.device)
            self.obs_stats = torch.zeros((2, 18), dtype=torch.float32, device=self.device)
            self.obs_pivot = torch.zeros(18, dtype=torch.float32, device=self.device)
            self.obs_acc = torch.zeros((slots, 2, 18), **f64)
            self._obs_acc_rows = 0                           # local rows summed into obs_acc
            self._write_obs_stats()
        if self.reward_scaling:
            self.ret_rms = _norm.RunningMoments(())
            self.ret_carry = torch.zeros(self.N, **f64)
            self.ret_acc = torch.zeros((slots, 2), **f64)
            self.rew_s = torch.zeros((self.T, self.N), dtype=torch.float32, device=self.device)

    def _write_obs_stats(self):
        """obs_rms -> the device statistics, in place (the captured rollout
        graphs read them on every replay); the pivot of the next sums is the
        mean in f32."""
        st = self.obs_rms.device_stats()
        self.obs_stats.copy_(torch.from_numpy(st))
        self.obs_pivot.copy_(torch.from_numpy(st[0].copy()))

    # -- opponent pool (satrl/pool.py) ----------------------------------------------------
    def _setup_pools(self, args):
        """State of opponent_pool: a pool per agent and the device member
        tensor, a block of 32 envs (global env id // 32) per entry, so that an
        assignment does not depend on the sharding: every rank holds whole
        blocks."""
        K = int(args.opponent_pool)
        if self.env_offset % _pool.BLOCK or (self.pg is not None and self.N % _pool.BLOCK):
            raise ValueError(f"opponent_pool needs env_offset % {_pool.BLOCK} == 0, and under data parallelism "
                             f"num_envs % {_pool.BLOCK} == 0 (got num_envs={self.N}, env_offset={self.env_offset})")
        seed = getattr(args, "opponent_seed", None)
        self.opponent_seed = self.seed if seed is None else int(seed)
        self.opponent_latest_prob = float(getattr(args, "opponent_latest_prob", 0.5))
        every = getattr(args, "opponent_snapshot_every", None)
        self.opponent_snapshot_every = None if every is None else int(every)
        self.pools = {"pursuer": _pool.OpponentPool(K, self.pursuer.H, self.device, self.opponent_seed),
                      "evader": _pool.OpponentPool(K, self.evader.H, self.device, self.opponent_seed)}
        self._n_blocks = (self.N + _pool.BLOCK - 1) // _pool.BLOCK
        self.member = torch.full((self._n_blocks,), -1, dtype=torch.int32, device=self.device)
        self.last_assignment = np.full(self._n_blocks, -1, dtype=np.int32)
        # league play: per agent a law table that never moves, and the
        # cumulative (episodes, captures) of the learner's rollouts against each member of
        # that agent's league: row 0 the live opponent, 1 + k stored slot k, 1 + K + j law j
        self.league_law_prob = float(getattr(args, "league_law_prob", 0.25))
        self.opponent_weighting = getattr(args, "opponent_weighting", "uniform")
        self.pfsp_power = int(getattr(args, "pfsp_power", 2))
        self._league = {k: _scripted.LawTable(self.device) for k in _scripted.AGENTS}
        self.league_counts = {k: np.zeros((1 + K + _scripted.LEAGUE_MAX_LAWS, 2), dtype=np.int64)
                              for k in _scripted.AGENTS}
        self._tally = torch.zeros((self._n_blocks, 2), dtype=torch.int64, device=self.device)
        self._tally_pending = False
        for agent, laws in dict(getattr(args, "league_laws", None) or {}).items():
            # (copies: one args object may build several trainers, and a law lives in one table)
            self.set_league_laws(agent, [_scripted.ScriptedLaw.from_state(x.state()) for x in laws])

    @property
    def frozen_agent(self):
        """The agent that does not learn under the current Flag."""
        return "evader" if self.flag == 0 else "pursuer"

    def _assign_opponents(self):
        """This iteration's member of every local block, over the frozen
        agent's pool (and, in league play, its laws): written into the member
        tensor in place and stream-ordered (the captured rollout graphs read it
        on every replay)."""
        pool = self.pools[self.frozen_agent]
        n_laws = len(self._league[self.frozen_agent])
        first = self.env_offset // _pool.BLOCK
        if n_laws or self.opponent_weighting == "pfsp":
            w = self._pfsp_weights() if self.opponent_weighting == "pfsp" and pool.filled else None
            a = _pool.league_assign(pool.seed, self.iteration_count, first, self._n_blocks, pool.K, pool.filled, n_laws,
                                    self.opponent_latest_prob, self.league_law_prob if n_laws else 0.0, w)
        else:
            a = pool.assign(self.iteration_count, first, self._n_blocks, self.opponent_latest_prob)
        self.member.copy_(torch.from_numpy(a))
        self.last_assignment = a

    # -- league play -----------------------------------------------------
    def league_laws(self, agent=None):
        """The ScriptedLaw objects of `agent`'s (default: the frozen agent's)
        league, in law order: ScriptedLaw.update on one of them is followed by
        the captured rollout graphs."""
        if self.pools is None:
            raise ValueError("no league: build the trainer with args.opponent_pool > 0")
        return list(self._league[self._league_agent(agent)].laws)

    def _league_agent(self, agent):
        agent = self.frozen_agent if agent is None else agent
        if agent not in _scripted.AGENTS:
            raise ValueError(f"agent is one of {_scripted.AGENTS}, got {agent!r}")
        return agent

    def set_league_laws(self, agent, laws):
        """`agent`'s ("pursuer" | "evader") league laws: a list of ScriptedLaw
        objects or builders' names, at most 8; an empty list or None detaches
        them.  The laws' values go into the agent's law table in place and
        their device blocks become rows of it.  The captured rollout graphs
        are dropped only when the agent's law count goes between zero and
        non-zero (the launch changes); the cumulative counts of the agent's
        law members start again at zero.  A law that already owns a device
        block (it was used elsewhere) is refused: pass a copy."""
        if self.pools is None:
            raise ValueError("league laws need an opponent pool (args.opponent_pool > 0); one law in place of an "
                             "agent's network is set_scripted_opponent")
        agent = self._league_agent(agent)
        tab = self._league[agent]
        had = len(tab)
        laws = [laws] if isinstance(laws, (str, _scripted.ScriptedLaw)) else list(laws or [])
        if laws and self.opponent_latest_prob + self.league_law_prob > 1.0:
            raise ValueError(f"opponent_latest_prob + league_law_prob must not exceed 1, got "
                             f"{self.opponent_latest_prob} + {self.league_law_prob}")
        tab.set(laws)                                # (validates everything before it changes anything)
        for ev in self._evaluators.values():         # their graphs hold law blocks that may have moved
            ev._graphs.clear()
            ev._laws.clear()
        self.league_counts[agent][1 + self.pools[agent].K:] = 0
        if bool(had) != bool(len(tab)):
            self._graphs.clear()

    def _learner_wins(self, counts):
        """The learner's wins out of rows (episodes, captures): the pursuer's
        are the captures, the evader's the episodes that ended otherwise."""
        return counts[:, 1] if self.flag == 0 else counts[:, 0] - counts[:, 1]

    def _pfsp_weights(self):
        """PFSP weights of the frozen agent's filled slots from the counts of
        the finished iterations: the same on every rank and for every sharding."""
        pool = self.pools[self.frozen_agent]
        c = self.league_counts[self.frozen_agent][1:1 + pool.filled]
        return _pool.pfsp_weights(c[:, 0], self._learner_wins(c), self.pfsp_power)

    def _run_tally(self):
        """After a rollout: this iteration's (episodes, captures) per local
        block, on the stream; finish_iteration folds them."""
        from .evaluate import capture_reward_of
        self._tally.zero_()
        _pool.league_tally(self.buf.rew, self.buf.done, capture_reward_of(self.env._p, self.flag), self._tally)
        self._tally_pending = True

    def _fold_tally(self):
        """The iteration's per-block counts, by last_assignment, into the
        cumulative per-member counts of the frozen agent's league (summed over
        ranks first: integers, exact)."""
        K = self.pools[self.frozen_agent].K
        rows = 1 + K + _scripted.LEAGUE_MAX_LAWS
        a = self.last_assignment.astype(np.int64)
        idx = np.where((a >= 0) & (a < rows - 1), a + 1, 0)
        local = np.zeros((rows, 2), dtype=np.int64)
        np.add.at(local, idx, self._tally.cpu().numpy())
        if self.pg is not None:
            local = _dist.sum_(torch.from_numpy(local).to(self.device), self.pg).cpu().numpy()
        self.league_counts[self.frozen_agent] += local
        self._tally_pending = False

    def league_table(self, agent=None):
        """The learner's rollout results against each member of `agent`'s
        (default: the frozen agent's) league, cumulative over the finished
        iterations: rows (member code, "live" | "stored" | "law", meta,
        episodes, captures) for the live opponent (-1), every filled slot k
        and every law (K + j).  A stored slot's counts start again when the
        ring overwrites it."""
        if self.pools is None:
            raise ValueError("no league: build the trainer with args.opponent_pool > 0")
        agent = self._league_agent(agent)
        pool, c = self.pools[agent], self.league_counts[agent]
        rows = [(-1, "live", {"agent": agent}, int(c[0, 0]), int(c[0, 1]))]
        rows += [(k, "stored", dict(pool.metas[k] or {}), int(c[1 + k, 0]), int(c[1 + k, 1]))
                 for k in range(pool.filled)]
        rows += [(pool.K + j, "law", {"agent": agent, "law": j}, int(c[1 + pool.K + j, 0]), int(c[1 + pool.K + j, 1]))
                 for j in range(len(self._league[agent]))]
        return rows

    def snapshot_opponent(self, agent=None):
        """Store `agent`'s ("pursuer" | "evader"; default: the learner's)
        current parameters in that agent's pool; returns the slot.  Under data
        parallelism every rank holds the same parameters and stores them
        locally."""
        if self.pools is None:
            raise ValueError("no opponent pool: build the trainer with args.opponent_pool > 0")
        if agent is None:
            agent = "pursuer" if self.learner is self.pursuer else "evader"
        if agent not in self.pools:
            raise ValueError("agent is 'pursuer' or 'evader'")
        L = self.pursuer if agent == "pursuer" else self.evader
        k = self.pools[agent].add(L.P, {"agent": agent, "iteration_count": self.iteration_count,
                                        "episodes": self.episodes})
        self.league_counts[agent][1 + k] = 0         # the ring overwrote the slot: its results were the old set's
        return k

    def pool_state(self):
        """Both pools as CPU tensors with their metas and ring cursors."""
        if self.pools is None:
            raise ValueError("no opponent pool: build the trainer with args.opponent_pool > 0")
        return {k: p.state() for k, p in self.pools.items()}

    def load_pool_state(self, d):
        """Restore pool_state(), in place: captured rollout graphs stay valid."""
        if self.pools is None:
            raise ValueError("no opponent pool: build the trainer with args.opponent_pool > 0")
        for k, p in self.pools.items():
            if d.get(k) is None:
                raise ValueError(f"no {k} pool in this state")
            p.load_state(d[k])

    # -- scripted opponents (satrl/scripted.py) ------------------------------------------------
    @property
    def scripted_opponents(self):
        """{agent: ScriptedLaw} of the agents that act with a law while frozen."""
        return dict(self._laws)

    def set_scripted_opponent(self, agent, law):
        """Attach `law` (a ScriptedLaw, a builder's name, or None to detach) to
        `agent` ("pursuer" | "evader"): the agent acts with it whenever it is
        the frozen one.  Attaching, detaching or replacing the law object drops
        the captured rollout graphs (they hold the launch and the block's
        address); changing an attached law's values (ScriptedLaw.update) never
        does.  The curriculum hook: train against a law, detach it, go on with
        self-play."""
        if agent not in _scripted.AGENTS:
            raise ValueError(f"agent is one of {_scripted.AGENTS}, got {agent!r}")
        if law is not None:
            law = _scripted.as_law(law)
            if self.pools is not None:
                raise ValueError("a scripted opponent and an opponent pool on the same agent are not supported "
                                 "(opponent_pool stores both agents)")
            law.block(self.device)
        if self._laws.get(agent) is law:
            return
        if law is None:
            del self._laws[agent]
        else:
            self._laws[agent] = law
        self._graphs.clear()

    def set_reset_spread(self, spread, seed=None):
        """The box the env's resets draw their starts from (args_param
        reset_spread; None: the reference's fixed reset), keyed by `seed`
        (default: the current reset seed) and this rank's env_offset.  The
        env reads it where it resets, so it holds from the next reset on; the
        captured rollout graphs are replayed as they are.  (Only the first
        box of a trainer built without one drops them: they hold the step
        kernel without the draw, VecSatellites.set_reset_dist.)"""
        from .env import reset_box
        if seed is not None:
            self.reset_seed = int(seed)
        box = reset_box(spread)
        self.reset_spread = spread
        if box is None:
            self.env.clear_reset_dist()
            return
        drew = self.env.draws
        self.env.set_reset_dist(box[0], box[1], self.reset_seed, env_offset=self.env_offset)
        if not drew:
            self._graphs.clear()

    def set_act_noise(self, spec, seed=None):
        """The env's actuation noise (args_param act_noise; None: every action
        is executed exactly), keyed by `seed` (default: the current noise seed)
        and this rank's env_offset, so data-parallel shards draw by global env
        id.  It holds from the next step on; the captured rollout graphs are
        replayed as they are.  (Only the first spec of a trainer built without
        one drops them: they hold the step kernel without the noise,
        VecSatellites.set_act_noise.)"""
        if seed is not None:
            self.act_noise_seed = int(seed)
        pair = act_noise_spec(spec)
        self.act_noise = spec
        if pair is None:
            self.env.clear_act_noise()
            return
        was = self.env.noisy
        self.env.set_act_noise(pair[0], pair[1], self.act_noise_seed, env_offset=self.env_offset)
        if not was:
            self._graphs.clear()

    def set_obs_noise(self, spec, seed=None):
        """The env's observation noise (args_param obs_noise; None: exact
        observations), keyed by `seed` (default: the current noise seed) and
        this rank's env_offset, so data-parallel shards draw by global env id.
        It holds from the next observation the env writes on (buf.obs[0], the
        row in flight, stays as it was written); the captured rollout graphs
        are replayed as they are.  (Only the first spec of a trainer built
        without one drops them: they hold the step kernel without the
        measurement, VecSatellites.set_obs_noise.)"""
        if seed is not None:
            self.obs_noise_seed = int(seed)
        norm = obs_noise_spec(spec)
        self.obs_noise = spec
        if norm is None:
            self.env.clear_obs_noise()
            return
        was = self.env.measures
        self.env.set_obs_noise(*(dict(zip(OBS_NOISE_KEYS, c)) for c in norm[:2]), hold=norm[2],
                               seed=self.obs_noise_seed, env_offset=self.env_offset)
        if not was:
            self._graphs.clear()

    def _reset_obs(self):
        """Every env restarts; buf.obs[0] is the (normalised) reset observation.
        ellipse_params is zeroed: the surrogate has not run on the reset state
        (it runs after every env step), and the rows of the states before the
        restart describe no env any more."""
        if self.ellipse_params is not None:
            self.ellipse_params.zero_()
        if not self.obs_norm:
            self.env.reset(self.flag, obs_out=self.buf.obs[0])
            return
        self.env.reset(self.flag, obs_out=self.obs_raw)
        _norm.obs_normalize(self.obs_raw, self.obs_stats, self.obs_clip, self.buf.obs[0])

    def _fold_obs_stats(self):
        """The iteration's slot sums -> obs_rms -> the device statistics; obs_acc is zeroed."""
        tot = _norm.slot_total(self.obs_acc, self.pg, self._first_slot, self._global_slots)
        self.obs_rms.merge_shifted(self._obs_acc_rows * _dist.world_size(self.pg), tot[0], tot[1],
                                   self.obs_pivot.cpu().numpy())
        self._write_obs_stats()
        self.obs_acc.zero_()
        self._obs_acc_rows = 0

    def _calibrate_obs_norm(self, steps):
        """First statistics from `steps` eager throw-away steps under the
        identity (mean 0, inv_std 1) with the reset observation's row 0 as the
        pivot; the env state, its episode indices (so the calibration does not
        shift which starts the training draws), env.stats and the step
        counters are restored."""
        piv = self.obs_raw[0].clone()
        _dist.broadcast_([piv], self.pg)
        self.obs_pivot.copy_(piv)
        f, i = self.env.get_state()
        ep = self.env.episode_index()
        st, raw0 = self.env.stats.clone(), self.obs_raw.clone()
        for s_ in range(steps):
            self.step_base.fill_(s_)
            self._policy_step(0)
            self.buf.obs[0].copy_(self.buf.obs[1])
        self._obs_acc_rows += steps * self.N
        self.env.set_state(f, i)
        self.env.set_episode_index(ep)
        self.env.stats.copy_(st)
        self.obs_raw.copy_(raw0)
        self.step_base.zero_()
        if self.ellipse_params is not None:
            self.ellipse_params.zero_()
        self._fold_obs_stats()
        _norm.obs_normalize(self.obs_raw, self.obs_stats, self.obs_clip, self.buf.obs[0])

    def normalize_obs(self, raw, out=None):
        """Raw observations f32 [n, 18] as the policy sees them under the
        current statistics (the identity without obs_norm)."""
        if not self.obs_norm:
            return raw if out is None else out.copy_(raw)
        out = torch.empty_like(raw) if out is None else out
        return _norm.obs_normalize(raw, self.obs_stats, self.obs_clip, out)

    def norm_state(self):
        """The running statistics as numpy arrays: a policy trained with
        obs_norm is meaningless without them."""
        return {"obs": self.obs_rms.state_dict() if self.obs_norm else None,
                "ret": self.ret_rms.state_dict() if self.reward_scaling else None,
                "carry": self.ret_carry.cpu().numpy() if self.reward_scaling else None}

    def load_norm_state(self, d):
        """Restore norm_state() and rewrite the device tensors; buf.obs[0] is
        normalised again from the current raw observation."""
        if self.obs_norm:
            if d.get("obs") is None:
                raise ValueError("no observation statistics in this state (obs_norm is on)")
            self.obs_rms.load_state_dict(d["obs"])
            self._write_obs_stats()
            _norm.obs_normalize(self.obs_raw, self.obs_stats, self.obs_clip, self.buf.obs[0])
        if self.reward_scaling:
            if d.get("ret") is None or d.get("carry") is None:
                raise ValueError("no return statistics in this state (reward_scaling is on)")
            self.ret_rms.load_state_dict(d["ret"])
            carry = torch.from_numpy(np.ascontiguousarray(d["carry"], dtype=np.float64))
            if tuple(carry.shape) != (self.N,):
                raise ValueError(f"carry of shape {tuple(carry.shape)} for {self.N} envs")
            self.ret_carry.copy_(carry)

    STRATA = 8

    def _setup_minibatches(self, args, pg):
        """Local minibatch size and index sampler (see args_param
        dp_minibatch / minibatch_sampler)."""
        W, r = _dist.world_size(pg), _dist.rank(pg)
        mode = getattr(args, "dp_minibatch", "global")
        if mode not in ("global", "per_gpu"):
            raise ValueError("dp_minibatch must be 'global' or 'per_gpu'")
        sampler = getattr(args, "minibatch_sampler", None)
        if sampler is None:
            sampler = "stratified" if (W > 1 and mode == "global") else "uniform"
        if sampler not in ("uniform", "stratified"):
            raise ValueError("minibatch_sampler must be 'uniform' or 'stratified'")
        mb = int(args.mini_batch_size)
        if W > 1 and mode == "global" and sampler != "stratified":
            raise ValueError("global-minibatch data parallelism draws stratified minibatches")
        self.world, self.rank = W, r
        self.dp_minibatch, self.sampler = mode, sampler
        self.global_minibatch = mb if mode == "global" else mb * W
        self.mb_local = mb // W if mode == "global" else mb
        if sampler == "stratified":
            S = self.STRATA
            if S % W or (self.N * W) % S or mb % S or (mode == "global" and mb % W):
                raise ValueError(f"stratified minibatches need world size | {S}, {S} | num_envs*world and "
                                 f"{S} | mini_batch_size (got W={W}, num_envs={self.N}, mb={mb})")
            self.my_strata = list(range(r * (S // W), (r + 1) * (S // W)))
            self.strata_gen = {}
            for s_ in self.my_strata:                # the same stream for a block whatever rank owns it
                g = torch.Generator(device=self.device)
                g.manual_seed(self.seed * 1000003 + 7919 * (s_ + 1))
                self.strata_gen[s_] = g
        for L in (self.pursuer, self.evader):
            L.mini_batch_size = self.mb_local

    def epoch_perm(self):
        """One epoch's minibatch order over the local packed table [T*N]
        (row t*N + j), minibatch-major: the full minibatches of mb_local rows,
        then the tail (BatchSampler drop_last=False)."""
        B = self.T * self.N
        if self.sampler == "uniform":
            return torch.randperm(B, device=self.device, generator=self.gen)
        return stratified_epoch_perm(self.T, self.N, self.world, self.rank, self.global_minibatch, self.strata_gen,
                                     self.STRATA, self.device)

    def _broadcast_params(self):
        # the module parameters are views into each learner's flat P
        _dist.broadcast_([self.pursuer.P, self.evader.P], self.pg)
        self.pursuer.sync_w2t()
        self.evader.sync_w2t()

    # -- rollout ------------------------------------------------------------------
    def _policy_step(self, t, events=None, env=True):
        """One step of CPPO_main.py:121-147 for all envs (no host sync).
        Bench-only knobs: `events` (a pair of torch.cuda.Event) around the env
        step; env=False skips the env step (timing only)."""
        buf = self.buf
        obs_t = buf.obs[t]
        if self.flag == 0:                       # pursuer transitions are stored (CPPO_main.py:141)
            pa, plp, ea, elp = buf.act[t], buf.logp[t], self.other_a, self.other_lp
        else:                                    # evader transitions are stored (CPPO_main.py:210)
            pa, plp, ea, elp = self.other_a, self.other_lp, buf.act[t], buf.logp[t]
        # both agents act on s (CPPO_main.py:122-123): one fused launch, pursuer = agent 0
        law = self._laws.get(self.frozen_agent)
        if law is not None:                      # the frozen agent's law on the raw row, the learner's MLP alone
            policy_act_scripted(self.learner.H, obs_t, self.obs_raw if self.obs_norm else obs_t, self.learner.P,
                                self.flag, 1.6, self.seed, self.env_offset, t, buf.act[t], buf.logp[t], law,
                                self.other_a, step_base=self.step_base)
        elif self.pools is None:
            policy_act(self.pursuer.H, obs_t, self.pursuer.P, self.evader.P, 1.6, self.seed, self.env_offset, t,
                       pa, plp, ea, elp, step_base=self.step_base)
        elif len(self._league[self.frozen_agent]):   # ... with its member of the league: a stored set or a law
            policy_act_league(self.pursuer.H, obs_t, self.obs_raw if self.obs_norm else obs_t, self.pursuer.P,
                              self.evader.P, 1.6, self.seed, self.env_offset, t, pa, plp, ea, elp, 1 - self.flag,
                              self.pools[self.frozen_agent].storage, self.member, self._league[self.frozen_agent],
                              step_base=self.step_base)
        else:                                    # the frozen agent acts, per 32-env block, with its member of the pool
            policy_act_pool(self.pursuer.H, obs_t, self.pursuer.P, self.evader.P, 1.6, self.seed, self.env_offset, t,
                            pa, plp, ea, elp, 1 - self.flag, self.pools[self.frozen_agent].storage, self.member,
                            step_base=self.step_base)
        if events is not None:
            events[0].record()
        if env:
            if self.obs_norm:                    # raw row -> the fixed scratch, normalised into the buffer
                self.env.step_autoreset(pa, ea, obs_out=self.obs_raw, reward_out=buf.rew[t], done_out=buf.done[t])
                _norm.obs_normalize(self.obs_raw, self.obs_stats, self.obs_clip, buf.obs[t + 1], self.obs_pivot,
                                    self.obs_acc)
            else:
                self.env.step_autoreset(pa, ea, obs_out=buf.obs[t + 1], reward_out=buf.rew[t], done_out=buf.done[t])
        if events is not None:
            events[1].record()
        if self.surrogate is not None:            # env.ellipse_params of the state the policy sees next
            self.surrogate.env_forward(self.env, out=self.ellipse_params)

    def set_flag(self, flag):
        """Switch the learning agent (Flag 0: pursuer, CPPO_main.py:94-161;
        Flag 1: evader, CPPO_main.py:163-230).  Every env restarts under the
        new Flag; rollout graphs are cached per Flag (they route the learner's
        actions into the buffer)."""
        flag = int(flag)
        if flag not in (0, 1):
            raise ValueError("Flag 0 (pursuer) or 1 (evader)")
        self.flag = flag
        self.learner = self.pursuer if flag == 0 else self.evader
        self._reset_obs()

    def self_play(self, phases, iterations_per_phase, timers=None, checkpoint_every=None, checkpoint_path=None):
        """Alternating training (the reference's Sign == 0 runs
        train_pursuer_network then train_evader_network, CPPO_main.py:336-338):
        `phases` phases of `iterations_per_phase` iterations, starting with the
        current Flag.  Returns the per-iteration statistics.  With an opponent
        pool the learner is stored in its pool at the end of every phase.
        checkpoint_path with checkpoint_every=k: save_checkpoint after every
        k-th iteration of this call and after the last one (a phase's last
        iteration: after the learner is stored); the saved Flag and
        iteration_count tell a resumed caller which phases remain."""
        out = []
        n = int(iterations_per_phase)
        for k in range(int(phases)):
            if k:
                self.set_flag(1 - self.flag)
            for j in range(n):
                out.append((self.flag, self.iteration(timers)))
                if j + 1 < n:
                    self._checkpoint_if_due(len(out), checkpoint_every, checkpoint_path)
            if self.pools is not None:
                self.snapshot_opponent()
            if n:
                self._checkpoint_if_due(len(out), checkpoint_every, checkpoint_path, force=k + 1 == int(phases))
        return out

    def _chunk_graph(self, c):
        key = (self.flag, c)
        if key not in self._graphs:
            t0 = c * self.chunk
            t1 = min(self.T, t0 + self.chunk)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            with torch.cuda.graph(g, pool=self._pool):
                for t in range(t0, t1):
                    self._policy_step(t)
            self._graphs[key] = g
        return self._graphs[key]

    def collect(self):
        """T environment steps for all N envs (CPPO_main.py:119-147)."""
        self._in_iteration = True
        self.step_base.fill_(self.rollout_steps)
        if self.pools is not None:
            self._assign_opponents()
        nchunks = (self.T + self.chunk - 1) // self.chunk
        if self.use_graphs:
            if not self._graphs:
                # eager warm-up of one step so lazy allocations happen before capture
                # (restores the env state afterwards).  A trainer that loaded a state
                # runs it in the middle of a run and restores the running episode
                # returns too; a fresh trainer's first warm-up leaves its reward in
                # them, as it always has
                f, i = self.env.get_state()
                ep = self.env.episode_index()
                st = self.env.stats.clone()
                ret = self.env.episode_return() if self._loaded else None
                raw = self.obs_raw.clone() if self.obs_norm else None    # step 0's raw row: a scripted law reads it
                self._policy_step(0)
                if raw is not None:
                    self.obs_raw.copy_(raw)
                self.env.set_state(f, i)
                self.env.set_episode_index(ep)
                self.env.stats.copy_(st)
                if ret is not None:
                    self.env.set_episode_return(ret)
                if self.obs_norm:                # the warm-up row is not part of the iteration's sums
                    self.obs_acc.zero_()
                torch.cuda.synchronize()
            for c in range(nchunks):
                self._chunk_graph(c).replay()
        else:
            for t in range(self.T):
                self._policy_step(t)
        self.rollout_steps += self.T
        if self.obs_norm:
            self._obs_acc_rows += self.T * self.N
        if self.pools is not None:
            self._run_tally()

    # -- learning -----------------------------------------------------------------
    def compute_advantages(self, chunk_steps=64):
        buf, L = self.buf, self.learner
        with torch.no_grad():
            policy_value(L.H, buf.obs.view(-1, 18), L.P, buf.values.view(-1))     # critic(s), all T+1 rows
            gae(self._scaled_rewards() if self.reward_scaling else buf.rew, buf.done, buf.values, L.gamma, L.lamda,
                adv_out=buf.adv, vt_out=buf.vtarget)
            adv_n = L.normalize_adv(buf.adv.reshape(-1))
            buf.pack(adv_n)

    def _scaled_rewards(self):
        """RewardScaling (normalization.py:50-63) over the iteration: the
        running discounted return of every env is scanned forward (R = 0 after
        a done step), its moments are merged into ret_rms, and GAE reads
        rew / (std + 1e-8).  buf.rew and the env's episode statistics stay raw."""
        buf = self.buf
        _norm.return_scan(buf.rew, buf.done, self.learner.gamma, self.ret_carry, self.ret_acc)
        tot = _norm.slot_total(self.ret_acc, self.pg, self._first_slot, self._global_slots)
        self.ret_acc.zero_()
        self.ret_rms.merge_shifted(self.T * self.N * _dist.world_size(self.pg), tot[0], tot[1], 0.0)
        scale = np.float32(1.0 / (float(self.ret_rms.std()) + _norm.EPS))
        torch.mul(buf.rew, float(scale), out=self.rew_s)
        return self.rew_s

    def update(self):
        if not self.diagnostics_on:
            self.learner.update_packed(self.buf.packed, self.episodes, perms=lambda ep: self.epoch_perm())
            return
        self._update_with_diagnostics()

    def _explained_variance(self):
        """The pre-update 1 - Var(v_target - V_old) / Var(v_target) over every
        rank's rows (population variances; buf.adv is the raw advantage
        v_target - V_old); NaN when Var(v_target) = 0."""
        buf = self.buf
        n = torch.tensor([float(buf.adv.numel())], dtype=torch.float64, device=self.device)
        m = _dist.sum_(torch.cat([moments(buf.adv), moments(buf.vtarget), n]), self.pg).cpu().tolist()
        var_adv = m[1] / m[4] - (m[0] / m[4]) ** 2
        var_vt = m[3] / m[4] - (m[2] / m[4]) ** 2
        return 1.0 - var_adv / var_vt if var_vt > 0 else float("nan")

    def _update_with_diagnostics(self):
        """update() with args.diagnostics / target_kl: the same minibatch
        steps, and after the last epoch run (with target_kl: after every epoch)
        learner.diagnostics over the table, or over the first diagnostics_rows
        rows of that epoch's permutation.  These are whole-set figures under
        the parameters after the epoch, not means over the minibatches during
        it.  With target_kl the epoch loop ends once approx_kl > target_kl (the
        plain comparison); the epochs not run draw no permutation, so the
        minibatch generator is then left in an earlier state than a full update
        leaves it.  Under a process group the sums are reduced over the ranks
        first: every rank records and decides the same.  Appends a dict to
        self.diagnostics; touches nothing the training reads."""
        L, buf = self.learner, self.buf
        ev_before = self._explained_variance()
        state = {"epochs": 0, "diag": None}

        def after_epoch(ep, perm):
            state["epochs"] = ep + 1
            if self.target_kl is None and ep + 1 < L.K_epochs:
                return False
            idx = None if self.diagnostics_rows is None else perm[:self.diagnostics_rows]
            sums = reduce_diagnostics_sums(L.diagnostics_sums(buf.packed, idx), self.pg)
            state["diag"] = L.diagnostics_from(sums)
            return self.target_kl is not None and state["diag"].approx_kl > self.target_kl

        L.update_packed(buf.packed, self.episodes, perms=lambda ep: self.epoch_perm(), after_epoch=after_epoch)
        rec = {"iteration_count": self.iteration_count, "episodes": self.episodes, "epochs_run": state["epochs"],
               "explained_variance": ev_before}
        rec.update(state["diag"].as_dict())
        self.diagnostics.append(rec)
        self.last_diagnostics = rec

    def finish_iteration(self):
        # next rollout starts from the current observation
        if self.obs_norm:                        # ... seen under the statistics the next iteration freezes
            self._fold_obs_stats()
            _norm.obs_normalize(self.obs_raw, self.obs_stats, self.obs_clip, self.buf.obs[0])
        else:
            self.buf.obs[0].copy_(self.buf.obs[self.T])
        st = _dist.sum_(self.env.stats, self.pg)
        self.episodes = float(st[0].item())
        code = self.env.check_errors()           # the stream is drained by the item() above: one 4-byte read
        if code != 0:                            # (this rank's envs; the word is sticky, every later call raises too)
            raise EnvError(code, f"VecTrainer iteration {self.iteration_count}")
        if self.pools is not None and self._tally_pending:
            self._fold_tally()
        self.iteration_count += 1
        self._in_iteration = False
        return st.cpu().numpy()

    # -- whole state and checkpoints (satrl/checkpoint.py) -------------------
    def state_dict(self):
        """Everything the next iteration reads, as a nested dict of CPU numpy
        arrays, plain scalars and lists of plain records.  Defined between
        iterations only (after finish_iteration): there the accumulators are
        zero and the rollout buffer apart from obs[0] is dead; anywhere else
        this raises.  The surrogate's weights and the reset box are
        configuration; `member`, `last_assignment` and `ellipse_params` are
        rewritten by the next rollout."""
        busy = self._in_iteration
        if self.obs_norm:
            busy = busy or self._obs_acc_rows != 0 or bool(self.obs_acc.ne(0).any().item())
        if self.reward_scaling:
            busy = busy or bool(self.ret_acc.ne(0).any().item())
        if busy:
            raise RuntimeError("a trainer's state is defined between iterations only: call state_dict() / "
                               "save_checkpoint() after finish_iteration(), not between collect() and it")
        d = {"flag": self.flag, "iteration_count": int(self.iteration_count), "rollout_steps": int(self.rollout_steps),
             "episodes": float(self.episodes), "pursuer": self.pursuer.state(), "evader": self.evader.state(),
             "env": self.env.full_state(), "obs0": self.buf.obs[0].cpu().numpy(),
             "gen": self.gen.get_state().cpu().numpy().copy(),
             "diagnostics": [dict(r) for r in self.diagnostics],
             "evaluations": [[int(it), float(ep), dict(s)] for it, ep, s in self.evaluations]}
        if self.sampler == "stratified":
            d["strata_gen"] = {str(s_): g.get_state().cpu().numpy().copy() for s_, g in self.strata_gen.items()}
        if self.obs_norm:
            d.update(obs_raw=self.obs_raw.cpu().numpy(), obs_rms=self.obs_rms.state_dict(),
                     obs_stats=self.obs_stats.cpu().numpy(), obs_pivot=self.obs_pivot.cpu().numpy())
        if self.reward_scaling:
            d.update(ret_rms=self.ret_rms.state_dict(), ret_carry=self.ret_carry.cpu().numpy())
        if self.pools is not None:
            d["pools"] = {}
            for k, p in self.pools.items():
                s = p.state()
                s["storage"] = s["storage"].numpy()
                d["pools"][k] = s
        if self._laws:                           # (optional: a run without laws writes what it always wrote)
            d["scripted"] = {k: law.state() for k, law in self._laws.items()}
        pair = act_noise_spec(self.act_noise)    # (optional likewise) the draw itself needs no state: it is a
        if pair is not None:                     # function of the env id, episode index and step count above
            d["act_noise"] = [list(pair[0]), list(pair[1]), int(self.act_noise_seed)]
        norm = obs_noise_spec(self.obs_noise)    # (optional too) a row is a function of the same restored values
        if norm is not None:
            d["obs_noise"] = [list(norm[0]), list(norm[1]), int(norm[2]), int(self.obs_noise_seed)]
        if self.pools is not None:
            d["league"] = {"law_prob": float(self.league_law_prob), "weighting": self.opponent_weighting,
                           "power": int(self.pfsp_power),
                           "laws": {k: [law.state() for law in t.laws] for k, t in self._league.items()},
                           "counts": {k: c.copy() for k, c in self.league_counts.items()}}
        return d

    def load_state_dict(self, d):
        """Restore state_dict() in place: captured rollout and update graphs and
        every tensor a minibatch plan points at stay valid.  Sets the Flag and
        the learner without restarting the envs; buf.obs[0] is restored as
        saved, not normalised again.  Without a "gen" entry (a checkpoint read
        under another sharding) the uniform sampler's generator is seeded as
        the constructor seeds it."""
        def scalar(k, typ):
            return typ(np.asarray(d[k]).item())

        def per_env(k, like):
            a = torch.from_numpy(np.ascontiguousarray(d[k]))
            if a.dtype != like.dtype or tuple(a.shape) != tuple(like.shape):
                raise ValueError(f"state {k!r}: {a.dtype} {tuple(a.shape)} for {like.dtype} {tuple(like.shape)} "
                                 f"(a state of another env count goes through load_checkpoint)")
            like.copy_(a)

        flag = scalar("flag", int)
        if flag not in (0, 1):
            raise ValueError("Flag 0 (pursuer) or 1 (evader)")
        for k, on in (("obs_rms", self.obs_norm), ("ret_rms", self.reward_scaling), ("pools", self.pools is not None)):
            if on != (k in d):
                raise ValueError(f"this state was saved {'with' if k in d else 'without'} {k}, the trainer runs "
                                 f"{'with' if on else 'without'} it")
        self.pursuer.load_state(d["pursuer"])
        self.evader.load_state(d["evader"])
        self.env.load_full_state(d["env"])
        per_env("obs0", self.buf.obs[0])
        if self.obs_norm:
            per_env("obs_raw", self.obs_raw)
            self.obs_rms.load_state_dict(d["obs_rms"])
            self._write_obs_stats()
            st = self.obs_rms.device_stats()
            if not (np.array_equal(st, d["obs_stats"]) and np.array_equal(st[0], d["obs_pivot"])):
                raise ValueError("the saved device statistics are not those of the saved observation moments")
            self.obs_acc.zero_()
            self._obs_acc_rows = 0
        if self.reward_scaling:
            self.ret_rms.load_state_dict(d["ret_rms"])
            per_env("ret_carry", self.ret_carry)
            self.ret_acc.zero_()
        if self.pools is not None:
            for k, p in self.pools.items():
                s = dict(d["pools"][k])
                s["K"], s["H"], s["cursor"], s["added"], s["seed"] = (int(np.asarray(s[x]).item()) for x in
                                                                      ("K", "H", "cursor", "added", "seed"))
                s["storage"] = torch.from_numpy(np.ascontiguousarray(s["storage"]))
                p.load_state(s)
        saved_laws = d.get("scripted") or {}
        for k in _scripted.AGENTS:               # a state without the entry: no laws
            if k not in saved_laws:
                self.set_scripted_opponent(k, None)
            elif k in self._laws:                # in place: the captured graphs stay
                st = saved_laws[k]
                self._laws[k].update(G=np.asarray(st["G"]), b=np.asarray(st["b"]),
                                     max_action=float(np.asarray(st["max_action"]).item()))
            else:
                self.set_scripted_opponent(k, _scripted.ScriptedLaw.from_state(saved_laws[k]))
        if self.pools is not None:
            self._load_league(d.get("league"))
        noise = d.get("act_noise")               # a state without the entry: no noise
        if noise is None:
            self.set_act_noise(None)
        else:
            self.set_act_noise({"pursuer": noise[0], "evader": noise[1]}, seed=int(noise[2]))
        noise = d.get("obs_noise")               # likewise; obs0 / obs_raw above are the saved rows, and the
        if noise is None:                        # next row the env writes is measured under the saved spec
            self.set_obs_noise(None)
        else:
            self.set_obs_noise({"pursuer": dict(zip(OBS_NOISE_KEYS, noise[0])),
                                "evader": dict(zip(OBS_NOISE_KEYS, noise[1])),
                                "hold": int(noise[2])}, seed=int(noise[3]))
        if "gen" in d:
            self.gen.set_state(torch.from_numpy(np.ascontiguousarray(d["gen"], dtype=np.uint8)))
        else:
            self.gen.manual_seed(self.seed * 1000003 + _dist.rank(self.pg))
        if self.sampler == "stratified":
            for s_, g in self.strata_gen.items():
                g.set_state(torch.from_numpy(np.ascontiguousarray(d["strata_gen"][str(s_)], dtype=np.uint8)))
        self.flag = flag
        self.learner = self.pursuer if flag == 0 else self.evader
        self.iteration_count = scalar("iteration_count", int)
        self.rollout_steps = scalar("rollout_steps", int)
        self.episodes = scalar("episodes", float)
        self.diagnostics = [dict(r) for r in d.get("diagnostics", [])]
        self.last_diagnostics = self.diagnostics[-1] if self.diagnostics else None
        self.evaluations = [(int(it), float(ep), dict(s)) for it, ep, s in d.get("evaluations", [])]
        self._in_iteration = False
        self._loaded = True

    def _load_league(self, lg):
        """The "league" entry of a state.  None (a state written before league
        play): the laws, the law probability, the weighting and the power stay
        what the trainer was built with, and the counts are zero.  Otherwise an
        agent whose law count is the saved one takes the saved values in place,
        so the captured graphs and the caller's law objects stay."""
        if lg is None:
            for c in self.league_counts.values():
                c[:] = 0
            self._tally_pending = False
            return
        weighting = lg.get("weighting", "uniform")
        if weighting not in _scripted.LEAGUE_WEIGHTINGS:
            raise ValueError(f"state 'league/weighting' is {weighting!r}, not one of {_scripted.LEAGUE_WEIGHTINGS}")
        self.opponent_weighting = weighting
        if "law_prob" in lg:
            self.league_law_prob = float(np.asarray(lg["law_prob"]).item())
        if "power" in lg:
            self.pfsp_power = int(np.asarray(lg["power"]).item())
        saved = lg.get("laws") or {}
        for k in _scripted.AGENTS:
            states, tab = list(saved.get(k) or []), self._league[k]
            if len(states) == len(tab):
                for law, st in zip(tab.laws, states):
                    law.update(G=np.asarray(st["G"], dtype=np.float64), b=np.asarray(st["b"], dtype=np.float64),
                               max_action=float(np.asarray(st["max_action"]).item()))
            else:
                self.set_league_laws(k, [_scripted.ScriptedLaw.from_state(st) for st in states])
        for k in _scripted.AGENTS:
            c = (lg.get("counts") or {}).get(k)
            if c is None:
                self.league_counts[k][:] = 0
                continue
            c = np.asarray(c)
            if c.shape != self.league_counts[k].shape or c.dtype.kind not in "iu":
                raise ValueError(f"state 'league/counts/{k}': {c.dtype} {c.shape} for int64 "
                                 f"{self.league_counts[k].shape}")
            self.league_counts[k][:] = c
        self._tally_pending = False

    def save_checkpoint(self, path):
        """The whole state into the directory `path` (satrl/checkpoint.py): one
        file per rank and meta.json, written beside `path` and renamed into
        place once complete.  Under a process group every rank calls this."""
        from . import checkpoint
        return checkpoint.save(self, path)

    def load_checkpoint(self, path, global_envs=None):
        """Continue from save_checkpoint(path), bit for bit where the sharding
        is the writer's; under another sharding every rank takes its env
        range out of the writer's files (the uniform sampler's minibatch order
        is then not the writer's; the stratified one's is).  global_envs:
        without a process group, the env count of the run this trainer holds a
        slice of (env_offset; default: this trainer's own N).  Returns the
        checkpoint's meta."""
        from . import checkpoint
        return checkpoint.load(self, path, global_envs)

    def _checkpoint_if_due(self, done, every, path, force=False):
        if path is not None and (force or (every and done % int(every) == 0)):
            self.save_checkpoint(path)

    @property
    def budget_reached(self):
        """True once the finished episodes (all envs, all ranks) reach
        max_train_steps: the reference's loop ends there (CPPO_main.py:110,
        `for epsiode in range(max_train_steps)`), and lr_decay is at 0."""
        return self.episodes >= self.args.max_train_steps

    def train(self, max_iterations=None, timers=None, evaluate_every=None, checkpoint_every=None,
              checkpoint_path=None, **eval_kwargs):
        """Iterations until the episode budget (or max_iterations) is reached;
        returns the per-iteration statistics.  evaluate_every=k: after every
        k-th iteration, evaluate(**eval_kwargs) and append (iteration_count,
        episodes, summary) to self.evaluations (args.evaluate_freq, which
        counts the reference's N = 1 steps, stays unread).  checkpoint_path
        with checkpoint_every=k: save_checkpoint(checkpoint_path) after every
        k-th iteration and after the last one; the previous checkpoint is
        replaced only once the new one is complete."""
        out, saved = [], 0
        while not self.budget_reached and (max_iterations is None or len(out) < max_iterations):
            out.append(self.iteration(timers))
            if evaluate_every and len(out) % int(evaluate_every) == 0:
                self.evaluations.append((self.iteration_count, self.episodes,
                                         self.evaluate(**eval_kwargs).summary()))
            if checkpoint_path is not None and checkpoint_every and len(out) % int(checkpoint_every) == 0:
                self.save_checkpoint(checkpoint_path)
                saved = len(out)
        if checkpoint_path is not None and saved != len(out):
            self.save_checkpoint(checkpoint_path)
        return out

    # -- evaluation (satrl/evaluate.py) -----------------------------------------------------
    def evaluate(self, num_envs=None, deterministic="learner", max_steps=None, states=None, seed=None, record=False,
                 opponent=None, act_noise="inherit", obs_noise="inherit"):
        """The current policies on a fresh env handle of the evaluator's own
        (`num_envs` envs, default N, this env's parameters): every env's first
        episode, at most max_steps steps (default max_episode_steps), as an
        EvalResult (per-env records and summary()).

        deterministic: which agents act with their mean ("learner", the
        default: the agent this Flag trains; "both"; "none"; or a set of
        "pursuer" / "evader"); the others sample as in the rollout, keyed by
        `seed` (default args.seed ^ evaluate.EVAL_SEED_XOR), agent id, global
        env id and a step counter that starts at 0, so equal calls give equal
        bits.  states=(f64_planes, i32_planes): start from these env states
        (VecSatellites.set_state) instead of reset(Flag).  With reset_spread the
        evaluator's env draws its starts from the same box under the
        evaluation seed, from episode index 0 on every call: a fixed test set
        of num_envs distinct scenarios (EvalResult.start).  record=True keeps
        the per-step streams (EvalResult.streams).  opponent=k: the frozen
        agent (the one this Flag does not train) acts with slot k of its
        opponent pool instead of its live parameters (IndexError for a slot
        that is not filled, ValueError without a pool).  opponent="scripted":
        the frozen agent acts with its scripted law (ValueError if it has
        none); opponent=<ScriptedLaw>: with that law, on the evaluator's raw
        observation (satrl/scripted.py).  act_noise: "inherit" (the
        default) runs the evaluator's env under this env's actuation noise as
        it is now, keyed by the evaluation seed; None executes every action
        exactly; a spec (args_param act_noise) evaluates under that spec, so
        a sweep over it is a robustness curve.  obs_noise: the same three
        forms for the observation noise (args_param obs_noise); the records
        (min_dis, final_dis) stay the truth, and with record=True
        streams["obs"] is the measurement and streams["obs64"] the truth.
        No state of the
        trainer changes.  Under data parallelism each rank evaluates its own
        envs; results are not reduced across ranks."""
        from .evaluate import VecEvaluator
        if isinstance(opponent, str):
            if opponent != "scripted":
                raise ValueError(f"opponent is a pool slot, 'scripted' or a ScriptedLaw, got {opponent!r}")
            opponent = self._laws.get(self.frozen_agent)
            if opponent is None:
                raise ValueError(f"evaluate(opponent='scripted'): the frozen agent ({self.frozen_agent}) has no "
                                 "scripted law")
        if isinstance(opponent, _scripted.ScriptedLaw):
            opponent.block(self.device)
        elif opponent is not None:
            if self.pools is None:
                raise ValueError("evaluate(opponent=k) needs an opponent pool (args.opponent_pool > 0)")
            self.pools[self.frozen_agent].slot(opponent)         # IndexError for a slot that is not filled
            opponent = int(opponent)
        n = self.N if num_envs is None else int(num_envs)
        if n not in self._evaluators:
            self._evaluators[n] = VecEvaluator(self, n)
        return self._evaluators[n].evaluate(deterministic=deterministic, max_steps=max_steps, states=states, seed=seed,
                                            record=record, opponent=opponent, act_noise=act_noise,
                                            obs_noise=obs_noise)

    def evaluate_pool(self, **kw):
        """evaluate(opponent=k, **kw) against every filled slot of the frozen
        agent's pool, [(meta, summary)] in slot order: the learner's row of
        the cross-play table.  With league laws, a row per law of the frozen
        agent follows (evaluate(opponent=law), meta {"agent", "law": j})."""
        if self.pools is None:
            raise ValueError("evaluate_pool needs an opponent pool (args.opponent_pool > 0)")
        pool = self.pools[self.frozen_agent]
        rows = [(dict(pool.metas[k]), self.evaluate(opponent=k, **kw).summary()) for k in range(pool.filled)]
        # league play: then one row per law of the frozen agent, in law order
        rows += [({"agent": self.frozen_agent, "law": j}, self.evaluate(opponent=law, **kw).summary())
                 for j, law in enumerate(self._league[self.frozen_agent].laws)]
        return rows

    def iteration(self, timers=None):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        self.collect()
        ev[1].record()
        self.compute_advantages()
        ev[2].record()
        self.update()
        ev[3].record()
        if self.learner.comm is not None:
            # RCCL watchdog over the update's graph replays: a dead or stalled
            # peer aborts the communicator and raises instead of hanging here
            self.learner.comm.wait(_dist.dp_timeout_s())
        stats = self.finish_iteration()
        if self.pools is not None and self.opponent_snapshot_every and \
                self.iteration_count % self.opponent_snapshot_every == 0:
            self.snapshot_opponent()
        if timers is not None:
            torch.cuda.synchronize()
            timers.setdefault("rollout_ms", []).append(ev[0].elapsed_time(ev[1]))
            timers.setdefault("gae_ms", []).append(ev[1].elapsed_time(ev[2]))
            timers.setdefault("update_ms", []).append(ev[2].elapsed_time(ev[3]))
        return stats
