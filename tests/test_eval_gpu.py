"""Policy evaluation on the GPU: satrl_policy_eval (policy_kernel MODE 2),
the episode-record kernels, and VecTrainer.evaluate end to end."""

import numpy as np
import pytest
import torch

import eval_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAPTURE = {0: 100.0, 1: -150.0}          # the capture literals of Flag 0 / Flag 1 (win_reward 100)
TIMEOUT = {0: 0.0, 1: 100.0}


def _args(**kw):
    from satrl.trainer import args_param
    a = args_param(chkpt_dir="/tmp", **kw)
    a.state_dim, a.action_dim, a.max_action = 18, 3, 1.6
    return a


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _records(res):
    return {k: getattr(res, k).cpu().numpy() for k in R.REC_F64 + R.REC_I32}


def _same_result(a, b):
    for k in R.REC_F64 + R.REC_I32:
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(torch.nan_to_num(x.double(), nan=-1.0), torch.nan_to_num(y.double(), nan=-1.0)), k
        assert torch.equal(torch.isnan(x.double()), torch.isnan(y.double())), k
    assert a.steps == b.steps
    if a.streams is not None and b.streams is not None:
        for k in a.streams:
            assert torch.equal(a.streams[k], b.streams[k]), k


# ---------------------------------------------------------------------------
# 1. policy_eval
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 128, 256])
def test_policy_eval_against_policy_act(H):
    """A sampled agent's action is policy_act's for the same key, bit for bit;
    a deterministic agent's is policy_act's on parameters whose log_std is
    -200 (exp underflows to exactly 0 in f32, mean + 0 * z = mean; -0 == +0
    under torch.equal) and matches the torch actor's forward at
    test_policy_act_and_value_kernels' own bar.  N: the 32-row workgroup and
    its ragged tail."""
    from satrl._lib import NativeError
    from satrl.ppo import PPOLearner, policy_act, policy_eval, ppo_layout
    torch.manual_seed(5)
    args = _args(hidden_width=H)
    Lp = PPOLearner(args, "pursuer", use_graph=False)
    Le = PPOLearner(args, "evader", use_graph=False)
    with torch.no_grad():
        for L in (Lp, Le):
            for p in list(L.actor.parameters()) + list(L.critic.parameters()):
                p.add_(torch.randn_like(p) * 0.05)
    ls = ppo_layout(H)["ls"]
    Pdet = []
    for L in (Lp, Le):
        q = L.P.clone()
        q[ls:ls + 3] = -200.0
        Pdet.append(q)
    g = torch.Generator(device=DEV).manual_seed(2)
    sb = torch.tensor([7], dtype=torch.int64, device=DEV)
    for N in (1, 31, 32, 33, 65):
        obs = torch.randn((N, 18), device=DEV, generator=g)
        with torch.no_grad():
            means = [Lp.actor(obs), Le.actor(obs)]
        new = lambda: torch.full((N, 3), float("nan"), device=DEV)      # noqa: E731
        for two in (True, False):
            P1, P1det = (Le.P, Pdet[1]) if two else (None, None)
            samp = [new() for _ in range(4)]
            mean = [new() for _ in range(4)]
            policy_act(H, obs, Lp.P, P1, 1.6, 123, 4096, 5, *(samp if two else samp[:2]), step_base=sb)
            policy_act(H, obs, Pdet[0], P1det, 1.6, 123, 4096, 5, *(mean if two else mean[:2]), step_base=sb)
            for det in range(4):
                a0, a1 = new(), new()
                if not two and det & 2:
                    with pytest.raises(NativeError):
                        policy_eval(H, obs, Lp.P, None, 1.6, det, 123, 4096, 5, a0, None, step_base=sb)
                    continue
                policy_eval(H, obs, Lp.P, P1, 1.6, det, 123, 4096, 5, a0, a1 if two else None, step_base=sb)
                for k, a in enumerate((a0, a1) if two else (a0,)):
                    what = (H, N, two, det, k)
                    if det >> k & 1:
                        assert torch.equal(a, mean[2 * k]), what
                        assert torch.allclose(a, means[k], rtol=1e-5, atol=1e-5), what
                    else:
                        assert torch.equal(a, samp[2 * k]), what
                if not two:
                    assert bool(torch.isnan(a1).all())               # one agent: act1 is not written


# ---------------------------------------------------------------------------
# 2. episode records on synthetic streams
# ---------------------------------------------------------------------------
def _synthetic(N, T=12, cap=100.0, timeout=0.0, seed=0):
    """Streams [T, N, ...] with the special envs at fixed indices mod 7:
    0 never done; 1 done at step 1 (the second call) with the capture literal;
    2 done twice (capture at step 3, timeout literal at step 8); 3 gets the
    capture literal on a step that is not done, then is done with the timeout
    literal; 4 done with the timeout literal at step 5; 5, 6: random dones.
    Rewards mix 1e17 with O(1) terms."""
    rng = np.random.default_rng(seed + N)
    reward = rng.normal(0, 3, (T, N))
    reward[::3] += rng.choice([1e17, -1e17, 1.0], (len(reward[::3]), N))
    done = np.zeros((T, N), np.uint8)
    idx = np.arange(N)
    k = idx % 7
    done[1, k == 1] = 1; reward[1, k == 1] = cap
    done[3, k == 2] = 1; reward[3, k == 2] = cap
    done[8, k == 2] = 1; reward[8, k == 2] = timeout
    reward[2, k == 3] = cap
    done[6, k == 3] = 1; reward[6, k == 3] = timeout
    done[5, k == 4] = 1; reward[5, k == 4] = timeout
    rnd = (rng.uniform(size=(T, N)) < 0.15) & (k >= 5)
    done[rnd] = 1
    reward[rnd] = rng.choice([cap, timeout], int(rnd.sum()))
    obs64 = rng.normal(0, 1, (T, N, 18)) * np.array([2e5, 3e4, 7e3] * 6)
    pa = rng.uniform(-1.6, 1.6, (T, N, 3)).astype(np.float32)
    ea = rng.uniform(-1.6, 1.6, (T, N, 3)).astype(np.float32)
    return reward, done, obs64, pa, ea


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_episode_record_synthetic_streams(N):
    from satrl.ppo import episode_record, episode_record_reset
    cap = 100.0
    reward, done, obs64, pa, ea = _synthetic(N, cap=cap)
    T = reward.shape[0]
    ref, alive_ref = R.record_streams(reward, done, obs64, pa, ea, cap)
    rf = torch.full((5, N), 7.0, dtype=torch.float64, device=DEV)
    ri = torch.full((2, N), 7, dtype=torch.int32, device=DEV)
    alive = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    episode_record_reset(rf, ri, alive)
    got0 = {k: rf[j].cpu().numpy() for j, k in enumerate(R.REC_F64)}
    assert int(alive.item()) == N and not ri.any()
    assert np.isnan(got0["final_dis"]).all() and np.isposinf(got0["min_dis"]).all()
    assert not got0["ret"].any() and not got0["dv_p"].any() and not got0["dv_e"].any()
    d_rew, d_done, d_obs, d_pa, d_ea = _t(reward), _t(done), _t(obs64), _t(pa), _t(ea)
    alive_got = []
    for t in range(T):
        episode_record(d_rew[t], d_done[t], d_obs[t], d_pa[t], d_ea[t], cap, rf, ri, alive)
        alive_got.append(int(alive.item()))
    assert alive_got == alive_ref
    got = {k: rf[j].cpu().numpy() for j, k in enumerate(R.REC_F64)}
    got.update({k: ri[j].cpu().numpy() for j, k in enumerate(R.REC_I32)})
    R.assert_records_equal(got, ref)
    # what the streams are there to show
    k = np.arange(N) % 7
    assert (got["outcome"][k == 0] == 0).all() and np.isnan(got["final_dis"][k == 0]).all()
    assert (got["length"][k == 0] == T).all()
    if N > 4:
        assert (got["outcome"][k == 1] == 1).all() and (got["length"][k == 1] == 2).all()
        assert (got["outcome"][k == 2] == 1).all() and (got["length"][k == 2] == 4).all()      # the first episode
        assert (got["outcome"][k == 3] == 2).all() and (got["length"][k == 3] == 7).all()      # not at step 2
        assert (got["outcome"][k == 4] == 2).all() and (got["length"][k == 4] == 6).all()


# ---------------------------------------------------------------------------
# 3. outcomes known beforehand, through the real env
# ---------------------------------------------------------------------------
def _scenario_states(N, flag):
    """Even envs: the pursuer 7000 m from the evader at rest (inside
    d_capture = 15000 whatever the first actions); odd envs: the reset
    geometry, 182 000 m apart."""
    from satrl.env import PYINT, pack_bits
    f = np.zeros((15, N))
    f[6] = 18000.0                                   # Ep = [18000, 0, 0]
    f[0] = np.where(np.arange(N) % 2 == 0, 18000.0 + 7000.0, 200000.0)
    f[12] = f[13] = 320.0
    f[14] = np.inf
    i = np.zeros((3, N), np.int32)
    i[2] = pack_bits(PYINT, PYINT, 1, flag)          # the bits of a freshly reset env of the trainer's
    return _t(f), _t(i)


@pytest.mark.parametrize("flag", [0, 1])
def test_evaluate_outcomes_known_beforehand(flag):
    from satrl.trainer import VecTrainer
    N = 65
    args = _args(batch_size=64 * 8, mini_batch_size=128, hidden_width=64, K_epochs=1, num_envs=64, horizon=8,
                 max_episode_steps=8, seed=3, rollout_graph_chunk=3, update_graph_group=2)
    tr = VecTrainer(args, flag=flag, d_capture=15000.0)
    res = tr.evaluate(num_envs=N, states=_scenario_states(N, flag))
    rec = _records(res)
    even = np.arange(N) % 2 == 0
    assert (rec["outcome"][even] == 1).all() and (rec["length"][even] == 1).all()
    assert (rec["ret"][even] == CAPTURE[flag]).all()
    assert (rec["final_dis"][even] <= 15000.0).all() and np.array_equal(rec["final_dis"][even], rec["min_dis"][even])
    assert (rec["outcome"][~even] == 2).all() and (rec["length"][~even] == 8).all()
    assert (rec["final_dis"][~even] > 15000.0).all()
    s = res.summary()
    assert s["episodes"] == N and s["unfinished"] == 0 and s["capture_rate"] == 33 / 65
    assert s["mean_length"] == (33 * 1 + 32 * 8) / 65 and res.steps == 8
    assert s["mean_return"] == rec["ret"].mean() and s["std_return"] == rec["ret"].std()
    # stopped early: the odd envs are unfinished and out of the rates
    res3 = tr.evaluate(num_envs=N, states=_scenario_states(N, flag), max_steps=3)
    rec3 = _records(res3)
    assert (rec3["outcome"][~even] == 0).all() and (rec3["length"][~even] == 3).all()
    assert np.isnan(rec3["final_dis"][~even]).all()
    for k in R.REC_F64 + R.REC_I32:
        assert np.array_equal(rec3[k][even], rec[k][even]), k
    s3 = res3.summary()
    assert s3["episodes"] == 33 and s3["unfinished"] == 32 and s3["capture_rate"] == 1.0
    assert s3["mean_length"] == 1.0 and s3["mean_return"] == CAPTURE[flag] and res3.steps == 3
    assert tr.env.check_errors() == 0


# ---------------------------------------------------------------------------
# 4. plumbing, record=True
# ---------------------------------------------------------------------------
def _plumbing_trainer(H, graphs, d_capture=15000.0, flag=0):
    from satrl.trainer import VecTrainer
    args = _args(batch_size=65 * 8, mini_batch_size=130, hidden_width=H, K_epochs=1, num_envs=65, horizon=8,
                 max_episode_steps=8, seed=11, rollout_graph_chunk=3, update_graph_group=2)
    return VecTrainer(args, flag=flag, d_capture=d_capture, use_graphs=graphs)


@pytest.mark.parametrize("H", [64, 256])
def test_evaluate_plumbing_recorded_streams(H):
    from satrl.env import VecSatellites
    from satrl.evaluate import EVAL_SEED_XOR
    from satrl.ppo import policy_eval
    N, T, flag = 65, 8, 0
    tr = _plumbing_trainer(H, True)
    res = tr.evaluate(record=True)                       # chunks of 3, 3 and 2 steps
    st = res.streams
    assert res.steps == T and all(st[k].shape[:2] == (T, N) for k in st)
    assert res.det_mask == 1 and res.seed == 11 ^ EVAL_SEED_XOR != 11
    # (a) the env kernel replays the recorded streams from the recorded actions
    env = VecSatellites(N, device=DEV, d_capture=15000.0, max_episode_steps=8, Flag=flag)
    obs0 = env.reset(flag)
    assert torch.equal(st["policy_input"][0], obs0)
    o32 = torch.empty((N, 18), dtype=torch.float32, device=DEV)
    o64 = torch.empty((N, 18), dtype=torch.float64, device=DEV)
    for t in range(T):
        _, r, d = env.step(st["pursuer_action"][t], st["evader_action"][t], None, obs_out=o32, obs64_out=o64)
        assert torch.equal(r, st["reward"][t]) and torch.equal(d, st["done"][t]), t
        assert torch.equal(o64, st["obs64"][t]) and torch.equal(o32, st["obs"][t]), t
        if t + 1 < T:
            assert torch.equal(st["policy_input"][t + 1], o32), t
    assert env.check_errors() == 0
    # (b) every step's actions are policy_eval of that step's input
    for t in range(T):
        a0, a1 = torch.empty((N, 3), device=DEV), torch.empty((N, 3), device=DEV)
        policy_eval(H, st["policy_input"][t], tr.pursuer.P, tr.evader.P, 1.6, res.det_mask, res.seed, 0, t, a0, a1)
        assert torch.equal(a0, st["pursuer_action"][t]) and torch.equal(a1, st["evader_action"][t]), t
    # (c) the records are the numpy recorder's over the streams
    ref, _ = R.record_streams(st["reward"].cpu().numpy(), st["done"].cpu().numpy(), st["obs64"].cpu().numpy(),
                              st["pursuer_action"].cpu().numpy(), st["evader_action"].cpu().numpy(), CAPTURE[flag])
    R.assert_records_equal(_records(res), ref)
    # (d) graphs and eager
    eager = _plumbing_trainer(H, False).evaluate(record=True)
    _same_result(res, eager)
    # (e) the same seed twice, another seed
    again = tr.evaluate(record=True)
    _same_result(res, again)
    _same_result(res, tr.evaluate())                     # without the streams: the same records
    other = tr.evaluate(record=True, seed=res.seed + 1)
    assert torch.equal(other.streams["pursuer_action"][0], st["pursuer_action"][0])      # the mean of the same obs
    assert not torch.equal(other.streams["evader_action"], st["evader_action"])


def test_evaluate_both_outcomes_occur():
    """(f) d_capture at the reset separation (182 000 m): the separation after
    a step is within a few hundred metres of it, on either side depending on
    the sampled actions, so some envs capture in the first steps and others
    time out."""
    tr = _plumbing_trainer(64, True, d_capture=182000.0)
    res = tr.evaluate(record=True)
    rec = _records(res)
    assert (rec["outcome"] == 1).any() and (rec["outcome"] == 2).any() and not (rec["outcome"] == 0).any()
    cap = rec["outcome"] == 1
    assert (rec["length"][cap] < 8).any() and (rec["length"][~cap] == 8).all()
    st = res.streams
    ref, _ = R.record_streams(st["reward"].cpu().numpy(), st["done"].cpu().numpy(), st["obs64"].cpu().numpy(),
                              st["pursuer_action"].cpu().numpy(), st["evader_action"].cpu().numpy(), CAPTURE[0])
    R.assert_records_equal(rec, ref)
    s = res.summary()
    assert s["capture_rate"] == cap.sum() / 65 and 0 < s["capture_rate"] < 1


# ---------------------------------------------------------------------------
# 5. training is unperturbed
# ---------------------------------------------------------------------------
def _trainer_state(tr):
    L = tr.learner
    f, i = tr.env.get_state()
    out = {"P": L.P, "M": L.M, "V": L.V, "steps": L.steps, "obs": tr.buf.obs, "act": tr.buf.act, "env_f64": f,
           "env_i32": i, "stats": tr.env.stats, "step_base": tr.step_base, "gen": tr.gen.get_state(),
           "otherP": (tr.evader if tr.flag == 0 else tr.pursuer).P}
    if tr.obs_norm:
        out["obs_acc"] = tr.obs_acc
        out.update({"obs_rms." + k: torch.from_numpy(v) for k, v in tr.obs_rms.state_dict().items()})
    if tr.reward_scaling:
        out["ret_carry"] = tr.ret_carry
        out.update({"ret_rms." + k: torch.from_numpy(v) for k, v in tr.ret_rms.state_dict().items()})
    torch.cuda.synchronize()
    return {k: v.detach().clone().cpu() for k, v in out.items()}, (tr.rollout_steps, tr.iteration_count, tr.episodes)


@pytest.mark.parametrize("norm", [False, True])
def test_evaluate_leaves_training_unperturbed(norm):
    from satrl.env import VecSatellites
    from satrl.trainer import VecTrainer
    kw = dict(obs_norm=True, reward_scaling=True, obs_norm_calib_steps=8) if norm else {}

    def make():
        args = _args(batch_size=64 * 8, mini_batch_size=128, hidden_width=64, K_epochs=1, num_envs=64, horizon=8,
                     max_episode_steps=6, seed=9, rollout_graph_chunk=4, update_graph_group=2, **kw)
        return VecTrainer(args, flag=0, d_capture=15000.0)

    A, B = make(), make()
    A.iteration()
    before = _trainer_state(A)
    res = A.evaluate(record=True)
    after = _trainer_state(A)
    assert before[1] == after[1]
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]), k
    if norm:                                             # the policy saw the raw rows under the current statistics
        st = res.streams
        env = VecSatellites(64, device=DEV, d_capture=15000.0, max_episode_steps=6, Flag=0)
        raw = torch.cat([env.reset(0)[None], st["obs"][:-1]])
        for t in range(res.steps):
            assert torch.equal(st["policy_input"][t], A.normalize_obs(raw[t].contiguous())), t
        assert not torch.equal(st["policy_input"], raw)
    A.iteration()
    B.iteration()
    B.iteration()
    sa, sb = _trainer_state(A), _trainer_state(B)
    assert sa[1] == sb[1]
    for k in sa[0]:
        assert torch.equal(sa[0][k], sb[0][k]), k
    assert res.steps == 6 and res.summary()["episodes"] == 64


# ---------------------------------------------------------------------------
# 6. periodic evaluation
# ---------------------------------------------------------------------------
def test_train_evaluate_every():
    from satrl.trainer import VecTrainer

    def make():
        args = _args(batch_size=64 * 8, mini_batch_size=128, hidden_width=64, K_epochs=1, num_envs=64, horizon=8,
                     max_episode_steps=6, seed=2, rollout_graph_chunk=4, update_graph_group=2)
        return VecTrainer(args, flag=0, d_capture=15000.0)

    A, B = make(), make()
    out_a = A.train(max_iterations=2, evaluate_every=1, max_steps=4)     # (keywords go to evaluate)
    out_b = B.train(max_iterations=2)
    assert B.evaluations == [] and len(A.evaluations) == 2 and len(out_a) == len(out_b) == 2
    for x, y in zip(out_a, out_b):
        assert np.array_equal(x, y)
    for n, (it, episodes, summary) in enumerate(A.evaluations):
        assert it == n + 1 and episodes == float(out_a[n][0])
        assert summary["episodes"] == 0 and summary["unfinished"] == 64       # 4 of the episode's 6 steps
        assert np.isnan(summary["capture_rate"])
    assert A.evaluate().summary()["episodes"] == 64
    assert torch.equal(A.learner.P, B.learner.P)
