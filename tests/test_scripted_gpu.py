"""Scripted opponents on the GPU: satrl_scripted_act and the fused
satrl_policy_act_scripted / satrl_policy_eval_scripted against the NumPy
restatement of the law and against plain two-agent satrl_policy_act /
satrl_policy_eval launches, under graph replay, and through VecTrainer
(collect, sharding, switching a law off, evaluate, checkpoints).  Every
comparison is bitwise: there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from test_scripted_cpu import raw_rows, restated

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
GUARD = 64                                               # canary rows behind every output


def _args(**kw):
    from satrl.trainer import args_param
    kw.setdefault("hidden_width", 64)
    kw.setdefault("num_envs", 64)
    kw.setdefault("horizon", 8)
    kw.setdefault("batch_size", kw["num_envs"] * kw["horizon"])
    kw.setdefault("mini_batch_size", 128)
    kw.setdefault("K_epochs", 1)
    kw.setdefault("rollout_graph_chunk", 4)
    kw.setdefault("max_episode_steps", 10)
    kw.setdefault("seed", 3)
    a = args_param(chkpt_dir="/tmp", **kw)
    a.state_dim, a.action_dim, a.max_action = 18, 3, 1.6
    return a


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _law(seed=0, scale=1e-6):
    """A random law whose actions on raw-scale rows are partly clamped."""
    from satrl.scripted import ScriptedLaw
    rng = np.random.default_rng(seed)
    return ScriptedLaw(rng.standard_normal((3, 18)) * scale, rng.standard_normal(3) * 0.2, 1.6)


def _raw(N, seed):
    return torch.from_numpy(raw_rows(np.random.default_rng(seed), N)).to(DEV)


_LIVE = {}


def _live(H):
    """Both agents' flat parameter sets at width H, once."""
    if H not in _LIVE:
        from satrl.ppo import PPOLearner
        torch.manual_seed(5)
        args = _args(hidden_width=H)
        _LIVE[H] = [PPOLearner(args, "pursuer", use_graph=False).P.clone(),
                    PPOLearner(args, "evader", use_graph=False).P.clone()]
    return _LIVE[H]


def _guarded(N, cols=3):
    big = torch.full((N + GUARD, cols), NAN, device=DEV)
    return big, big[:N]


# ---------------------------------------------------------------------------
# 1. the stand-alone kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 31, 32, 33, 70, 257])
def test_standalone_kernel_equals_numpy_and_the_host_build(N):
    from satrl.scripted import coast, scripted_act, scripted_act_host
    law = _law(N)
    for rows in (raw_rows(np.random.default_rng(N), N),
                 np.random.default_rng(N + 1).standard_normal((N, 18)).astype(np.float32) * 3e5):
        rows[0, 4] = np.nan if N > 1 else rows[0, 4]
        big, act = _guarded(N)
        scripted_act(torch.from_numpy(rows).to(DEV), law, act)
        got = act.cpu().numpy()
        assert np.array_equal(_np_bits(got), _np_bits(restated(rows, law.G, law.b, law.max_action)))
        assert np.array_equal(_np_bits(got), _np_bits(scripted_act_host(rows, law)))
        assert bool(torch.isnan(big[N:]).all())
        if N > 1:
            assert np.isnan(got[0]).all() and not np.isnan(got[1:]).any()
            assert 0 < int((np.abs(got[1:]) == np.float32(1.6)).sum())
    finite = torch.from_numpy(raw_rows(np.random.default_rng(9), N)).to(DEV)
    assert not bool(scripted_act(finite, coast()).view(torch.int32).any())      # +0.0 everywhere


# ---------------------------------------------------------------------------
# 2. / 3. the fused kernels against the two-agent launches
# ---------------------------------------------------------------------------
SEED, ENV_OFFSET, STEP, STEP_BASE = 123, 96, 5, 11


def _inputs(N):
    g = torch.Generator(device=DEV).manual_seed(1000 + N)
    obs = torch.randn((N, 18), device=DEV, generator=g)
    obs_law = _raw(N, 2000 + N)                          # another tensor than obs
    sb = torch.tensor([STEP_BASE], dtype=torch.int64, device=DEV)
    return obs, obs_law, sb


@pytest.mark.parametrize("agent", [0, 1])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_fused_act_kernel_equals_policy_act_and_the_law(H, agent):
    from satrl.ppo import policy_act, policy_act_scripted
    from satrl.scripted import scripted_act
    live = _live(H)
    law = _law(7)
    for N in (1, 33, 70):
        obs, obs_law, sb = _inputs(N)
        ref = [torch.full((N, 3), NAN, device=DEV) for _ in range(4)]
        policy_act(H, obs, live[0], live[1], 1.6, SEED, ENV_OFFSET, STEP, *ref, step_base=sb)
        want_law = scripted_act(obs_law, law)
        keep = [t.clone() for t in (obs, obs_law, live[agent], law.block())]
        (ba, act), (bl, logp), (bs, act_s) = _guarded(N), _guarded(N), _guarded(N)
        policy_act_scripted(H, obs, obs_law, live[agent], agent, 1.6, SEED, ENV_OFFSET, STEP, act, logp, law, act_s,
                            step_base=sb)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(act).any() | torch.isnan(logp).any())
        assert _same(act, ref[2 * agent]), (H, agent, N, "act")
        assert _same(logp, ref[2 * agent + 1]), (H, agent, N, "logp")
        assert not _same(act, ref[2 - 2 * agent]), (H, agent, N)         # the other agent's key stream differs
        assert _same(act_s, want_law), (H, agent, N, "act_scripted")
        assert np.array_equal(_np_bits(act_s.cpu().numpy()),
                              _np_bits(restated(obs_law.cpu().numpy(), law.G, law.b, 1.6)))
        for name, b in (("act", ba), ("logp", bl), ("act_scripted", bs)):
            assert bool(torch.isnan(b[N:]).all()), (H, agent, N, "guard", name)
        for name, x, y in zip(("obs", "obs_law", "P", "law"), (obs, obs_law, live[agent], law.block()), keep):
            assert torch.equal(x, y), name
        # obs_law may be obs itself
        act2, logp2, act_s2 = (torch.full((N, 3), NAN, device=DEV) for _ in range(3))
        policy_act_scripted(H, obs, obs, live[agent], agent, 1.6, SEED, ENV_OFFSET, STEP, act2, logp2, law, act_s2,
                            step_base=sb)
        assert _same(act2, act) and _same(logp2, logp) and _same(act_s2, scripted_act(obs, law))


@pytest.mark.parametrize("agent", [0, 1])
@pytest.mark.parametrize("H", [64, 256])
def test_fused_eval_kernel_equals_policy_eval_and_the_law(H, agent):
    from satrl.ppo import policy_eval, policy_eval_scripted
    from satrl.scripted import scripted_act
    live = _live(H)
    law = _law(8)
    for N in (1, 33, 70):
        obs, obs_law, sb = _inputs(N)
        want_law = scripted_act(obs_law, law)
        for det in (1, 0):
            ref = [torch.full((N, 3), NAN, device=DEV) for _ in range(2)]
            policy_eval(H, obs, live[0], live[1], 1.6, det << agent, SEED, ENV_OFFSET, STEP, *ref, step_base=sb)
            (ba, act), (bs, act_s) = _guarded(N), _guarded(N)
            policy_eval_scripted(H, obs, obs_law, live[agent], agent, 1.6, det, SEED, ENV_OFFSET, STEP, act, law,
                                 act_s, step_base=sb)
            torch.cuda.synchronize()
            assert not bool(torch.isnan(act).any())
            assert _same(act, ref[agent]), (H, agent, N, det, "act")
            assert _same(act_s, want_law), (H, agent, N, det, "act_scripted")
            assert bool(torch.isnan(ba[N:]).all()) and bool(torch.isnan(bs[N:]).all())
        # the mean and the sample differ (the two comparisons above are two)
        a1, a0, s_ = (torch.empty((N, 3), device=DEV) for _ in range(3))
        policy_eval_scripted(H, obs, obs_law, live[agent], agent, 1.6, 1, SEED, ENV_OFFSET, STEP, a1, law, s_,
                             step_base=sb)
        policy_eval_scripted(H, obs, obs_law, live[agent], agent, 1.6, 0, SEED, ENV_OFFSET, STEP, a0, law, s_,
                             step_base=sb)
        assert not _same(a1, a0)


# ---------------------------------------------------------------------------
# 4. a captured launch follows the law block
# ---------------------------------------------------------------------------
def test_captured_graph_follows_law_updates():
    from satrl.ppo import policy_act_scripted
    from satrl.scripted import intercept_matrix, scripted_act
    H, N = 64, 70
    live = _live(H)
    law = _law(9)
    obs, obs_law, sb = _inputs(N)
    act, logp, act_s = (torch.full((N, 3), NAN, device=DEV) for _ in range(3))

    def launch():
        policy_act_scripted(H, obs, obs_law, live[0], 0, 1.6, SEED, ENV_OFFSET, STEP, act, logp, law, act_s,
                            step_base=sb)

    launch()                                             # eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for t in (act, logp, act_s):
        t.fill_(NAN)
    g.replay()
    first = [t.clone() for t in (act, logp, act_s)]
    assert _same(first[2], scripted_act(obs_law, law)) and not bool(torch.isnan(first[0]).any())
    ptr = law.block().data_ptr()
    law.update(G=intercept_matrix(10) * 1e-2, b=[0.1, -0.2, 0.3])
    assert law.block().data_ptr() == ptr                 # in place
    for t in (act, logp, act_s):
        t.fill_(NAN)
    g.replay()                                           # the same graph object: no recapture
    want = restated(obs_law.cpu().numpy(), law.G, law.b, 1.6)
    assert np.array_equal(_np_bits(act_s.cpu().numpy()), _np_bits(want))
    assert not _same(act_s, first[2])
    assert _same(act, first[0]) and _same(logp, first[1])


# ---------------------------------------------------------------------------
# 5. - 7. the trainer
# ---------------------------------------------------------------------------
BUF = ("obs", "act", "logp", "rew", "done")


def _trainer(flag=0, use_graphs=True, env_offset=0, law="default", **kw):
    from satrl.scripted import intercept
    from satrl.trainer import VecTrainer
    if law == "default":
        law = {("evader" if flag == 0 else "pursuer"): intercept(10)}
    # (d_capture 100 m: the episodes run on past their first step, so the law sees moving states)
    return VecTrainer(_args(scripted_opponent=law, **kw), flag=flag, d_capture=100.0, use_graphs=use_graphs,
                      env_offset=env_offset)


def _buf_same(a, b, cols=slice(None), cols_b=slice(None), what=""):
    for k in BUF:
        assert _same(getattr(a.buf, k)[:, cols], getattr(b.buf, k)[:, cols_b]), (what, k)


@pytest.mark.parametrize("case", ["flag0", "obs_norm", "flag1"])
def test_trainer_collect_with_graphs_on_and_off(case):
    kw = dict(obs_norm=True, obs_norm_calib_steps=4) if case == "obs_norm" else {}
    flag = 1 if case == "flag1" else 0
    A = _trainer(flag, True, **kw)
    B = _trainer(flag, False, **kw)
    law = B.scripted_opponents[B.frozen_agent]
    assert set(B.scripted_opponents) == {B.frozen_agent}
    A.collect()
    # B.collect() with use_graphs=False, step by step, to see the raw observation of the last step
    B._in_iteration = True
    B.step_base.fill_(B.rollout_steps)
    for t in range(B.T):
        if t == B.T - 1:
            raw = (B.obs_raw if B.obs_norm else B.buf.obs[t]).clone()
        B._policy_step(t)
    torch.cuda.synchronize()
    _buf_same(A, B, what=case)
    assert _same(A.other_a, B.other_a)
    want = restated(raw.cpu().numpy(), law.G, law.b, law.max_action)
    assert np.array_equal(_np_bits(B.other_a.cpu().numpy()), _np_bits(want))
    assert np.abs(want).max() > 0                        # the law does command something
    if case == "obs_norm":                               # ... from the raw row, not the one the learner sees
        seen = restated(B.buf.obs[B.T - 1].cpu().numpy(), law.G, law.b, law.max_action)
        assert not np.array_equal(_np_bits(seen), _np_bits(want))
    assert A.env.check_errors() == 0 and B.env.check_errors() == 0


def test_rollout_does_not_depend_on_the_sharding():
    whole = _trainer(0, True)
    parts = [_trainer(0, True, env_offset=o, num_envs=32) for o in (0, 32)]
    for tr in [whole] + parts:
        tr.collect()
    torch.cuda.synchronize()
    for k, p in enumerate(parts):
        _buf_same(whole, p, slice(32 * k, 32 * k + 32), what=f"shard {k}")
        assert _same(whole.other_a[32 * k:32 * k + 32], p.other_a)


def test_switching_a_law_off_and_updating_it():
    from satrl.scripted import evade_matrix
    A = _trainer(0, True, law={"evader": "evade"})
    A.iteration()
    graphs = dict(A._graphs)
    assert graphs
    A.scripted_opponents["evader"].update(G=evade_matrix(10, 0.25))     # only the gain: the same graph objects
    assert A._graphs == graphs and all(A._graphs[k] is g for k, g in graphs.items())
    A.set_scripted_opponent("evader", None)
    assert not A._graphs and A.scripted_opponents == {}
    sd = A.state_dict()
    assert "scripted" not in sd
    B = _trainer(0, True, law=None)                      # never had a law
    B.load_state_dict(sd)
    A.iteration()
    B.iteration()
    torch.cuda.synchronize()
    _buf_same(A, B, what="after the switch")
    assert _same(A.pursuer.P, B.pursuer.P) and _same(A.other_a, B.other_a) and _same(A.other_lp, B.other_lp)
    with pytest.raises(ValueError):
        _trainer(0, True, law={"evader": "coast"}, opponent_pool=2)
    C = _trainer(0, True, law=None, opponent_pool=2, num_envs=32)
    with pytest.raises(ValueError):
        C.set_scripted_opponent("evader", "coast")
    with pytest.raises(ValueError):
        A.set_scripted_opponent("umpire", "coast")


# ---------------------------------------------------------------------------
# 8. evaluate
# ---------------------------------------------------------------------------
def test_evaluate_against_a_law():
    from satrl.scripted import coast, intercept
    tr = _trainer(0, True, law=None)
    with pytest.raises(ValueError):
        tr.evaluate(num_envs=32, max_steps=16, opponent="scripted")
    law = coast()
    r1 = tr.evaluate(num_envs=32, max_steps=16, opponent=law)
    r2 = tr.evaluate(num_envs=32, max_steps=16, opponent=law)
    assert r1.steps > 0 and bool((r1.dv_e == 0).all()) and bool((r1.dv_p > 0).all())
    for k in ("ret", "final_dis", "min_dis", "dv_p", "dv_e", "length", "outcome"):
        assert torch.equal(getattr(r1, k), getattr(r2, k)), k
    plain = tr.evaluate(num_envs=32, max_steps=16)
    assert bool((plain.dv_e > 0).all())
    tr.set_scripted_opponent("evader", intercept(10))
    r3 = tr.evaluate(num_envs=32, max_steps=16, opponent="scripted", record=True)
    assert bool((r3.dv_e > 0).all())
    lw = tr.scripted_opponents["evader"]
    raw0 = r3.streams["obs"][0].cpu().numpy()            # step 0's output is step 1's raw input
    want = restated(raw0, lw.G, lw.b, lw.max_action)
    assert np.array_equal(_np_bits(r3.streams["evader_action"][1].cpu().numpy()), _np_bits(want))


# ---------------------------------------------------------------------------
# 9. checkpoints
# ---------------------------------------------------------------------------
def _snap(tr):
    torch.cuda.synchronize()
    out = {"obs0": tr.buf.obs[0].cpu().numpy()}
    for name, L in (("pursuer", tr.pursuer), ("evader", tr.evader)):
        for k in ("P", "M", "V", "steps", "lr"):
            out[f"{name}.{k}"] = getattr(L, k).cpu().numpy()
    for k in BUF:
        out["buf." + k] = getattr(tr.buf, k).cpu().numpy()
    return out


def test_checkpoint_carries_the_laws(tmp_path):
    from satrl.scripted import evade
    path = str(tmp_path / "ck")
    A = _trainer(0, True, law={"evader": evade(10, 0.5)})
    A.iteration()
    A.save_checkpoint(path)
    assert "scripted" in A.state_dict()
    A.iteration()
    want = _snap(A)
    for law in ({"evader": "coast"}, None):              # the saved law replaces the values in place, or is attached
        B = _trainer(0, True, law=law)
        B.load_checkpoint(path)
        assert np.array_equal(B.scripted_opponents["evader"].G, A.scripted_opponents["evader"].G)
        B.iteration()
        got = _snap(B)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), (law, k)
    # without laws: the state has no such entry and loads as it always did
    path2 = str(tmp_path / "ck2")
    C = _trainer(0, True, law=None)
    C.iteration()
    assert "scripted" not in C.state_dict()
    C.save_checkpoint(path2)
    C.iteration()
    D = _trainer(0, True, law=None)
    D.load_checkpoint(path2)
    D.iteration()
    got, want = _snap(D), _snap(C)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert D.scripted_opponents == {}
    E = _trainer(0, True, law={"evader": "coast"})       # a checkpoint without laws loads as "no laws"
    E.load_checkpoint(path2)
    assert E.scripted_opponents == {}
