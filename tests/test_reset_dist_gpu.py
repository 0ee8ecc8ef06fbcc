"""Randomised episode starts on the gfx950 kernels (include/satenv.h
satenv_reset_dist): every step kernel against the NumPy restatement bit for
bit, sharding, graph replay, and the trainer / evaluator on top."""
import numpy as np
import pytest
import torch

import reset_dist_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 130            # two 64-env workgroups + 2 lanes; ragged at 16 and 32 envs per workgroup too
SEED = 0x1234ABCD5678EF01
OFFSET = 1000
D_CAPTURE = 1000.0  # no start of the box is inside it: every episode times out on its third step


def _env(n=N, device=DEV, **kw):
    from satrl.env import VecSatellites
    kw.setdefault("d_capture", D_CAPTURE)
    kw.setdefault("max_episode_steps", 3)
    if device == "cpu":
        kw.setdefault("threads", 2)
    return VecSatellites(n, device=device, **kw)


def _np(t):
    return t.cpu().numpy().copy()


def _kin(env):
    return _np(env.get_state()[0][:12])


def _vel_int(env):
    return (_np(env.get_state()[1][2]) >> 4) & 1


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _actions(n, device=DEV):
    return tuple(torch.from_numpy(a).to(device) for a in R.fixed_actions(n))


def _run7(env, n, seed=SEED, offset=OFFSET, actions=None):
    """reset + 7 autoreset steps under the box; every step's outputs, public
    state and episode index as numpy arrays."""
    env.set_reset_dist(R.LO, R.HI, seed, env_offset=offset)
    pa, ea = _actions(n, env.device) if actions is None else actions
    out = [(_np(env.reset(0)),) + tuple(_np(x) for x in env.get_state()) + (_np(env.episode_index()),)]
    for _ in range(7):
        o, r, d = env.step_autoreset(pa, ea)
        out.append((_np(o), _np(r), _np(d)) + tuple(_np(x) for x in env.get_state()) + (_np(env.episode_index()),))
    assert env.check_errors() == 0
    return out


def _assert_runs_equal(a, b, what):
    assert len(a) == len(b)
    for step, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for k, (p, q) in enumerate(zip(x, y)):
            assert _bits_equal(p, q), (what, step, k)


def _assert_draws(run, n, seed=SEED, offset=OFFSET):
    """The kinematics and obs after the reset (entry 0) and after the autoresets
    of steps 3 and 6 are the restatement's draws of episodes 0, 1, 2."""
    gid = offset + np.arange(n)
    for ep, step in enumerate((0, 3, 6)):
        want = R.expected_draw(R.LO, R.HI, seed, gid, ep)
        f64, i32, idx = run[step][-3:]
        assert _bits_equal(f64[:12], want), step
        assert _bits_equal(run[step][0], R.obs_of(want).astype(np.float32)), step
        assert (((i32[2] >> 4) & 1) == 0).all()
        assert (idx == ep + 1).all()
    for step in range(1, 8):
        assert (run[step][2] == (1 if step % 3 == 0 else 0)).all(), step
    assert (run[7][-1] == 3).all()


@pytest.fixture(scope="module")
def wide64():
    """The product kernel's run (kind 2, 64 envs per workgroup): the reference of the kernel comparisons."""
    return _run7(_env(), N)


def test_gpu_draws_equal_restatement_and_host_build(wide64):
    _assert_draws(wide64, N)
    host = _run7(_env(device="cpu"), N)
    for step in (0, 3, 6):                 # the states right after a reset: bit for bit the host build's
        assert _bits_equal(wide64[step][-3][:12], host[step][-3][:12]), step
        assert _bits_equal(wide64[step][-1], host[step][-1])


@pytest.mark.parametrize("kind,wide", [(2, 32), (2, 16), (1, 64), (0, 64)])
def test_every_step_kernel_draws_the_same(wide64, kind, wide):
    env = _env()
    env.set_step_kernel(kind, wide)
    _assert_runs_equal(_run7(env, N), wide64, (kind, wide))


def test_rk45_instantiation_draws_the_same_starts():
    runs = []
    for _ in range(2):
        env = _env(propagator=2)
        env.set_step_kernel(1, 64)
        runs.append(_run7(env, N))
    _assert_runs_equal(runs[0], runs[1], "propagator 2")
    _assert_draws(runs[0], N)


def test_sharding_invariance():
    pa, ea = _actions(256)
    whole = _run7(_env(256), 256, offset=0, actions=(pa, ea))
    parts = [_run7(_env(128), 128, offset=o, actions=(pa[o:o + 128].contiguous(), ea[o:o + 128].contiguous()))
             for o in (0, 128)]
    for step in range(8):
        for k, x in enumerate(whole[step]):
            axis = 1 if x.ndim == 2 and x.shape[0] in (15, 3) else 0      # state planes are [planes, N]
            y = np.concatenate([parts[0][step][k], parts[1][step][k]], axis=axis)
            assert _bits_equal(x, y), (step, k)


def test_set_reset_dist_between_graph_replays_needs_no_recapture():
    env = _env()
    pa, ea = _actions(N)
    obs = torch.empty((N, 18), dtype=torch.float32, device=DEV)
    rew = torch.empty(N, dtype=torch.float32, device=DEV)
    done = torch.empty(N, dtype=torch.uint8, device=DEV)
    env.set_reset_dist(R.LO, R.HI, SEED, env_offset=OFFSET)
    env.reset(0)
    env.step_autoreset(pa, ea, obs_out=obs, reward_out=rew, done_out=done)      # lazy initialisation before capture
    env.set_episode_index(None)
    env.reset(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(3):
            env.step_autoreset(pa, ea, obs_out=obs, reward_out=rew, done_out=done)
    gid = OFFSET + np.arange(N)
    g.replay()
    torch.cuda.synchronize()
    assert (_np(done) == 1).all()
    first = _kin(env)
    assert _bits_equal(first, R.expected_draw(R.LO, R.HI, SEED, gid, 1))
    other = SEED ^ 0xFFFF
    env.set_reset_dist(R.LO, R.HI - 1.0, other, env_offset=OFFSET + 7)          # same stream, before the replay
    g.replay()
    torch.cuda.synchronize()
    second = _kin(env)
    assert _bits_equal(second, R.expected_draw(R.LO, R.HI - 1.0, other, gid + 7, 2))
    assert not _bits_equal(second, R.expected_draw(R.LO, R.HI, SEED, gid, 2))
    assert _bits_equal(_np(obs), R.obs_of(second).astype(np.float32))
    assert (_np(env.episode_index()) == 3).all()


# -- trainer / evaluator ---------------------------------------------------------------------
TN, TT = 64, 8


def _args(**kw):
    from satrl.trainer import args_param
    base = dict(chkpt_dir="/tmp", num_envs=TN, horizon=TT, batch_size=TN * TT, hidden_width=64, mini_batch_size=64,
                K_epochs=1, max_episode_steps=3, seed=11, rollout_graph_chunk=4, update_graph_group=2,
                reset_spread=list(R.HALF))
    base.update(kw)
    return args_param(**base)


def _trainer(graphs=True, **kw):
    from satrl.trainer import VecTrainer
    return VecTrainer(_args(**kw), flag=0, d_capture=D_CAPTURE, use_graphs=graphs)


def test_trainer_rollout_starts_are_the_draws_with_and_without_graphs():
    got = []
    for graphs in (True, False):
        tr = _trainer(graphs)
        box = tr.env.reset_dist
        assert _bits_equal(box["lo"], R.LO) and _bits_equal(box["hi"], R.HI) and box["seed"] == 11
        obs0 = _np(tr.buf.obs[0])                # (the iteration's end moves the last row here)
        tr.iteration()
        torch.cuda.synchronize()
        got.append((_np(tr.buf.obs), _np(tr.buf.rew), _np(tr.buf.done), _np(tr.env.episode_index()), obs0))
    for a, b in zip(*got):
        assert _bits_equal(a, b)
    obs, _, done, idx, obs0 = got[0]
    gid = np.arange(TN)
    assert _bits_equal(obs0, R.obs_of(R.expected_draw(R.LO, R.HI, 11, gid, 0)).astype(np.float32))
    assert _bits_equal(obs[0], obs[TT])
    ep = np.zeros(TN, dtype=np.int64)
    resets = 0
    for t in range(TT):
        d = done[t] != 0
        if d.any():
            ep[d] += 1
            want = R.obs_of(R.expected_draw(R.LO, R.HI, 11, gid[d], ep[d])).astype(np.float32)
            assert _bits_equal(obs[t + 1][d], want), t
            resets += int(d.sum())
    assert resets == 2 * TN and (ep == 2).all() and (idx == 3).all()


def _assert_rollout_draws(tr, lo, hi, seed, ep):
    """Every buf.obs[t + 1] row behind a done step of the last rollout is the
    draw of that env's next episode index; ep: the indices before the rollout
    (updated in place).  Returns the number of resets."""
    obs, done = _np(tr.buf.obs), _np(tr.buf.done)
    gid, resets = tr.env_offset + np.arange(tr.N), 0
    for t in range(tr.T):
        d = done[t] != 0
        if d.any():
            want = R.obs_of(R.expected_draw(lo, hi, seed, gid[d], ep[d])).astype(np.float32)
            assert _bits_equal(obs[t + 1][d], want), t
            ep[d] += 1
            resets += int(d.sum())
    assert _bits_equal(ep.astype(np.int32), _np(tr.env.episode_index()))
    return resets


def test_set_reset_spread_between_iterations_replays_the_captured_graphs():
    tr = _trainer(True, reset_spread=None)           # built without a box: the step kernels without the draw
    tr.iteration()
    torch.cuda.synchronize()
    ep = _np(tr.env.episode_index()).astype(np.int64)
    assert (ep == 3).all() and tr._graphs and not tr.env.draws
    tr.set_reset_spread(list(R.HALF))                # the trainer's first box: those graphs are dropped
    assert not tr._graphs and tr.env.draws
    tr.iteration()
    torch.cuda.synchronize()
    assert _assert_rollout_draws(tr, R.LO, R.HI, 11, ep) == 3 * TN
    graphs = dict(tr._graphs)
    tr.set_reset_spread({"lo": R.LO, "hi": R.HI + 3.0}, seed=12)      # a curriculum step: the same graphs
    tr.iteration()
    torch.cuda.synchronize()
    assert tr._graphs.keys() == graphs.keys() and all(tr._graphs[k] is g for k, g in graphs.items())
    assert _assert_rollout_draws(tr, R.LO, R.HI + 3.0, 12, ep) >= 2 * TN
    tr.set_reset_spread(None)                        # off again: the same graphs, the fixed reset
    tr.iteration()
    torch.cuda.synchronize()
    assert all(tr._graphs[k] is g for k, g in graphs.items())
    obs, done = _np(tr.buf.obs), _np(tr.buf.done)
    fixed = R.obs_of(R.CENTRE[:, None]).astype(np.float32)[0]
    rows = obs[1:][done != 0]
    assert len(rows) >= 2 * TN and (rows == fixed).all()


def test_trainer_reset_seed_offset_and_set_reset_spread():
    from satrl.trainer import VecTrainer
    tr = VecTrainer(_args(reset_seed=99), flag=0, d_capture=D_CAPTURE, env_offset=320, use_graphs=False)
    gid = 320 + np.arange(TN)
    assert _bits_equal(_np(tr.buf.obs[0]), R.obs_of(R.expected_draw(R.LO, R.HI, 99, gid, 0)).astype(np.float32))
    tr.set_reset_spread({"lo": R.LO, "hi": R.HI + 3.0})
    tr._reset_obs()
    want = R.expected_draw(R.LO, R.HI + 3.0, 99, gid, 1)
    assert _bits_equal(_kin(tr.env), want)
    tr.set_reset_spread(None)
    assert tr.env.reset_dist is None
    tr._reset_obs()
    assert _bits_equal(_kin(tr.env), np.repeat(R.CENTRE[:, None], TN, axis=1))


def test_obs_norm_calibration_restores_the_episode_index():
    tr = _trainer(False, obs_norm=True, obs_norm_calib_steps=7)      # 7 throw-away steps: two autoresets per env
    assert (_np(tr.env.episode_index()) == 1).all()                   # as the first _reset_obs() left it
    assert _bits_equal(_kin(tr.env), R.expected_draw(R.LO, R.HI, 11, np.arange(TN), 0))


def test_evaluate_is_a_fixed_set_of_distinct_scenarios():
    from satrl.evaluate import EVAL_SEED_XOR
    tr = _trainer()
    a = tr.evaluate(deterministic="both")
    b = tr.evaluate(deterministic="both")
    want = R.expected_draw(R.LO, R.HI, 11 ^ EVAL_SEED_XOR, np.arange(TN), 0)
    assert _bits_equal(_np(a.start), want) and _bits_equal(_np(b.start), want)
    assert len({want[:, i].tobytes() for i in range(TN)}) == TN
    for name in ("ret", "final_dis", "min_dis", "dv_p", "dv_e", "length", "outcome"):
        assert _bits_equal(_np(getattr(a, name)), _np(getattr(b, name))), name
    assert a.summary() == b.summary()
    ret = _np(a.ret)
    assert len(np.unique(ret)) > 1                 # N scenarios, not one
    c = tr.evaluate(deterministic="both", seed=5)
    assert _bits_equal(_np(c.start), R.expected_draw(R.LO, R.HI, 5, np.arange(TN), 0))
    # the training env is not touched
    assert (_np(tr.env.episode_index()) == 1).all()
    # without the box every env plays the one scenario of the fixed reset
    plain = _trainer(reset_spread=None)
    p = plain.evaluate(deterministic="both")
    assert len(np.unique(_np(p.ret))) == 1
    assert _bits_equal(_np(p.start), np.repeat(R.CENTRE[:, None], TN, axis=1))
    # states= keeps its meaning: no reset, no draw, the same records with and without the box
    f, i = tr.env.get_state()
    f = f.clone()
    f[0] += torch.arange(TN, dtype=torch.float64, device=f.device) * 100.0
    s1 = tr.evaluate(deterministic="both", states=(f, i))
    s2 = plain.evaluate(deterministic="both", states=(f, i))
    assert _bits_equal(_np(s1.start), _np(f[:12])) and _bits_equal(_np(s2.start), _np(f[:12]))
    for name in ("ret", "final_dis", "min_dis", "dv_p", "dv_e", "length", "outcome"):
        assert _bits_equal(_np(getattr(s1, name)), _np(getattr(s2, name))), name
