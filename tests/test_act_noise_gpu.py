"""Actuation noise on the gfx950 kernels (include/satenv.h satenv_act_noise):
every step kernel against the host build and the NumPy restatement bit for
bit, with a reset box, sharding, graph replay, and the trainer, evaluator and
checkpoints on top."""
import numpy as np
import pytest
import torch

import act_noise_reference as A
import reset_dist_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 130            # two 64-env workgroups + 2 lanes; ragged at 16 and 32 envs per workgroup too
SEED = 0x1234ABCD5678EF01
OFFSET = 1000
D_CAPTURE = 1000.0  # nothing starts inside it: every episode times out on its third step
NOISE = ((0.05, 0.02), (0.2, 0.1))


def _env(n=N, device=DEV, **kw):
    from satrl.env import VecSatellites
    kw.setdefault("d_capture", D_CAPTURE)
    kw.setdefault("max_episode_steps", 3)
    if device == "cpu":
        kw.setdefault("threads", 2)
    return VecSatellites(n, device=device, **kw)


def _np(t):
    return t.cpu().numpy().copy()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _actions(n, device=DEV):
    return tuple(torch.from_numpy(a).to(device) for a in A.actions(n))


def _snap(env):
    return tuple(_np(x) for x in env.get_state()) + (_np(env.episode_index()),)


def _run7(env, n, noise=NOISE, seed=SEED, offset=OFFSET, actions=None, box=False, executed=None):
    """reset + 7 autoreset steps; every step's outputs, public state and episode
    index as numpy arrays.  noise: set on the handle (None: never).  box: with
    reset_dist_reference's box.  executed: (noise, seed, offset) -- the handle
    is fed the restatement's executed actions of those settings instead."""
    if box:
        env.set_reset_dist(R.LO, R.HI, seed ^ 0x55, env_offset=offset)
    if noise is not None:
        env.set_act_noise(*noise, seed=seed, env_offset=offset)
    pa, ea = _actions(n, env.device) if actions is None else actions
    out = [(_np(env.reset(0)),) + _snap(env)]
    for _ in range(7):
        xa = pa, ea
        if executed is not None:
            _, i32, ep = _snap(env)
            xa = A.executed_pair(executed[0], executed[1], executed[2] + np.arange(n), ep, i32[1] + 1, _np(pa), _np(ea))
            xa = tuple(torch.from_numpy(x).to(env.device) for x in xa)
        o, r, d = env.step_autoreset(*xa)
        out.append((_np(o), _np(r), _np(d)) + _snap(env))
    assert env.check_errors() == 0
    return out


def _assert_runs_equal(a, b, what):
    assert len(a) == len(b)
    for step, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for k, (p, q) in enumerate(zip(x, y)):
            assert _bits_equal(p, q), (what, step, k)


def _runs_differ(a, b):
    return any(not _bits_equal(p, q) for x, y in zip(a, b) for p, q in zip(x, y))


@pytest.fixture(scope="module")
def wide64():
    """The product kernel's noisy run (kind 2, 64 envs per workgroup): the reference of the kernel comparisons."""
    return _run7(_env(), N)


def test_product_kernel_equals_host_build_and_restatement(wide64):
    _assert_runs_equal(wide64, _run7(_env(device="cpu"), N), "host build")
    # the executed actions: a handle that never had noise, fed the restatement's a', gives the same run
    fed = _run7(_env(), N, noise=None, executed=(NOISE, SEED, OFFSET))
    _assert_runs_equal(wide64, fed, "restatement's executed actions")
    for step in range(1, 8):
        assert (wide64[step][2] == (1 if step % 3 == 0 else 0)).all(), step
    assert (wide64[7][-1] == 3).all()                      # the key's episode index advanced twice
    assert _runs_differ(wide64, _run7(_env(), N, noise=None))


@pytest.mark.parametrize("kind,wide", [(2, 32), (2, 16), (1, 64), (0, 64)])
def test_every_step_kernel_executes_the_same_actions(wide64, kind, wide):
    env = _env()
    env.set_step_kernel(kind, wide)
    _assert_runs_equal(_run7(env, N), wide64, (kind, wide))


def test_rk45_instantiation_against_itself():
    runs = []
    for _ in range(2):
        env = _env(propagator=2)
        env.set_step_kernel(1, 64)
        runs.append(_run7(env, N))
    _assert_runs_equal(runs[0], runs[1], "propagator 2")
    plain = _env(propagator=2)
    assert _runs_differ(runs[0], _run7(plain, N, noise=None))


def test_noise_with_a_reset_box():
    run = _run7(_env(), N, box=True)
    gid = OFFSET + np.arange(N)
    for ep, step in enumerate((0, 3, 6)):                  # the starts are still the box's draws
        want = R.expected_draw(R.LO, R.HI, SEED ^ 0x55, gid, ep)
        assert _bits_equal(run[step][-3][:12], want), step
        assert _bits_equal(run[step][0], R.obs_of(want).astype(np.float32)), step
        assert (run[step][-1] == ep + 1).all()
    _assert_runs_equal(run, _run7(_env(device="cpu"), N, box=True), "host build")
    # float velocities from the first step on: the executed actions move every kinematic plane
    fed = _run7(_env(), N, noise=None, box=True, executed=(NOISE, SEED, OFFSET))
    _assert_runs_equal(run, fed, "restatement's executed actions")
    assert not _bits_equal(run[1][-3][3:6], _run7(_env(), N, noise=None, box=True)[1][-3][3:6])


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


def _prepared(noise):
    """A handle after reset and one throw-away step (lazy initialisation before
    a capture), back at the reset's state; its output buffers."""
    env = _env()
    if noise is not None:
        env.set_act_noise(noise, noise, seed=SEED, env_offset=OFFSET)
    env.reset(0)
    f, i = env.get_state()
    ep = env.episode_index()
    pa, ea = _actions(N)
    out = (torch.empty((N, 18), dtype=torch.float32, device=DEV), torch.empty(N, dtype=torch.float32, device=DEV),
           torch.empty(N, dtype=torch.uint8, device=DEV))
    env.step_autoreset(pa, ea, obs_out=out[0], reward_out=out[1], done_out=out[2])
    env.set_state(f, i)
    env.set_episode_index(ep)
    env.set_episode_return(None)
    torch.cuda.synchronize()
    return env, pa, ea, out


def _three(env, pa, ea, out):
    for _ in range(3):
        env.step_autoreset(pa, ea, obs_out=out[0], reward_out=out[1], done_out=out[2])


def _seg(env, out):
    torch.cuda.synchronize()
    return tuple(_np(x) for x in out) + _snap(env) + (_np(env.episode_return()),)


def test_set_act_noise_between_graph_replays_needs_no_recapture():
    env, pa, ea, out = _prepared((0.05, 0.02))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _three(env, pa, ea, out)
    ref, rpa, rea, rout = _prepared((0.05, 0.02))         # the same settings, eager
    g.replay()
    _three(ref, rpa, rea, rout)
    first = _seg(env, out)
    assert all(_bits_equal(p, q) for p, q in zip(first, _seg(ref, rout))) and (first[2] == 1).all()
    for e in (env, ref):                                   # same stream, before the replay
        e.set_act_noise((0.2, 0.1), (0.2, 0.1), seed=SEED ^ 0xFFFF, env_offset=OFFSET + 7)
    g.replay()
    _three(ref, rpa, rea, rout)
    second = _seg(env, out)
    assert all(_bits_equal(p, q) for p, q in zip(second, _seg(ref, rout)))
    # ... and it was the new setting that ran: the old one gives other bits from the same state
    old, opa, oea, oout = _prepared((0.05, 0.02))
    old.set_state(*(torch.from_numpy(x).to(DEV) for x in first[3:5]))
    old.set_episode_index(torch.from_numpy(first[5]).to(DEV))
    _three(old, opa, oea, oout)
    assert not _bits_equal(_seg(old, oout)[3], second[3])
    # disabled: the replay is a handle's run that never had noise, from the same state
    env.clear_act_noise()
    g.replay()
    third = _seg(env, out)
    plain, ppa, pea, pout = _prepared(None)
    plain.set_state(*(torch.from_numpy(x).to(DEV) for x in second[3:5]))
    plain.set_episode_index(torch.from_numpy(second[5]).to(DEV))
    plain.set_episode_return(torch.from_numpy(second[6]).to(DEV))
    _three(plain, ppa, pea, pout)
    assert not plain.noisy and all(_bits_equal(p, q) for p, q in zip(third, _seg(plain, pout)))
    assert env.check_errors() == 0


# -- trainer / evaluator / checkpoints -----------------------------------------------------------
TN, TT = 64, 16
SPEC = (0.05, 0.02)


def _args(**kw):
    from satrl.trainer import args_param
    base = dict(chkpt_dir="/tmp", num_envs=TN, horizon=TT, batch_size=TN * TT, hidden_width=64, mini_batch_size=256,
                K_epochs=1, max_episode_steps=3, seed=11, rollout_graph_chunk=4, update_graph_group=2, act_noise=SPEC)
    base.update(kw)
    return args_param(**base)


def _trainer(graphs=True, **kw):
    from satrl.trainer import VecTrainer
    return VecTrainer(_args(**kw), flag=0, d_capture=D_CAPTURE, use_graphs=graphs)


def _rollout(tr):
    torch.cuda.synchronize()
    return {"obs": _np(tr.buf.obs), "rew": _np(tr.buf.rew), "done": _np(tr.buf.done), "act": _np(tr.buf.act),
            "P": _np(tr.learner.P), "ep": _np(tr.env.episode_index())}


def test_trainer_iterations_with_and_without_graphs():
    got = []
    for graphs in (True, False):
        tr = _trainer(graphs)
        assert tr.env.noisy and tr.env.act_noise() == {"pursuer": SPEC, "evader": SPEC, "seed": 11, "env_offset": 0}
        tr.iteration()
        tr.iteration()
        got.append(_rollout(tr))
    for k in got[0]:
        assert _bits_equal(got[0][k], got[1][k]), k
    plain = _trainer(True, act_noise=None)
    plain.iteration()
    plain.iteration()
    assert not plain.env.noisy and not _bits_equal(_rollout(plain)["obs"], got[0]["obs"])


def test_buffer_keeps_the_commanded_actions():
    """Against a coasting evader (zero actions, which the noise leaves zero) the
    rollout is reproduced on a host handle WITHOUT noise that is fed the
    restatement's executed actions of the buffer's stored ones: so the stored
    ones are the commanded actions, and the env ran the executed ones."""
    tr = _trainer(True, scripted_opponent="coast", act_noise_seed=77)
    f, i = tr.env.get_state()
    ep = tr.env.episode_index()
    tr.iteration()
    got = _rollout(tr)
    host = _env(TN, device="cpu")
    host.set_state(f.cpu(), i.cpu())
    host.set_episode_index(ep.cpu())
    zeros = torch.zeros((TN, 3), dtype=torch.float32)
    moved = 0
    for t in range(TT):
        cnt = host.get_state()[1][1].numpy() + 1
        a = A.clip16(got["act"][t])
        x = A.executed(SPEC[0], SPEC[1], 77, 0, np.arange(TN), host.episode_index().numpy(), cnt, a)
        moved += int((x != a).any(axis=1).sum())
        o, r, d = host.step_autoreset(torch.from_numpy(x), zeros)
        assert _bits_equal(o.numpy(), got["obs"][t + 1]), t
        assert _bits_equal(r.numpy(), got["rew"][t]) and _bits_equal(d.numpy(), got["done"][t]), t
    # (a row whose three components all sit on the +-1.6 clip may keep its bits)
    assert moved > TT * TN // 2 and (got["ep"] == 1 + TT // 3).all()


def test_set_act_noise_between_iterations_replays_the_captured_graphs():
    tr = _trainer(True, act_noise=None)              # built without noise: the step kernels without it
    tr.iteration()
    torch.cuda.synchronize()
    assert tr._graphs and not tr.env.noisy and tr.env.act_noise() is None
    tr.set_act_noise(SPEC)                           # the trainer's first noise: those graphs are dropped
    assert not tr._graphs and tr.env.noisy and tr.env.act_noise()["seed"] == 11
    tr.iteration()
    graphs = dict(tr._graphs)
    assert graphs
    tr.set_act_noise({"pursuer": (0.2, 0.1)}, seed=12)       # a curriculum step: the same graphs
    assert tr.env.act_noise() == {"pursuer": (0.2, 0.1), "evader": (0.0, 0.0), "seed": 12, "env_offset": 0}
    tr.iteration()
    assert tr._graphs.keys() == graphs.keys() and all(tr._graphs[k] is g for k, g in graphs.items())
    tr.set_act_noise(None)                           # off again: the same graphs
    tr.iteration()
    torch.cuda.synchronize()
    assert all(tr._graphs[k] is g for k, g in graphs.items()) and tr.env.act_noise() is None
    from satrl.trainer import VecTrainer
    off = VecTrainer(_args(), flag=0, d_capture=D_CAPTURE, env_offset=320, use_graphs=False)
    assert off.env.act_noise()["env_offset"] == 320  # data-parallel shards draw by global env id


REC = ("ret", "final_dis", "min_dis", "dv_p", "dv_e", "length", "outcome")


def test_evaluate_under_noise():
    tr, plain = _trainer(), _trainer(act_noise=None)
    tr.iteration()
    plain.learner.P.copy_(tr.learner.P)
    plain.learner.sync_w2t()
    torch.cuda.synchronize()
    before = (_np(tr.pursuer.P), _np(tr.evader.P)) + _snap(tr.env) + (tr.rollout_steps, tr.env.act_noise())
    a = tr.evaluate(deterministic="both")
    b = tr.evaluate(deterministic="both")
    none = tr.evaluate(deterministic="both", act_noise=None)
    wide = tr.evaluate(deterministic="both", act_noise={"pursuer": (0.5, 0.5)})
    again = tr.evaluate(deterministic="both")                     # after other settings on the same handle
    p = plain.evaluate(deterministic="both")
    for name in REC:
        x = _np(getattr(a, name))
        assert _bits_equal(x, _np(getattr(b, name))) and _bits_equal(x, _np(getattr(again, name))), name
        assert _bits_equal(_np(getattr(none, name)), _np(getattr(p, name))), name
    assert a.summary() == b.summary()
    # one scenario (the fixed reset, both agents' means): only the noise tells the envs apart
    assert len(np.unique(_np(p.ret))) == 1 and len(np.unique(_np(a.ret))) > 1
    assert not _bits_equal(_np(a.ret), _np(wide.ret))
    after = (_np(tr.pursuer.P), _np(tr.evader.P)) + _snap(tr.env) + (tr.rollout_steps, tr.env.act_noise())
    for x, y in zip(before[:5], after[:5]):
        assert _bits_equal(x, y)
    assert before[5:] == after[5:]
    with pytest.raises(ValueError):
        tr.evaluate(act_noise="on")


def test_checkpoint_resumes_bitwise_under_noise(tmp_path):
    path = str(tmp_path / "ck")
    A_ = _trainer(act_noise={"pursuer": SPEC, "evader": (0.2, 0.1)}, act_noise_seed=5)
    A_.iteration()
    A_.save_checkpoint(path)
    A_.iteration()
    want = _rollout(A_)
    for kw in (dict(act_noise={"pursuer": SPEC, "evader": (0.2, 0.1)}, act_noise_seed=5), dict(act_noise=None)):
        B = _trainer(**kw)                                        # the checkpoint carries the spec and the seed
        B.load_checkpoint(path)
        assert B.env.act_noise() == {"pursuer": SPEC, "evader": (0.2, 0.1), "seed": 5, "env_offset": 0}
        B.iteration()
        got = _rollout(B)
        for k in want:
            assert _bits_equal(got[k], want[k]), (k, kw)
