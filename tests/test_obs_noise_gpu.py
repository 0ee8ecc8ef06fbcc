"""Observation noise on the gfx950 kernels (include/satenv.h satenv_obs_noise):
every step kernel and the reset kernel against the host build and the NumPy
restatement bit for bit, with a reset box and actuation noise, sharding and
graph replay, and the trainer, evaluator and checkpoints on top.  Every
comparison is bitwise."""
import numpy as np
import pytest
import torch

import obs_noise_reference as R
from reset_dist_reference import HI, LO

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 200            # three full 64-env workgroups and a ragged 8; ragged at 16 and 32 envs per workgroup too
T, MAX_STEPS, HOLD = 12, 5, 3       # two autoresets, four refresh windows
SEED = 0x0BADC0DE12345678
OFFSET = 2 ** 32 - 70               # the global ids straddle the counter's second word
D_CAPTURE = 1000.0                  # nothing starts inside it: every episode times out on its fifth step
KEYS = ("bias_pos", "bias_vel", "pos", "vel")
BOTH = ((120.0, 0.04, 35.0, 0.015), (300.0, 0.08, 60.0, 0.03))
SPEC = {"pursuer": dict(zip(KEYS, BOTH[0])), "evader": dict(zip(KEYS, BOTH[1]))}
ACT = ((0.05, 0.02), (0.2, 0.1))


def _env(n=N, device=DEV, **kw):
    from satrl.env import VecSatellites
    kw.setdefault("d_capture", D_CAPTURE)
    kw.setdefault("max_episode_steps", MAX_STEPS)
    if device == "cpu":
        kw.setdefault("threads", 2)
    return VecSatellites(n, device=device, **kw)


def _np(t):
    return t.cpu().numpy().copy()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _actions(n=N, t=T, first=0):
    """f32 [2, t, n, 3]: the rows of envs first .. first + n of one fixed pseudo-random table."""
    table = np.random.default_rng(11).uniform(-1.6, 1.6, (2, T, 256, 3)).astype(np.float32)
    return torch.from_numpy(table[:, :t, first:first + n].copy())


def _setup(env, noise, offset, extras):
    if extras:
        env.set_reset_dist(LO, HI, SEED ^ 1, env_offset=offset)
        env.set_act_noise(*ACT, seed=SEED ^ 2, env_offset=offset)
    if noise:
        env.set_obs_noise(SPEC["pursuer"], SPEC["evader"], hold=HOLD, seed=SEED, env_offset=offset)


def _rec(env, obs, **more):
    f, i = env.get_state()
    return dict(obs=_np(obs), f64=_np(f), i32=_np(i), ep=_np(env.episode_index()),
                **{k: _np(v) for k, v in more.items()})


def _run(env, n=N, noise=True, offset=OFFSET, extras=False, first=0):
    """reset + T autoreset steps: per write the f32 row and the handle's state (the truth)."""
    _setup(env, noise, offset, extras)
    act = _actions(n, first=first).to(env.device)
    out = [_rec(env, env.reset(0))]
    for t in range(T):
        o, r, d = env.step_autoreset(act[0, t], act[1, t])
        out.append(_rec(env, o, rew=r, done=d))
    assert env.check_errors() == 0          # (env.stats is left out: f64 atomics sum it in wave order)
    return out


def _run_step(env, n=N, noise=True, offset=OFFSET):
    """The same through satenv_step + satenv_reset: the done envs are reset by a mask, so every such
    reset rewrites the rows of the envs it leaves alone; obs64 rides along."""
    _setup(env, noise, offset, False)
    act = _actions(n).to(env.device)
    dev = env.device
    obs64 = torch.empty((n, 18), dtype=torch.float64, device=dev)
    odd = (torch.arange(n, device=dev) % 3 == 0).to(torch.uint8)
    out = [_rec(env, env.reset(0, obs64_out=obs64, obs_out=torch.empty((n, 18), dtype=torch.float32, device=dev)),
                obs64=obs64)]
    for t in range(T):
        o = torch.empty((n, 18), dtype=torch.float32, device=dev)
        _, r, d = env.step(act[0, t], act[1, t], None, obs_out=o, obs64_out=obs64)
        out.append(_rec(env, o, obs64=obs64, rew=r, done=d))
        mask = d if bool(d.any()) else (odd if t == 1 else None)       # step 2: a third restarts early
        if mask is not None:
            o = torch.empty((n, 18), dtype=torch.float32, device=dev)
            env.reset(0, mask=mask, obs_out=o, obs64_out=obs64)
            out.append(_rec(env, o, obs64=obs64, mask=mask))
    assert env.check_errors() == 0
    return out


def _assert_runs_equal(a, b, what, but=()):
    assert len(a) == len(b)
    for step, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            if k not in but:
                assert _bits_equal(x[k], y[k]), (what, step, k)


def _assert_measured(run, offset=OFFSET, spec=BOTH, hold=HOLD, seed=SEED):
    """Every f32 row of the run is the restatement of the truth beside it at the planes' (ep, cnt)."""
    for step, x in enumerate(run):
        truth = x["f64"][0:12].T
        n = truth.shape[0]
        want = R.row_of(R.measured(spec, hold, seed, offset + np.arange(n), x["ep"], x["i32"][1], truth))
        assert _bits_equal(x["obs"], want), step
        assert (x["obs"] != R.row_of(truth)).any(axis=1).all(), step
        if "obs64" in x:
            assert _bits_equal(x["obs64"], np.concatenate([truth[:, 0:6] - truth[:, 6:12], truth], axis=1)), step


@pytest.fixture(scope="module")
def wide64():
    """The product kernel's run (kind 2, 64 envs per workgroup): the reference of the kernel comparisons."""
    return _run(_env())


@pytest.fixture(scope="module")
def wide64_step():
    return _run_step(_env())


def test_autoreset_kernel_equals_host_build_and_restatement(wide64):
    _assert_runs_equal(wide64, _run(_env(device="cpu")), "host build")
    _assert_measured(wide64)
    for t in range(T + 1):
        assert (wide64[t]["i32"][1] == t % MAX_STEPS).all() and (wide64[t]["ep"] == 1 + t // MAX_STEPS).all(), t
    # ... and nothing but the f32 row differs from a handle that never had the noise
    plain = _env()
    _assert_runs_equal(wide64, _run(plain, noise=False), "no noise", but=("obs",))
    assert not plain.measures


def test_step_and_masked_reset_equal_host_build_and_restatement(wide64_step):
    _assert_runs_equal(wide64_step, _run_step(_env(device="cpu")), "host build")
    _assert_measured(wide64_step)
    masks = [x["mask"] for x in wide64_step if "mask" in x]
    assert len(masks) == 5 and all(0 < int(m.sum()) < N for m in masks)   # every one leaves rows to rewrite
    _assert_runs_equal(wide64_step, _run_step(_env(), noise=False), "no noise", but=("obs",))


@pytest.mark.parametrize("kind,wide", [(2, 32), (2, 16), (1, 64), (0, 64)])
def test_every_schedule_writes_the_same_rows(wide64, wide64_step, kind, wide):
    env = _env()
    env.set_step_kernel(kind, wide)
    _assert_runs_equal(_run(env), wide64, (kind, wide))
    env = _env()
    env.set_step_kernel(kind, wide)
    _assert_runs_equal(_run_step(env), wide64_step, (kind, wide, "step"))


def test_rk45_instantiation():
    runs = []
    for noise in (True, False):
        env = _env(propagator=2)
        env.set_step_kernel(1, 64)
        runs.append(_run(env, noise=noise))
    _assert_runs_equal(runs[0], runs[1], "propagator 2", but=("obs",))
    _assert_measured(runs[0])


def test_with_a_reset_box_and_act_noise():
    run = _run(_env(), extras=True)
    _assert_measured(run)
    _assert_runs_equal(run, _run(_env(device="cpu"), extras=True), "host build")
    _assert_runs_equal(run, _run(_env(), noise=False, extras=True), "no obs noise", but=("obs",))
    assert not _bits_equal(run[MAX_STEPS]["f64"][0:12], run[0]["f64"][0:12])      # the box did draw other starts


def test_sharding_invariance(wide64):
    whole = _run(_env(), offset=0)
    parts = [_run(_env(n), n, offset=o, first=o) for o, n in ((0, 128), (128, 72))]
    for step in range(T + 1):
        for k, x in whole[step].items():
            axis = 1 if k in ("f64", "i32") else 0
            y = np.concatenate([parts[0][step][k], parts[1][step][k]], axis=axis)
            assert _bits_equal(x, y), (step, k)
    assert not _bits_equal(whole[1]["obs"], wide64[1]["obs"])                    # the offset is part of the key


def _prepared(noise):
    """A handle after reset and one throw-away step (lazy initialisation before a capture), back at
    the reset's state; its actions and output buffers."""
    env = _env()
    if noise:
        env.set_obs_noise(SPEC["pursuer"], SPEC["evader"], hold=HOLD, seed=SEED, env_offset=OFFSET)
    env.reset(0)
    f, i = env.get_state()
    ep = env.episode_index()
    act = _actions(N, 1).to(DEV)
    out = (torch.empty((N, 18), dtype=torch.float32, device=DEV), torch.empty(N, dtype=torch.float32, device=DEV),
           torch.empty(N, dtype=torch.uint8, device=DEV))
    env.step_autoreset(act[0, 0], act[1, 0], obs_out=out[0], reward_out=out[1], done_out=out[2])
    env.set_state(f, i)
    env.set_episode_index(ep)
    env.set_episode_return(None)
    torch.cuda.synchronize()
    return env, act, out


def _three(env, act, out):
    for _ in range(3):
        env.step_autoreset(act[0, 0], act[1, 0], obs_out=out[0], reward_out=out[1], done_out=out[2])


def _seg(env, out):
    torch.cuda.synchronize()
    return _rec(env, out[0], rew=out[1], done=out[2], ret=env.episode_return())


def _truth_row(seg):
    return R.row_of(seg["f64"][0:12].T)


def test_set_obs_noise_between_graph_replays_needs_no_recapture():
    env, act, out = _prepared(True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _three(env, act, out)
    ref, ract, rout = _prepared(True)                      # the same settings, eager
    gid = OFFSET + np.arange(N)
    wide = {"bias_pos": 1000.0, "vel": 0.5}
    settings = [None,                                                                     # as captured
                lambda e: e.set_obs_noise(wide, SPEC["evader"], hold=HOLD, seed=SEED ^ 0xFFFF, env_offset=OFFSET),
                lambda e: e.set_obs_noise(wide, SPEC["evader"], hold=1, seed=SEED ^ 0xFFFF, env_offset=OFFSET),
                lambda e: e.clear_obs_noise(),
                lambda e: e.set_obs_noise(SPEC["pursuer"], SPEC["evader"], hold=2, seed=SEED, env_offset=OFFSET)]
    specs = [(BOTH, HOLD, SEED), ((R.craft_of(wide), BOTH[1]), HOLD, SEED ^ 0xFFFF),
             ((R.craft_of(wide), BOTH[1]), 1, SEED ^ 0xFFFF), None, (BOTH, 2, SEED)]
    for setting, spec in zip(settings, specs):
        if setting is not None:
            for e in (env, ref):                           # same stream, before the replay
                setting(e)
        g.replay()
        _three(ref, ract, rout)
        a, b = _seg(env, out), _seg(ref, rout)
        assert all(_bits_equal(a[k], b[k]) for k in a), specs.index(spec)
        truth = a["f64"][0:12].T
        if spec is None:
            assert _bits_equal(a["obs"], _truth_row(a)) and env.obs_noise() is None
        else:
            want = R.row_of(R.measured(spec[0], spec[1], spec[2], gid, a["ep"], a["i32"][1], truth))
            assert _bits_equal(a["obs"], want), specs.index(spec)
    assert env.check_errors() == 0


def test_a_graph_captured_before_the_first_enable_keeps_exact_observations():
    env, act, out = _prepared(False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _three(env, act, out)
    env.set_obs_noise(SPEC["pursuer"], SPEC["evader"], hold=HOLD, seed=SEED, env_offset=OFFSET)
    assert env.measures
    g.replay()                                             # the kernels it holds cannot measure
    a = _seg(env, out)
    assert _bits_equal(a["obs"], _truth_row(a))
    _three(env, act, out)                                  # a launch of today's can
    b = _seg(env, out)
    want = R.row_of(R.measured(BOTH, HOLD, SEED, OFFSET + np.arange(N), b["ep"], b["i32"][1], b["f64"][0:12].T))
    assert _bits_equal(b["obs"], want) and not _bits_equal(b["obs"], _truth_row(b))


# -- trainer / evaluator / checkpoints -----------------------------------------------------------
TN, TT = 64, 8
TSPEC = dict(SPEC, hold=HOLD)


def _args(**kw):
    from satrl.trainer import args_param
    base = dict(chkpt_dir="/tmp", num_envs=TN, horizon=TT, batch_size=TN * TT, hidden_width=64, mini_batch_size=64,
                K_epochs=1, max_episode_steps=MAX_STEPS, seed=11, rollout_graph_chunk=4, update_graph_group=2,
                obs_noise=TSPEC)
    base.update(kw)
    return args_param(**base)


def _trainer(graphs=True, **kw):
    from satrl.trainer import VecTrainer
    return VecTrainer(_args(**kw), flag=0, d_capture=D_CAPTURE, use_graphs=graphs)


def _rollout(tr):
    torch.cuda.synchronize()
    out = {"obs": _np(tr.buf.obs), "rew": _np(tr.buf.rew), "done": _np(tr.buf.done), "act": _np(tr.buf.act),
           "P": _np(tr.learner.P), "ep": _np(tr.env.episode_index()), "f64": _np(tr.env.get_state()[0])}
    if tr.obs_norm:
        out.update(stats=_np(tr.obs_stats), raw=_np(tr.obs_raw), mean=tr.obs_rms.mean.copy(), M2=tr.obs_rms.M2.copy())
    return out


def test_trainer_iterations_with_and_without_graphs():
    got = []
    for graphs in (True, False):
        tr = _trainer(graphs)
        assert tr.env.measures and tr.env.obs_noise() == dict(TSPEC, seed=11, env_offset=0)
        tr.iteration()
        tr.iteration()
        got.append(_rollout(tr))
    for k in got[0]:
        assert _bits_equal(got[0][k], got[1][k]), k
    plain = _trainer(True, obs_noise=None)
    plain.iteration()
    assert not plain.env.measures and not _bits_equal(_rollout(plain)["obs"][1], got[0]["obs"][1])


def _record(monkeypatch):
    """Per policy step of every eager trainer built from now on (a calibration's included): the raw row
    the step read, the frozen agent's action, and the env's truth and raw row after it."""
    from satrl.trainer import VecTrainer
    real, rec = VecTrainer._policy_step, []

    def policy_step(self, t, *a, **k):
        seen = (self.obs_raw if self.obs_norm else self.buf.obs[t]).clone()
        real(self, t, *a, **k)
        f, i = self.env.get_state()
        rec.append(dict(seen=_np(seen), other=_np(self.other_a), f64=_np(f), i32=_np(i),
                        ep=_np(self.env.episode_index()), raw=_np(self.obs_raw if self.obs_norm else self.buf.obs[t + 1])))

    monkeypatch.setattr(VecTrainer, "_policy_step", policy_step)
    return rec


def _recorded(monkeypatch, **kw):
    rec = _record(monkeypatch)
    return _trainer(False, **kw), rec


def _want_rows(x, seed=11):
    return R.row_of(R.measured(BOTH, HOLD, seed, np.arange(TN), x["ep"], x["i32"][1], x["f64"][0:12].T))


def test_buffer_rows_are_the_measured_rows(monkeypatch):
    tr, rec = _recorded(monkeypatch, obs_noise_seed=77)
    assert tr.env.obs_noise()["seed"] == 77
    f, i = tr.env.get_state()
    reset = dict(f64=_np(f), i32=_np(i), ep=_np(tr.env.episode_index()))
    assert _bits_equal(_np(tr.buf.obs[0]), _want_rows(reset, 77))          # the reset's row: (1, 0)
    tr.iteration()
    torch.cuda.synchronize()
    assert len(rec) == TT
    obs = _np(tr.buf.obs)
    for t, x in enumerate(rec):
        assert _bits_equal(x["raw"], _want_rows(x, 77)), t
        if t:                                              # ... and the row the next step's policies read
            assert _bits_equal(x["seen"], obs[t]), t
        if t + 1 < TT:                                     # (finish_iteration moves the last row to slot 0)
            assert _bits_equal(obs[t + 1], x["raw"]), t
    assert _bits_equal(obs[0], rec[-1]["raw"])
    assert (rec[-1]["ep"] == 2).all() and (rec[MAX_STEPS - 1]["i32"][1] == 0).all()


def test_obs_norm_statistics_are_those_of_the_measured_rows(monkeypatch):
    from satrl import norm
    real, fed = norm.obs_normalize, []

    def obs_normalize(raw, stats, clip, out, pivot=None, acc=None):
        if acc is not None:
            fed.append(_np(raw))                           # the rows the statistics accumulate
        return real(raw, stats, clip, out, pivot, acc)

    monkeypatch.setattr(norm, "obs_normalize", obs_normalize)
    tr, rec = _recorded(monkeypatch, obs_norm=True, obs_norm_calib_steps=4)
    assert len(rec) == 4 and len(fed) == 4 and tr.obs_rms.n == 4 * TN
    tr.iteration()
    torch.cuda.synchronize()
    assert len(rec) == 4 + TT and len(fed) == 4 + TT and tr.obs_rms.n == (4 + TT) * TN
    for t, (x, rows) in enumerate(zip(rec, fed)):
        assert _bits_equal(rows, x["raw"]) and _bits_equal(rows, _want_rows(x)), t
    plain = _trainer(False, obs_norm=True, obs_norm_calib_steps=4, obs_noise=None)
    assert not _bits_equal(_np(plain.obs_stats), _np(tr.obs_stats))


def test_a_scripted_opponent_acts_on_the_measured_row(monkeypatch):
    from satrl.scripted import intercept
    from test_scripted_cpu import restated
    law = intercept(10)
    tr, rec = _recorded(monkeypatch, scripted_opponent={"evader": law})
    tr.iteration()
    torch.cuda.synchronize()
    assert len(rec) == TT
    for t, x in enumerate(rec):
        want = restated(x["seen"], law.G, law.b, law.max_action)
        assert _bits_equal(x["other"], want.astype(np.float32)), t
        assert _bits_equal(x["raw"], _want_rows(x)), t
    # ... which is not what it would command on the truth
    truth = R.row_of(rec[0]["f64"][0:12].T)
    assert not _bits_equal(restated(truth, law.G, law.b, law.max_action).astype(np.float32), rec[1]["other"])


def _pooled(graphs, league, **kw):
    """A trainer whose frozen evader plays, per 32-env block, the live set, a stored one or (league) a law."""
    from satrl import scripted as S
    kw.update(opponent_pool=2, opponent_latest_prob=0.25, opponent_seed=4)
    if league:
        kw.update(league_laws={"evader": [S.evade(gain=0.5), S.constant([0.4, -0.3, 0.2])]}, league_law_prob=0.5)
    tr = _trainer(graphs, **kw)
    tr.pools["evader"].add(tr.evader.P * 1.25, {"agent": "evader", "iteration_count": -1, "episodes": 0.0})
    return tr


@pytest.mark.parametrize("league", [False, True])
def test_pool_and_league_launches_read_the_measured_row(monkeypatch, league):
    got = []
    for graphs in (True, False):
        tr = _pooled(graphs, league)
        tr.iteration()
        tr.iteration()
        got.append(_rollout(tr))
    for k in got[0]:
        assert _bits_equal(got[0][k], got[1][k]), (league, k)
    rec = _record(monkeypatch)
    tr = _pooled(False, league)
    tr.iteration()
    torch.cuda.synchronize()
    obs = _np(tr.buf.obs)
    for t, x in enumerate(rec):
        assert _bits_equal(x["raw"], _want_rows(x)), t
        if t:
            assert _bits_equal(x["seen"], obs[t]), t
    assert len(rec) == TT


def test_set_obs_noise_between_iterations_replays_the_captured_graphs():
    tr = _trainer(True, obs_noise=None)              # built without noise: the kernels without it
    tr.iteration()
    torch.cuda.synchronize()
    assert tr._graphs and not tr.env.measures and tr.env.obs_noise() is None
    tr.set_obs_noise(TSPEC)                          # the trainer's first noise: those graphs are dropped
    assert not tr._graphs and tr.env.measures and tr.env.obs_noise()["seed"] == 11
    tr.iteration()
    graphs = dict(tr._graphs)
    assert graphs
    tr.set_obs_noise({"pursuer": (50.0, 0.02), "hold": 10}, seed=12)     # a curriculum step: the same graphs
    exact = dict(zip(KEYS, R.EXACT))
    assert tr.env.obs_noise() == {"pursuer": dict(exact, pos=50.0, vel=0.02), "evader": exact, "hold": 10, "seed": 12,
                                  "env_offset": 0}
    tr.iteration()
    assert tr._graphs.keys() == graphs.keys() and all(tr._graphs[k] is g for k, g in graphs.items())
    tr.set_obs_noise(None)                           # off again: the same graphs
    tr.iteration()
    torch.cuda.synchronize()
    assert all(tr._graphs[k] is g for k, g in graphs.items()) and tr.env.obs_noise() is None
    from satrl.trainer import VecTrainer
    off = VecTrainer(_args(), flag=0, d_capture=D_CAPTURE, env_offset=320, use_graphs=False)
    assert off.env.obs_noise()["env_offset"] == 320  # data-parallel shards draw by global env id


def test_evaluate_between_iterations_changes_nothing():
    a, b = _trainer(), _trainer()
    a.iteration()
    a.evaluate()
    a.evaluate(obs_noise=(500.0, 1.0))
    a.iteration()
    b.iteration()
    b.iteration()
    x, y = _rollout(a), _rollout(b)
    for k in x:
        assert _bits_equal(x[k], y[k]), k


REC = ("ret", "final_dis", "min_dis", "dv_p", "dv_e", "length", "outcome")


def _streams(res):
    return {k: _np(v) for k, v in res.streams.items()}


def test_evaluate_under_obs_noise():
    tr, plain = _trainer(), _trainer(obs_noise=None)
    tr.iteration()
    plain.learner.P.copy_(tr.learner.P)
    plain.learner.sync_w2t()
    torch.cuda.synchronize()
    wide = {"pursuer": {"bias_pos": 1000.0, "pos": 200.0, "vel": 0.3}, "evader": (400.0, 0.2), "hold": 2}
    wide_craft = (R.craft_of(wide["pursuer"]), (0.0, 0.0, 400.0, 0.2))
    cases = [("inherit", BOTH, HOLD), (wide, wide_craft, 2)]
    gid = np.arange(TN)
    for arg, craft, hold in cases:
        a = tr.evaluate(deterministic="both", record=True, obs_noise=arg)
        b = tr.evaluate(deterministic="both", record=True, obs_noise=arg)
        sa, sb = _streams(a), _streams(b)
        assert a.steps == MAX_STEPS and all(_bits_equal(sa[k], sb[k]) for k in sa)
        for name in REC:
            assert _bits_equal(_np(getattr(a, name)), _np(getattr(b, name))), name
        for k in range(a.steps):                           # no autoreset here: episode 1, the device counter
            want = R.measured_rows(craft, hold, a.seed, gid, 1, k + 1, sa["obs64"][k])
            assert _bits_equal(sa["obs"][k], want), (arg, k)
            assert not _bits_equal(sa["obs"][k], sa["obs64"][k].astype(np.float32))
    none = tr.evaluate(deterministic="both", record=True, obs_noise=None)
    p = plain.evaluate(deterministic="both", record=True)
    sn, sp = _streams(none), _streams(p)
    assert all(_bits_equal(sn[k], sp[k]) for k in sn)
    assert _bits_equal(sn["obs"], sn["obs64"].astype(np.float32))
    for name in REC:
        assert _bits_equal(_np(getattr(none, name)), _np(getattr(p, name))), name
    assert tr.env.obs_noise() == dict(TSPEC, seed=11, env_offset=0)      # the trainer's own setting stays
    with pytest.raises(ValueError, match="obs_noise"):
        tr.evaluate(obs_noise="on")


def test_checkpoint_resumes_bitwise_under_obs_noise(tmp_path):
    path = str(tmp_path / "ck")
    spec = {"pursuer": SPEC["pursuer"], "evader": (60.0, 0.03), "hold": 2}
    first = _trainer(obs_noise=spec, obs_noise_seed=5)
    first.iteration()
    first.save_checkpoint(path)
    first.iteration()
    want = _rollout(first)
    for kw in (dict(obs_noise=spec, obs_noise_seed=5), dict(obs_noise=None)):
        B = _trainer(**kw)                                        # the checkpoint carries the spec and the seed
        B.load_checkpoint(path)
        assert B.env.obs_noise() == {"pursuer": SPEC["pursuer"], "evader": dict(zip(KEYS, (0.0, 0.0, 60.0, 0.03))),
                                     "hold": 2, "seed": 5, "env_offset": 0}
        B.iteration()
        got = _rollout(B)
        for k in want:
            assert _bits_equal(got[k], want[k]), (k, kw)
    off = _trainer(obs_noise=None)
    off.iteration()
    off.save_checkpoint(str(tmp_path / "off"))
    C = _trainer()                                                # a state without the entry means off
    C.load_checkpoint(str(tmp_path / "off"))
    assert C.env.obs_noise() is None
