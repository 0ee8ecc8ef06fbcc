"""Whole-state checkpoints of VecTrainer on the GPU: save after iteration k,
load into a fresh trainer, and iterations k+1... give the bits of the run
that never stopped.  Every comparison is np.array_equal / torch.equal.

Shapes: 64 and 96 envs (two and three 32-env blocks, more than one workgroup
of the wide step kernel), horizon 8 with max_episode_steps 5 (every env
times out, resets in-kernel and moves its episode index and running return
inside each iteration), minibatches of 64 rows, 2 epochs."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch

from conftest import PKG_DIR

pytestmark = pytest.mark.gpu

HALF = [2000.0] * 3 + [2.0] * 3 + [2000.0] * 3 + [2.0] * 3        # reset_spread half-widths
CASES = {
    "graphs-96": dict(num_envs=96),
    "eager-64": dict(num_envs=64, use_graphs=False),
    "flag1": dict(num_envs=64, flag=1),
    "h256": dict(num_envs=64, hidden_width=256),
    # every block plays the stored (half-scale) opponent, never the live one
    "pool": dict(num_envs=64, opponent_pool=2, opponent_snapshot_every=1, opponent_latest_prob=0.0, reset_spread=HALF,
                 stored_opponent=True),
    # an update stops after its first epoch (approx_kl > target_kl), so the minibatch
    # generator is saved in the state a shortened update leaves it in
    "everything": dict(num_envs=96, obs_norm=True, obs_norm_calib_steps=8, reward_scaling=True, reset_spread=HALF,
                       opponent_pool=2, opponent_snapshot_every=1, target_kl=1e-12, stored_opponent=True),
}


def _args(num_envs=64, max_episode_steps=5, **kw):
    sys.path.insert(0, PKG_DIR)
    from satrl.trainer import args_param
    base = dict(batch_size=num_envs * 8, mini_batch_size=64, hidden_width=64, K_epochs=2, num_envs=num_envs, horizon=8,
                max_episode_steps=max_episode_steps, seed=2, rollout_graph_chunk=4, update_graph_group=2,
                chkpt_dir="/tmp")
    return args_param(**dict(base, **kw))


def _trainer(case, **over):
    from satrl.trainer import VecTrainer
    kw = dict(CASES[case] if isinstance(case, str) else case, **over)
    flag, graphs = kw.pop("flag", 0), kw.pop("use_graphs", True)
    env_offset, stored = kw.pop("env_offset", 0), kw.pop("stored_opponent", False)
    tr = VecTrainer(_args(**kw), flag=flag, d_capture=15000.0, use_graphs=graphs, env_offset=env_offset)
    if stored:                      # the frozen agent's pool holds an opponent that differs from the live one
        frozen = tr.evader if tr.flag == 0 else tr.pursuer
        tr.pools[tr.frozen_agent].add(frozen.P * 0.5, {"agent": tr.frozen_agent, "iteration_count": 0, "episodes": 0.0})
    return tr


def _snap(tr):
    torch.cuda.synchronize()
    out = {"iteration_count": np.asarray(tr.iteration_count), "episodes": np.asarray(tr.episodes),
           "rollout_steps": np.asarray(tr.rollout_steps), "flag": np.asarray(tr.flag),
           "obs0": tr.buf.obs[0].cpu().numpy()}
    for name, L in (("pursuer", tr.pursuer), ("evader", tr.evader)):
        for k in ("P", "M", "V", "steps", "lr"):
            out[f"{name}.{k}"] = getattr(L, k).cpu().numpy()
    for k, v in tr.env.full_state().items():
        out["env." + k] = v
    return out


def _assert_same(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


_REF = {}


@pytest.fixture
def ref(tmp_path_factory):
    """case -> the uninterrupted run, once per case: 2 iterations, a
    checkpoint, 2 more; snapshots after iterations 2, 3 and 4."""
    def get(case):
        if case not in _REF:
            path = str(tmp_path_factory.mktemp("ck_" + case) / "ck")
            A = _trainer(case)
            first = A.train(max_iterations=2)
            assert A.save_checkpoint(path) == path
            r = dict(path=path, snap2=_snap(A), first=first, stats=[], snaps=[])
            for _ in range(2):
                r["stats"] += A.train(max_iterations=1)
                r["snaps"].append(_snap(A))
            r["norm"] = A.norm_state() if A.obs_norm else None
            r["pool"] = A.pool_state() if A.pools is not None else None
            r["diagnostics"] = list(A.diagnostics)
            assert A.env.check_errors() == 0
            _REF[case] = r
        return _REF[case]
    return get


@pytest.mark.parametrize("case", list(CASES))
def test_bitwise_resume(ref, case):
    r = ref(case)
    s2, s4 = r["snap2"], r["snaps"][1]
    # the run moved everything the checkpoint has to carry
    assert s2["iteration_count"] == 2 and s4["iteration_count"] == 4 and s4["episodes"] > s2["episodes"] > 0
    assert s2["env.ep_return"].any() and s2["env.episode_index"].min() >= 3 and s2["env.stats"][0] > 0
    learner = "evader" if CASES[case].get("flag") else "pursuer"
    assert s2[learner + ".steps"].min() > 0 and s2[learner + ".M"].any() and s2[learner + ".lr"][0] < 2e-4
    assert not np.array_equal(s2[learner + ".P"], s4[learner + ".P"])
    B = _trainer(case)
    meta = B.load_checkpoint(r["path"])
    assert meta["iteration_count"] == 2 and meta["shards"] == [[0, B.N]] and meta["world_size"] == 1
    _assert_same(_snap(B), s2, "loaded")
    stats = B.train(max_iterations=2)
    assert B.env.check_errors() == 0
    _assert_same(_snap(B), s4, "two iterations after the load")
    assert len(stats) == 2 and all(np.array_equal(a, b) for a, b in zip(stats, r["stats"]))
    if case == "everything":
        assert [d["epochs_run"] for d in r["diagnostics"]] == [1] * 4          # every update stopped early
        assert json.dumps(B.diagnostics) == json.dumps(r["diagnostics"])
        got, want = B.norm_state(), r["norm"]
        for part in ("obs", "ret"):
            for k in want[part]:
                assert np.array_equal(got[part][k], want[part][k]), (part, k)
        assert np.array_equal(got["carry"], want["carry"]) and want["carry"].any()
    if r["pool"] is not None:
        got = B.pool_state()
        for agent, want in r["pool"].items():
            assert torch.equal(got[agent]["storage"], want["storage"]), agent
            assert got[agent]["metas"] == want["metas"] and got[agent]["cursor"] == want["cursor"]
            assert got[agent]["added"] == want["added"] and got[agent]["seed"] == want["seed"]
        assert r["pool"]["pursuer"]["added"] == 4 and r["pool"]["evader"]["added"] == 1


@pytest.mark.parametrize("max_episode_steps", [5, 20])
def test_warm_up_after_a_load_keeps_the_episode_return(tmp_path, max_episode_steps):
    """The eager warm-up step before the first graph capture runs, in a
    resumed trainer, in the middle of a run: its reward must not stay in the
    running returns.  With 20-step episodes no env ends inside the next
    rollout, so the returns themselves would carry it; with 5-step episodes
    it would reach stats[1] through the episode that ends next."""
    case = dict(num_envs=64, max_episode_steps=max_episode_steps)
    A = _trainer(case)
    A.train(max_iterations=1)
    A.save_checkpoint(tmp_path / "ck")
    A.collect()
    B = _trainer(case)
    B.load_checkpoint(tmp_path / "ck")
    assert not B._graphs
    B.collect()
    assert B._graphs
    torch.cuda.synchronize()
    want = A.env.episode_return()
    assert want.ne(0).any() and torch.equal(B.env.episode_return(), want)
    assert torch.equal(B.env.stats, A.env.stats)
    assert torch.equal(B.buf.rew, A.buf.rew) and torch.equal(B.buf.obs, A.buf.obs)


def test_load_is_in_place_under_captured_graphs(ref):
    r = ref("pool")
    C = _trainer("pool")
    C.train(max_iterations=1)
    assert C._graphs and C.learner.stepper(64).graph is not None
    graphs = dict(C._graphs)
    tensors = {"P": C.pursuer.P, "M": C.pursuer.M, "V": C.pursuer.V, "eP": C.evader.P, "eM": C.evader.M,
               "eV": C.evader.V, "obs": C.buf.obs, "pool_p": C.pools["pursuer"].storage,
               "pool_e": C.pools["evader"].storage, "stats": C.env.stats, "steps": C.pursuer.steps,
               "lr": C.pursuer.lr, "W2T": C.pursuer.W2T, "member": C.member}
    ptrs = {k: t.data_ptr() for k, t in tensors.items()}
    w = C.pursuer.actor.fc1.weight
    C.load_checkpoint(r["path"])
    assert {k: t.data_ptr() for k, t in tensors.items()} == ptrs
    assert all(getattr(C.pursuer, k) is tensors[k] for k in ("P", "M", "V")) and C.buf.obs is tensors["obs"]
    assert C._graphs == graphs and C.pursuer.actor.fc1.weight is w
    _assert_same(_snap(C), r["snap2"], "loaded")
    assert np.array_equal(w.detach().cpu().numpy(), C.pursuer.flat_views(C.pursuer.P)["actor.fc1.weight"].cpu().numpy())
    stats = C.train(max_iterations=1)
    assert C._graphs == graphs
    _assert_same(_snap(C), r["snaps"][0], "one iteration after the load")
    assert np.array_equal(stats[0], r["stats"][0])


def _rollout(tr):
    tr.collect()
    torch.cuda.synchronize()
    b = tr.buf
    out = {k: getattr(b, k).cpu().numpy() for k in ("obs", "act", "logp", "rew", "done")}
    st = tr.env.full_state()
    return out, st


def test_resharded_load_without_a_process_group(tmp_path):
    """One trainer of 64 envs writes; two trainers of 32 envs (env_offset 0
    and 32) read their halves.  Their next rollouts and env states are the
    halves of the writer's, with randomised starts and an opponent pool on."""
    case = dict(CASES["pool"])
    A = _trainer(case)
    A.train(max_iterations=2)
    A.save_checkpoint(tmp_path / "ck")
    want, env_want = _rollout(A)
    assert want["done"].any() and (np.asarray(A.last_assignment) >= 0).all()     # the stored opponent plays
    stats0 = 0.0
    for r in range(2):
        B = _trainer(case, num_envs=32, env_offset=32 * r)
        with pytest.raises(ValueError, match="global_envs=64.*global_envs=32"):
            B.load_checkpoint(tmp_path / "ck")
        B.load_checkpoint(tmp_path / "ck", global_envs=64)
        assert B.iteration_count == 2 and B.episodes == A.episodes
        sl = slice(32 * r, 32 * r + 32)
        got, env_got = _rollout(B)
        for k in want:
            assert np.array_equal(got[k], want[k][:, sl]), (r, k)
        for k in ("f64", "i32"):
            assert np.array_equal(env_got[k], env_want[k][:, sl]), (r, k)
        for k in ("ep_return", "episode_index"):
            assert np.array_equal(env_got[k], env_want[k][sl]), (r, k)
        assert np.array_equal(B.last_assignment, A.last_assignment[r:r + 1])
        stats0 += env_got["stats"][0]
    assert stats0 == env_want["stats"][0]                         # the readers' episode counts sum to the writer's
    with pytest.raises(ValueError, match="split a 32-env block"):
        _trainer(dict(num_envs=48, opponent_pool=2, opponent_snapshot_every=1,
                      reset_spread=HALF)).load_checkpoint(tmp_path / "ck", global_envs=64)
    with pytest.raises(ValueError, match="outside"):
        _trainer(case, num_envs=64, env_offset=32).load_checkpoint(tmp_path / "ck", global_envs=64)


# -- data parallelism: two ranks on one device over gloo -------------------------------
def _dp_rank(rank, port, path, q):
    import datetime

    import torch.distributed as dist
    os.environ["SATRL_DP_TIMEOUT_S"] = "60"               # every wait on the peer is bounded
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2,
                            timeout=datetime.timedelta(seconds=120))
    try:
        sys.path.insert(0, PKG_DIR)
        from satrl.trainer import VecTrainer

        def trainer():
            return VecTrainer(_args(32), flag=0, d_capture=15000.0, pg=dist.group.WORLD, env_offset=32 * rank)

        A = trainer()
        assert A.sampler == "stratified" and A.mb_local == 32
        A.iteration()
        A.save_checkpoint(path)
        A.iteration()
        B = trainer()
        meta = B.load_checkpoint(path)
        assert B.iteration_count == 1 == meta["iteration_count"]
        B.iteration()
        torch.cuda.synchronize()
        out = {}
        for name, tr in (("A", A), ("B", B)):
            out[name] = {k: getattr(tr.learner, k).cpu().numpy() for k in ("P", "M", "V", "steps", "lr")}
            out[name].update(obs0=tr.buf.obs[0].cpu().numpy(), ep_return=tr.env.episode_return().cpu().numpy(),
                             stats=tr.env.stats.cpu().numpy(), episodes=np.asarray(tr.episodes))
        q.put((rank, out))
    except BaseException:
        import traceback
        q.put((rank, traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def test_world2_resume_on_one_device(tmp_path):
    """Two ranks x 32 envs with the stratified sampler: save at iteration 1,
    two fresh trainers load and run one iteration; P (and the rest of the
    learner and the per-rank env state) equals the uninterrupted run's on
    both ranks, and meta.json lists both shards."""
    import queue
    import time

    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    path = str(tmp_path / "ck")
    ps = [ctx.Process(target=_dp_rank, args=(r, port, path, q)) for r in range(2)]
    for p in ps:
        p.start()
    res, t_end = {}, time.monotonic() + 240
    while len(res) < 2 and time.monotonic() < t_end:
        try:
            r, v = q.get(timeout=2)
            assert not isinstance(v, str), f"rank {r}:\n{v}"
            res[r] = v
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in ps):
                break
    for p in ps:
        p.join(timeout=30)
        if p.exitcode is None:
            p.kill()
    assert len(res) == 2 and all(p.exitcode == 0 for p in ps), ([p.exitcode for p in ps], sorted(res))
    for r in range(2):
        for k, want in res[r]["A"].items():
            assert np.array_equal(res[r]["B"][k], want), (r, k)
        assert res[r]["A"]["steps"][0] == 2 * 2 * 8                      # 2 iterations x 2 epochs x 8 global minibatches
    assert np.array_equal(res[0]["B"]["P"], res[1]["B"]["P"])
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    assert meta["world_size"] == 2 and meta["global_envs"] == 64 and meta["shards"] == [[0, 32], [32, 32]]
    assert sorted(os.listdir(path)) == ["meta.json", "rank0.npz", "rank1.npz"]


def test_train_and_self_play_write_checkpoints(tmp_path):
    from satrl import checkpoint as ck
    case = dict(num_envs=64, use_graphs=False, opponent_pool=2)
    A = _trainer(case)
    p = str(tmp_path / "run")
    out = A.train(max_iterations=3, checkpoint_every=2, checkpoint_path=p)      # written after 2 and after the last
    assert len(out) == 3 and ck.read_meta(p)["iteration_count"] == 3 and A.iteration_count == 3
    assert sorted(os.listdir(tmp_path)) == ["run"]
    B = _trainer(case)
    B.load_checkpoint(p)
    _assert_same(_snap(B), _snap(A))
    # a state exists between iterations only
    A.collect()
    with pytest.raises(RuntimeError, match="between iterations"):
        A.state_dict()
    with pytest.raises(RuntimeError, match="between iterations"):
        A.save_checkpoint(p)
    A.compute_advantages()
    A.update()
    A.finish_iteration()
    assert A.state_dict()["iteration_count"] == 4 and ck.read_meta(p)["iteration_count"] == 3
    # self_play: the Flag and the stored learners of the phase that just ended are in the checkpoint
    A.self_play(2, 1, checkpoint_every=1, checkpoint_path=p)
    meta = ck.read_meta(p)
    assert meta["iteration_count"] == 6 and meta["flag"] == 1 and A.pools["evader"].added == 1
    B.load_checkpoint(p)
    assert B.flag == 1 and B.learner is B.evader
    _assert_same(_snap(B), _snap(A))
    assert B.pool_state()["evader"]["added"] == 1 and B.pool_state()["pursuer"]["added"] == 1
    assert torch.equal(B.pools["evader"].storage, A.pools["evader"].storage)
