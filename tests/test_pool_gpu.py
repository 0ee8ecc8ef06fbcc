"""Opponent pool on the GPU: satrl_policy_act_pool (the pooled policy kernel)
against plain satrl_policy_act launches, under graph replay, and through
VecTrainer (collect, sharding, self_play, evaluate).  Every comparison is
bitwise: a pooled block's rows are the plain kernel's for that block's
parameter set, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INT32_MIN = -2 ** 31


def _args(**kw):
    from satrl.trainer import args_param
    kw.setdefault("hidden_width", 64)
    kw.setdefault("num_envs", 96)
    kw.setdefault("horizon", 16)
    kw.setdefault("batch_size", kw["num_envs"] * kw["horizon"])
    kw.setdefault("mini_batch_size", 128)
    kw.setdefault("K_epochs", 1)
    kw.setdefault("rollout_graph_chunk", 8)
    kw.setdefault("max_episode_steps", 10)
    kw.setdefault("seed", 3)
    a = args_param(chkpt_dir="/tmp", **kw)
    a.state_dim, a.action_dim, a.max_action = 18, 3, 1.6
    return a


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _perturbations(total, n, seed=17):
    """n fixed host perturbations of a flat parameter buffer."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(total, generator=g) * 0.05 for _ in range(n)]


def _block_rows(b, N):
    return slice(32 * b, min(32 * (b + 1), N))


# ---------------------------------------------------------------------------
# 1. the kernel against K plain launches
# ---------------------------------------------------------------------------
def _kernel_setup(H):
    from satrl.ppo import PPOLearner, ppo_layout
    torch.manual_seed(5)
    args = _args(hidden_width=H)
    live = [PPOLearner(args, "pursuer", use_graph=False).P.clone(), PPOLearner(args, "evader", use_graph=False).P.clone()]
    total = ppo_layout(H)["total"]
    assert live[0].numel() == total
    return live, total


def _pool_of(live_P, total, K, stride):
    """K parameter sets that differ from the live one and from each other in
    every element, in a [K, stride] pool whose padding is NaN."""
    pool = torch.full((K, stride), NAN, device=DEV)
    for k, d in enumerate(_perturbations(total, K, seed=100 + K)):
        pool[k, :total] = live_P + d.to(DEV) * (k + 1)
    return pool


def _plain(H, obs, P0, P1, seed, env_offset, step, sb):
    from satrl.ppo import policy_act
    N = obs.shape[0]
    out = [torch.full((N, 3), NAN, device=DEV) for _ in range(4)]
    policy_act(H, obs, P0, P1, 1.6, seed, env_offset, step, *out, step_base=sb)
    return out


def _check_pooled(H, N, member_list, live, pool, K, tag):
    from satrl.ppo import policy_act_pool
    g = torch.Generator(device=DEV).manual_seed(1000 + N)
    obs = torch.randn((N, 18), device=DEV, generator=g)
    sb = torch.tensor([11], dtype=torch.int64, device=DEV)
    seed, env_offset, step = 123, 64, 5
    nb = (N + 31) // 32
    assert len(member_list) == nb
    member = torch.tensor(member_list, dtype=torch.int32, device=DEV)
    G = 64                                                   # guard rows behind every output
    for agent in (1, 0):
        # the plain launches: one per parameter set the pooled agent can act with
        ref = {}
        for c in set(m if 0 <= m < K else -1 for m in member_list) | {-1}:
            Pc = live[agent] if c < 0 else pool[c]
            P0, P1 = (Pc, live[1]) if agent == 0 else (live[0], Pc)
            ref[c] = _plain(H, obs, P0, P1, seed, env_offset, step, sb)
        keep = [t.clone() for t in (obs, live[0], live[1], pool, member)]
        big = [torch.full((N + G, 3), NAN, device=DEV) for _ in range(4)]
        out = [b[:N] for b in big]
        policy_act_pool(H, obs, live[0], live[1], 1.6, seed, env_offset, step, *out, agent, pool, member, step_base=sb)
        torch.cuda.synchronize()
        pooled, other = (out[2:], out[:2]) if agent == 1 else (out[:2], out[2:])
        for b, m in enumerate(member_list):
            c = m if 0 <= m < K else -1                      # outside [0, K): the live parameters
            rows = _block_rows(b, N)
            want = ref[c][2:] if agent == 1 else ref[c][:2]
            for name, x, y in zip(("act", "logp"), pooled, want):
                assert not bool(torch.isnan(x[rows]).any()), (tag, agent, b, name)
                assert _same(x[rows], y[rows]), (tag, agent, b, m, name)
        want = ref[-1][:2] if agent == 1 else ref[-1][2:]
        for name, x, y in zip(("act", "logp"), other, want):
            assert _same(x, y), (tag, agent, "other agent", name)
        for k, b in enumerate(big):
            assert bool(torch.isnan(b[N:]).all()), (tag, agent, "guard", k)
        for name, x, y in zip(("obs", "P0", "P1", "pool", "member"), (obs, live[0], live[1], pool, member), keep):
            assert _same(x, y), (tag, agent, name)
        # the stored sets do change the pooled agent's rows (the comparison above is not vacuous)
        if any(0 <= m < K for m in member_list):
            b = next(b for b, m in enumerate(member_list) if 0 <= m < K)
            live_rows = (ref[-1][2] if agent == 1 else ref[-1][0])[_block_rows(b, N)]
            assert not _same(pooled[0][_block_rows(b, N)], live_rows), (tag, agent)


@pytest.mark.parametrize("H", [64, 128, 256])
def test_pooled_kernel_equals_plain_launches_per_block(H):
    """N = 167: five full blocks and a 7-row one, K = 3 sets at a padded
    stride, members 3 and INT32_MIN outside [0, K); then N = 7, one ragged
    block.  env_offset 64, step 5 and a step_base word of 11."""
    from satrl.pool import pool_stride
    live, total = _kernel_setup(H)
    K = 3
    stride = pool_stride(H) + 64                             # more padding than the pool's own rounding
    pool = _pool_of(live[1], total, K, stride)
    _check_pooled(H, 167, [0, 2, -1, 1, 3, INT32_MIN], live, pool, K, f"H {H} N 167")
    _check_pooled(H, 7, [2], live, pool, K, f"H {H} N 7 stored")
    _check_pooled(H, 7, [K], live, pool, K, f"H {H} N 7 live")


def test_pooled_launch_rejects_what_the_header_says():
    from satrl._lib import NativeError
    from satrl.ppo import policy_act_pool
    live, total = _kernel_setup(64)
    N = 40
    obs = torch.zeros((N, 18), device=DEV)
    out = [torch.full((N, 3), NAN, device=DEV) for _ in range(4)]
    member = torch.zeros(2, dtype=torch.int32, device=DEV)
    short = torch.zeros((2, total - 4), device=DEV)
    with pytest.raises(NativeError, match="satrl_policy_act_pool"):
        policy_act_pool(64, obs, live[0], live[1], 1.6, 0, 0, 0, *out, 1, short, member)
    good = torch.zeros((2, total), device=DEV)
    with pytest.raises(NativeError):
        policy_act_pool(64, obs, live[0], live[1], 1.6, 0, 0, 0, *out, 2, good, member)
    with pytest.raises(NativeError):                         # one entry per 32-row block
        policy_act_pool(64, obs, live[0], live[1], 1.6, 0, 0, 0, *out, 1, good, member[:1])
    assert all(bool(torch.isnan(t).all()) for t in out)


# ---------------------------------------------------------------------------
# 2. graph replay follows in-place changes of member and pool
# ---------------------------------------------------------------------------
def test_captured_pooled_launch_follows_member_and_pool():
    from satrl.pool import pool_stride
    from satrl.ppo import policy_act_pool
    H, N, K = 64, 64, 3
    live, total = _kernel_setup(H)
    pool = _pool_of(live[1], total, K, pool_stride(H))
    obs = torch.randn((N, 18), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    sb = torch.tensor([3], dtype=torch.int64, device=DEV)
    member = torch.tensor([1, -1], dtype=torch.int32, device=DEV)
    out = [torch.full((N, 3), NAN, device=DEV) for _ in range(4)]

    def launch():
        policy_act_pool(H, obs, live[0], live[1], 1.6, 9, 0, 2, *out, 1, pool, member, step_base=sb)

    def expect(members):
        for b, m in enumerate(members):
            ref = _plain(H, obs, live[0], live[1] if m < 0 else pool[m], 9, 0, 2, sb)
            rows = _block_rows(b, N)
            for x, y in zip(out, ref):
                assert _same(x[rows], y[rows]), (members, b)

    launch()                                                 # eager once before the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    for t in out:
        t.fill_(NAN)
    g.replay()
    torch.cuda.synchronize()
    expect([1, -1])
    member.copy_(torch.tensor([2, 0], dtype=torch.int32))    # in place, no recapture
    pool[0, :total].copy_(live[0])                           # slot 0 <- another parameter set, in place
    for t in out:
        t.fill_(NAN)
    g.replay()
    torch.cuda.synchronize()
    expect([2, 0])


# ---------------------------------------------------------------------------
# 3. / 4. the trainer's rollout
# ---------------------------------------------------------------------------
def _trainer(use_graphs=True, env_offset=0, **kw):
    from satrl.trainer import VecTrainer
    return VecTrainer(_args(**kw), flag=0, d_capture=15000.0, env_offset=env_offset, use_graphs=use_graphs)


def _fill_evader_pool(tr, n):
    """n perturbed evader parameter sets into tr's evader pool (the same sets for every trainer of a seed)."""
    P = tr.evader.P
    for j, d in enumerate(_perturbations(P.numel(), n)):
        tr.pools["evader"].add(P + d.to(DEV), {"agent": "evader", "iteration_count": -1 - j, "episodes": 0.0})


@pytest.mark.parametrize("use_graphs", [True, False])
def test_trainer_with_an_empty_pool_collects_what_it_collects_without(use_graphs):
    a = _trainer(use_graphs, opponent_pool=4)
    b = _trainer(use_graphs)
    assert a.pools is not None and b.pools is None and b.member is None
    assert a.pools["pursuer"].filled == 0 and a.pools["evader"].filled == 0
    assert tuple(a.member.shape) == (3,) and a.member.dtype == torch.int32
    a.collect()
    b.collect()
    torch.cuda.synchronize()
    assert (a.last_assignment == -1).all()
    for name in ("obs", "act", "logp", "rew", "done"):
        x, y = getattr(a.buf, name), getattr(b.buf, name)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    assert _same(a.other_a, b.other_a)


def test_trainer_with_a_filled_pool_plays_the_assigned_slots():
    from satrl.pool import opponent_assign
    from satrl.ppo import policy_act
    tr = _trainer(True, opponent_pool=4, opponent_latest_prob=0.0, opponent_seed=1)
    _fill_evader_pool(tr, 3)
    N, T, H = tr.N, tr.T, tr.pursuer.H
    pool = tr.pools["evader"]
    ptr0 = (tr.member.data_ptr(), pool.storage.data_ptr())
    seen = []
    for it in range(2):
        base = tr.rollout_steps
        tr.collect()
        torch.cuda.synchronize()
        want = opponent_assign(1, tr.iteration_count, 0, 3, 3, 0.0)
        assert tr.iteration_count == it and np.array_equal(tr.last_assignment, want), it
        assert np.array_equal(tr.member.cpu().numpy(), want) and (want >= 0).all(), it
        sb = torch.tensor([base], dtype=torch.int64, device=DEV)
        for b, m in enumerate(want.tolist()):
            ref = _plain(H, tr.buf.obs[T - 1], tr.pursuer.P, pool.slot(m), tr.seed, tr.env_offset, T - 1, sb)
            rows = _block_rows(b, N)
            assert _same(tr.other_a[rows], ref[2][rows]), (it, b, m)
            assert _same(tr.buf.act[T - 1][rows], ref[0][rows]), (it, b)      # the learner: its live parameters
            live = _plain(H, tr.buf.obs[T - 1], tr.pursuer.P, tr.evader.P, tr.seed, tr.env_offset, T - 1, sb)
            assert not _same(tr.other_a[rows], live[2][rows]), (it, b)        # ... and not the live opponent
        seen.append((len(tr._graphs), want.copy()))
        tr.finish_iteration()
    assert seen[0][0] == seen[1][0] == (T + tr.chunk - 1) // tr.chunk           # replayed, not recaptured
    assert not np.array_equal(seen[0][1], seen[1][1])                           # under a new assignment
    assert ptr0 == (tr.member.data_ptr(), pool.storage.data_ptr())


def test_trainer_refuses_env_offsets_inside_a_block():
    with pytest.raises(ValueError, match="opponent_pool"):
        _trainer(True, env_offset=16, opponent_pool=2)


# ---------------------------------------------------------------------------
# 5. sharding
# ---------------------------------------------------------------------------
def test_pooled_rollout_is_sharding_invariant():
    kw = dict(opponent_pool=4, opponent_latest_prob=0.5, opponent_seed=1)
    whole = _trainer(True, num_envs=128, **kw)
    parts = [_trainer(True, num_envs=64, env_offset=o, **kw) for o in (0, 64)]
    for tr in [whole] + parts:
        _fill_evader_pool(tr, 3)
        tr.collect()
    torch.cuda.synchronize()
    a = whole.last_assignment
    assert (a == -1).any() and (a >= 0).any()                # live and stored opponents in this rollout
    for k, tr in enumerate(parts):
        assert np.array_equal(tr.last_assignment, a[2 * k:2 * k + 2]), k
        cols = slice(64 * k, 64 * (k + 1))
        for name in ("act", "obs", "rew"):
            x, y = getattr(tr.buf, name), getattr(whole.buf, name)[:, cols]
            assert torch.equal(_bits(x), _bits(y)), (k, name)


# ---------------------------------------------------------------------------
# 6. self_play stores the learner at every phase end
# ---------------------------------------------------------------------------
def test_self_play_snapshots_and_pool_state_round_trip():
    tr = _trainer(True, opponent_pool=4)
    assert tr.flag == 0
    saved = []
    snap = tr.snapshot_opponent

    def recording(agent=None):
        name = "pursuer" if tr.learner is tr.pursuer else "evader"
        saved.append((name, tr.learner.P.clone(), tr.iteration_count, tr.episodes))
        return snap(agent)

    tr.snapshot_opponent = recording
    out = tr.self_play(phases=3, iterations_per_phase=1)
    torch.cuda.synchronize()
    assert [f for f, _ in out] == [0, 1, 0]
    assert [s[0] for s in saved] == ["pursuer", "evader", "pursuer"]
    assert tr.pools["pursuer"].filled == 2 and tr.pools["evader"].filled == 1
    slots = {"pursuer": 0, "evader": 0}
    for name, P, it, eps in saved:
        k = slots[name]
        slots[name] += 1
        assert _same(tr.pools[name].slot(k), P), (name, k)
        assert tr.pools[name].metas[k] == {"agent": name, "iteration_count": it, "episodes": eps}
    assert [s[2] for s in saved] == [1, 2, 3]
    assert not _same(saved[0][1], saved[2][1])               # the pursuer learned in between
    st = tr.pool_state()
    assert all(not d["storage"].is_cuda for d in st.values())
    fresh = _trainer(True, opponent_pool=4)
    fresh.load_pool_state(st)
    for name in ("pursuer", "evader"):
        p, q = tr.pools[name], fresh.pools[name]
        assert q.filled == p.filled and q.cursor == p.cursor and q.metas == p.metas
        assert _same(q.storage, p.storage)
    with pytest.raises(ValueError):
        _trainer(True).pool_state()


def test_snapshot_every_iteration():
    tr = _trainer(True, opponent_pool=2, opponent_snapshot_every=2)
    for _ in range(4):
        tr.iteration()
    assert tr.pools["pursuer"].filled == 2 and tr.pools["evader"].filled == 0
    assert [m["iteration_count"] for m in tr.pools["pursuer"].metas] == [2, 4]
    assert _same(tr.pools["pursuer"].slot(1), tr.pursuer.P)


# ---------------------------------------------------------------------------
# 7. evaluate(opponent=k)
# ---------------------------------------------------------------------------
def test_evaluate_against_a_stored_opponent():
    tr = _trainer(True, opponent_pool=4)
    _fill_evader_pool(tr, 2)
    plain = _trainer(True)
    before = (tr.pursuer.P.clone(), tr.evader.P.clone(), [t.clone() for t in tr.env.get_state()],
              tr.step_base.clone(), tr.buf.obs[0].clone())
    res = {k: tr.evaluate(opponent=k) for k in (0, 1)}
    live = tr.evaluate()
    for k in (0, 1):
        plain.evader.P.copy_(tr.pools["evader"].slot(k))
        want = plain.evaluate()
        for name in ("ret", "length", "outcome"):
            x, y = getattr(res[k], name), getattr(want, name)
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (k, name)
        assert res[k].steps == want.steps
    assert not torch.equal(res[0].ret, res[1].ret) and not torch.equal(res[0].ret, live.ret)
    with pytest.raises(IndexError):
        tr.evaluate(opponent=2)                              # not filled
    with pytest.raises(IndexError):
        tr.evaluate(opponent=4)
    with pytest.raises(ValueError):
        plain.evaluate(opponent=0)                           # no pool
    with pytest.raises(ValueError):
        plain.evaluate_pool()
    table = tr.evaluate_pool()
    assert [m["iteration_count"] for m, _ in table] == [-1, -2]
    assert [repr(s) for _, s in table] == [repr(res[0].summary()), repr(res[1].summary())]
    after = (tr.pursuer.P, tr.evader.P, tr.env.get_state(), tr.step_base, tr.buf.obs[0])
    assert _same(before[0], after[0]) and _same(before[1], after[1])
    for x, y in zip(before[2], after[2]):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.equal(before[3], after[3]) and _same(before[4], after[4])
