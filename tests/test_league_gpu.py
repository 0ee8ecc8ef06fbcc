"""League play on the GPU: satrl_policy_act_league against plain
satrl_policy_act / satrl_scripted_act launches per block, under graph replay,
satrl_league_tally against a NumPy count, and VecTrainer (assignment, counts,
sharding, PFSP, checkpoints, evaluate_pool).  Every comparison is bitwise or
an exact integer count: there is no tolerance anywhere in this file."""
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
    kw.setdefault("num_envs", 128)
    kw.setdefault("horizon", 8)
    kw.setdefault("batch_size", kw["num_envs"] * kw["horizon"])
    kw.setdefault("mini_batch_size", 64)
    kw.setdefault("K_epochs", 1)
    kw.setdefault("rollout_graph_chunk", 4)
    kw.setdefault("update_graph_group", 2)
    kw.setdefault("max_episode_steps", 5)        # every env times out and resets inside each rollout
    kw.setdefault("seed", 3)
    a = args_param(chkpt_dir="/tmp", **kw)
    a.state_dim, a.action_dim, a.max_action = 18, 3, 1.6
    return a


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _perturbations(total, n, seed=17):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(total, generator=g) * 0.05 for _ in range(n)]


def _block_rows(b, N):
    return slice(32 * b, min(32 * (b + 1), N))


def _is_pos_zero(t):
    return bool((_bits(t) == 0).all())


# ---------------------------------------------------------------------------
# 1. the kernel against plain launches and the stand-alone law kernel
# ---------------------------------------------------------------------------
def _kernel_setup(H):
    from satrl.ppo import PPOLearner, ppo_layout
    torch.manual_seed(5)
    args = _args(hidden_width=H)
    live = [PPOLearner(args, "pursuer", use_graph=False).P.clone(), PPOLearner(args, "evader", use_graph=False).P.clone()]
    total = ppo_layout(H)["total"]
    return live, total


def _pool_of(live_P, total, K, stride):
    pool = torch.full((K, stride), NAN, device=DEV)
    for k, d in enumerate(_perturbations(total, K, seed=100 + K)):
        pool[k, :total] = live_P + d.to(DEV) * (k + 1)
    return pool


def _law_rows(J, rows=None):
    """A law table of J laws, intercept() first and random finite G after it;
    rows past J (to `rows`) are NaN: the kernel must never read them."""
    from satrl import scripted as S
    rng = np.random.default_rng(7)
    laws = [S.intercept()] + [S.ScriptedLaw(rng.normal(size=(3, 18)) * 1e-3, rng.normal(size=3) * 0.1, 1.0 + 0.25 * j)
                              for j in range(1, J)]
    tab = torch.full((rows or J, S.LAW_DOUBLES), NAN, dtype=torch.float64, device=DEV)
    for j, law in enumerate(laws):
        tab[j] = torch.from_numpy(law.packed()).to(DEV)
    return tab


def _plain(H, obs, P0, P1, seed, env_offset, step, sb):
    from satrl.ppo import policy_act
    N = obs.shape[0]
    out = [torch.full((N, 3), NAN, device=DEV) for _ in range(4)]
    policy_act(H, obs, P0, P1, 1.6, seed, env_offset, step, *out, step_base=sb)
    return out


def _check_league(H, N, member_list, live, pool, K, laws, J, tag):
    from satrl.ppo import policy_act_league
    from satrl.scripted import scripted_act
    g = torch.Generator(device=DEV).manual_seed(1000 + N)
    obs = torch.randn((N, 18), device=DEV, generator=g)
    obs_law = torch.randn((N, 18), device=DEV, generator=g) * 1000.0      # the raw row: not obs
    sb = torch.tensor([11], dtype=torch.int64, device=DEV)
    seed, env_offset, step = 123, 64, 5
    assert len(member_list) == (N + 31) // 32
    member = torch.tensor(member_list, dtype=torch.int32, device=DEV)
    law_ref = [scripted_act(obs_law, laws[j]) for j in range(J)]
    G = 64                                                   # guard rows behind every output

    def code(m):                                             # the parameter set of a non-law block
        return m if 0 <= m < K else -1

    for agent in (1, 0):
        ref = {}
        for c in {code(m) for m in member_list} | {-1}:
            Pc = live[agent] if c < 0 else pool[c]
            P0, P1 = (Pc, live[1]) if agent == 0 else (live[0], Pc)
            ref[c] = _plain(H, obs, P0, P1, seed, env_offset, step, sb)
        keep = [t.clone() for t in (obs, obs_law, live[0], live[1], pool, member, laws)]
        big = [torch.full((N + G, 3), NAN, device=DEV) for _ in range(4)]
        out = [b[:N] for b in big]
        policy_act_league(H, obs, obs_law, live[0], live[1], 1.6, seed, env_offset, step, *out, agent, pool, member,
                          laws, J, step_base=sb)
        torch.cuda.synchronize()
        mine, other = (out[2:], out[:2]) if agent == 1 else (out[:2], out[2:])
        for b, m in enumerate(member_list):
            rows = _block_rows(b, N)
            if K <= m < K + J:                               # a law block: the law on obs_law, +0.0 log-probs
                assert _same(mine[0][rows], law_ref[m - K][rows]), (tag, agent, b, m, "law act")
                assert _is_pos_zero(mine[1][rows]), (tag, agent, b, m, "law logp")
                continue
            want = ref[code(m)][2:] if agent == 1 else ref[code(m)][:2]
            for name, x, y in zip(("act", "logp"), mine, want):
                assert not bool(torch.isnan(x[rows]).any()), (tag, agent, b, name)
                assert _same(x[rows], y[rows]), (tag, agent, b, m, name)
        want = ref[-1][:2] if agent == 1 else ref[-1][2:]
        for name, x, y in zip(("act", "logp"), other, want):
            assert _same(x, y), (tag, agent, "other agent", name)
        for k, b in enumerate(big):
            assert bool(torch.isnan(b[N:]).all()), (tag, agent, "guard", k)
        for name, x, y in zip(("obs", "obs_law", "P0", "P1", "pool", "member"), (obs, obs_law, live[0], live[1], pool,
                                                                                 member), keep):
            assert _same(x, y), (tag, agent, name)
        assert torch.equal(laws.view(torch.int64), keep[6].view(torch.int64)), (tag, agent, "laws")
    # the two laws differ from each other and from every network's rows: the comparison is not vacuous
    if J > 1:
        assert not _same(law_ref[0], law_ref[1])


@pytest.mark.parametrize("H", [64, 128, 256])
def test_league_kernel_equals_plain_and_scripted_launches_per_block(H):
    """N = 167 (five full blocks and a 7-row one), K = 3 sets at a padded
    stride, J = 2 laws in a table whose further rows are NaN, obs_law != obs;
    members live, stored, both laws and K + J / INT32_MIN outside every range;
    then N = 7, one ragged block, as a law."""
    from satrl.pool import pool_stride
    live, total = _kernel_setup(H)
    K, J = 3, 2
    pool = _pool_of(live[1], total, K, pool_stride(H) + 64)
    laws = _law_rows(J, rows=4)
    _check_league(H, 167, [-1, 0, 2, K, K + 1, K + J], live, pool, K, laws, J, f"H {H} N 167")
    _check_league(H, 167, [-1, 0, 2, K, K + 1, INT32_MIN], live, pool, K, laws, J, f"H {H} N 167 INT32_MIN")
    _check_league(H, 7, [K + 1], live, pool, K, laws, J, f"H {H} N 7 law")


@pytest.mark.parametrize("H", [64, 128, 256])
def test_league_kernel_without_law_members_is_the_pooled_kernel(H):
    from satrl.pool import pool_stride
    from satrl.ppo import policy_act_league, policy_act_pool
    live, total = _kernel_setup(H)
    K, J, N = 3, 2, 167
    pool = _pool_of(live[1], total, K, pool_stride(H))
    laws = _law_rows(J)
    g = torch.Generator(device=DEV).manual_seed(2)
    obs = torch.randn((N, 18), device=DEV, generator=g)
    obs_law = torch.randn((N, 18), device=DEV, generator=g)
    member = torch.tensor([0, -1, 2, 1, -1, 0], dtype=torch.int32, device=DEV)
    sb = torch.tensor([4], dtype=torch.int64, device=DEV)
    for agent in (0, 1):
        a = [torch.full((N, 3), NAN, device=DEV) for _ in range(4)]
        b = [torch.full((N, 3), NAN, device=DEV) for _ in range(4)]
        policy_act_league(H, obs, obs_law, live[0], live[1], 1.6, 77, 32, 3, *a, agent, pool, member, laws, J,
                          step_base=sb)
        policy_act_pool(H, obs, live[0], live[1], 1.6, 77, 32, 3, *b, agent, pool, member, step_base=sb)
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(a, b)):
            assert _same(x, y) and not bool(torch.isnan(x).any()), (H, agent, k)


def test_league_launch_rejects_what_the_header_says():
    """Every refusal include/satrl_ppo.h lists for satrl_policy_act_league, on
    live device buffers: through the Python wrapper where it can form the
    call, and through the C entry point itself for the cases the wrapper's own
    shape checks would stop first (NULL and misaligned pointers, K <= 0).
    Nothing is launched: the outputs keep their NaN."""
    import satrl._lib as L
    from satrl._lib import NativeError
    from satrl.ppo import policy_act_league
    live, total = _kernel_setup(64)
    N = 40
    obs = torch.zeros((N, 18), device=DEV)
    out = [torch.full((N, 3), NAN, device=DEV) for _ in range(4)]
    member = torch.zeros(2, dtype=torch.int32, device=DEV)
    good = torch.zeros((2, total), device=DEV)
    laws = _law_rows(2, rows=9)

    def call(pool=good, agent=1, member=member, laws=laws, J=2, obs_law=obs):
        policy_act_league(64, obs, obs_law, live[0], live[1], 1.6, 0, 0, 0, *out, agent, pool, member, laws, J)

    with pytest.raises(NativeError, match="satrl_policy_act_league: pool_stride"):
        call(pool=torch.zeros((2, total - 4), device=DEV))
    with pytest.raises(NativeError, match="satrl_policy_act_league: pool_agent"):
        call(agent=2)
    with pytest.raises(NativeError, match="satrl_policy_act_league: J"):
        call(J=0)
    with pytest.raises(NativeError, match="satrl_policy_act_league: J"):
        call(J=9)
    with pytest.raises(ValueError):                          # more laws than the table has rows
        call(laws=laws[:2], J=3)
    with pytest.raises(NativeError):                         # one member per 32-row block
        call(member=member[:1])
    with pytest.raises(NativeError):
        call(obs_law=obs[:8])
    with pytest.raises(NativeError):
        call(laws=laws.float())
    # the C entry point itself
    from satrl.pool import pool_stride
    lib, vp = L.lib(), L.C.c_void_p
    wide = torch.zeros((2, pool_stride(64)), device=DEV)
    base = dict(H=64, N=N, obs=obs.data_ptr(), P0=live[0].data_ptr(), P1=live[1].data_ptr(), act0=out[0].data_ptr(),
                logp0=out[1].data_ptr(), act1=out[2].data_ptr(), logp1=out[3].data_ptr(), agent=1,
                pool=wide.data_ptr(), stride=wide.shape[1], K=2, member=member.data_ptr(), obs_law=obs.data_ptr(),
                laws=laws.data_ptr(), J=2)
    assert wide.data_ptr() % 16 == 0 and laws.data_ptr() % 8 == 0 and wide.shape[1] % 4 == 0

    def raw(**kw):
        a = dict(base, **kw)
        p = {k: (None if a[k] is None else vp(a[k])) for k in ("obs", "P0", "P1", "act0", "logp0", "act1", "logp1",
                                                               "pool", "member", "obs_law", "laws")}
        assert lib.satrl_gae(0, 0, None, None, None, 0.0, 0.0, None, None, None) == -1      # another call's text first
        rc = lib.satrl_policy_act_league(a["H"], a["N"], p["obs"], p["P0"], p["P1"], 1.6, 0, 0, 0, None, p["act0"],
                                         p["logp0"], p["act1"], p["logp1"], a["agent"], p["pool"], a["stride"],
                                         a["K"], p["member"], p["obs_law"], p["laws"], a["J"], L.stream_ptr())
        return rc, lib.satrl_ppo_last_error()

    for word, kw in ((b"H", dict(H=100)), (b"N", dict(N=0)), (b"obs is NULL", dict(obs=None)),
                     (b"P0 is NULL", dict(P0=None)), (b"act0 is NULL", dict(act0=None)),
                     (b"logp0 is NULL", dict(logp0=None)), (b"P1", dict(P1=None)), (b"act1", dict(act1=None)),
                     (b"logp1", dict(logp1=None)), (b"pool_agent", dict(agent=-1)), (b"pool_agent", dict(agent=2)),
                     (b"pool is NULL", dict(pool=None)), (b"member is NULL", dict(member=None)),
                     (b"K", dict(K=0)), (b"K", dict(K=-1)), (b"pool_stride", dict(stride=total - 1)),
                     (b"pool_stride", dict(stride=wide.shape[1] + 2)), (b"16-byte", dict(pool=wide.data_ptr() + 4)),
                     (b"obs_law is NULL", dict(obs_law=None)), (b"laws is NULL", dict(laws=None)),
                     (b"J", dict(J=0)), (b"J", dict(J=9)), (b"8-byte", dict(laws=laws.data_ptr() + 4))):
        rc, msg = raw(**kw)
        assert rc == -1 and msg.startswith(b"satrl_policy_act_league: ") and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in out)


# ---------------------------------------------------------------------------
# 2. graph replay follows in-place changes of member, pool and a law
# ---------------------------------------------------------------------------
def test_captured_league_launch_follows_member_pool_and_law():
    from satrl import scripted as S
    from satrl.pool import pool_stride
    from satrl.ppo import policy_act_league
    H, N, K = 64, 64, 3
    live, total = _kernel_setup(H)
    pool = _pool_of(live[1], total, K, pool_stride(H))
    tab = S.LawTable(DEV)
    law = S.evade(gain=0.5)
    tab.set(["intercept", law])
    g = torch.Generator(device=DEV).manual_seed(4)
    obs = torch.randn((N, 18), device=DEV, generator=g)
    raw = torch.randn((N, 18), device=DEV, generator=g) * 100.0
    sb = torch.tensor([3], dtype=torch.int64, device=DEV)
    member = torch.tensor([1, K + 1], dtype=torch.int32, device=DEV)
    out = [torch.full((N, 3), NAN, device=DEV) for _ in range(4)]

    def launch():
        policy_act_league(H, obs, raw, live[0], live[1], 1.6, 9, 0, 2, *out, 1, pool, member, tab, step_base=sb)

    def expect(members):
        for b, m in enumerate(members):
            rows = _block_rows(b, N)
            if m >= K:
                assert _same(out[2][rows], S.scripted_act(raw, tab.laws[m - K])[rows]), (members, b)
                assert _is_pos_zero(out[3][rows]), (members, b)
                ref = _plain(H, obs, live[0], live[1], 9, 0, 2, sb)
                assert _same(out[0][rows], ref[0][rows]) and _same(out[1][rows], ref[1][rows]), (members, b)
            else:
                ref = _plain(H, obs, live[0], live[1] if m < 0 else pool[m], 9, 0, 2, sb)
                for x, y in zip(out, ref):
                    assert _same(x[rows], y[rows]), (members, b)

    launch()                                                 # eager once before the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        launch()
    for t in out:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    expect([1, K + 1])
    before = out[2][32:].clone()
    member.copy_(torch.tensor([K + 1, 0], dtype=torch.int32))            # in place, no recapture
    pool[0, :total].copy_(live[0])                                       # slot 0 <- another parameter set
    law.update(G=S.evade_matrix(gain=0.125), b=[0.01, -0.02, 0.03])      # the law's row of the table, in place
    for t in out:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    expect([K + 1, 0])
    assert not _same(S.scripted_act(raw, law)[32:], before)              # the update did change the law's actions


# ---------------------------------------------------------------------------
# 3. the tally kernel
# ---------------------------------------------------------------------------
def _count(rew, done, cap, N):
    nb = (N + 31) // 32
    out = np.zeros((nb, 2), dtype=np.int64)
    for b in range(nb):
        d = done[:, 32 * b:32 * (b + 1)] != 0
        out[b, 0] = d.sum()
        out[b, 1] = (d & (rew[:, 32 * b:32 * (b + 1)] == np.float32(cap))).sum()
    return out


def test_league_tally_counts_episodes_and_captures_per_block():
    from satrl.pool import league_tally
    T, N, cap, timeout = 5, 39, 150.0, -20.0
    rng = np.random.default_rng(3)
    rew = rng.normal(size=(T, N)).astype(np.float32)
    done = np.zeros((T, N), dtype=np.uint8)
    for t, i, r, d in ((0, 0, cap, 1), (4, 0, cap, 1), (2, 5, timeout, 1), (3, 31, cap, 1), (1, 32, cap, 1),
                       (4, 38, timeout, 1), (4, 37, cap, 255),       # any non-zero done byte counts
                       (2, 7, cap, 0), (0, 33, cap, 0),              # the capture literal on a step that is not done
                       (1, 20, np.nextafter(np.float32(cap), np.float32(0)), 1)):   # a done step one ulp below it
        rew[t, i], done[t, i] = r, d
    want = _count(rew, done, cap, N)
    assert want.tolist() == [[5, 3], [3, 2]]
    G = 8
    big = torch.full((2 + G, 2), -7, dtype=torch.int64, device=DEV)
    tally = big[:2]
    tally.zero_()
    r_d, d_d = torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV)
    league_tally(r_d, d_d, cap, tally)
    torch.cuda.synchronize()
    assert np.array_equal(tally.cpu().numpy(), want)
    league_tally(r_d, d_d, cap, tally)                       # a second call adds to the first
    torch.cuda.synchronize()
    assert np.array_equal(tally.cpu().numpy(), 2 * want)
    assert bool((big[2:] == -7).all())                       # nothing outside [ceil(N / 32)][2]
    assert np.array_equal(r_d.cpu().numpy(), rew) and np.array_equal(d_d.cpu().numpy(), done)
    # more than one workgroup, a ragged last half-wave, T above the unroll
    T, N = 19, 167
    rew = np.where(rng.random((T, N)) < 0.3, np.float32(cap), np.float32(-20.0)).astype(np.float32)
    done = (rng.random((T, N)) < 0.4).astype(np.uint8)
    tally = torch.zeros(((N + 31) // 32, 2), dtype=torch.int64, device=DEV)
    league_tally(torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV), cap, tally)
    torch.cuda.synchronize()
    assert np.array_equal(tally.cpu().numpy(), _count(rew, done, cap, N))


# ---------------------------------------------------------------------------
# 4. the trainer
# ---------------------------------------------------------------------------
# (opponent_seed 4: by the host rule, blocks 0..3 of iterations 0..2 then mix live, stored and law members)
OPP_SEED = 4
LEAGUE = dict(opponent_pool=4, opponent_latest_prob=0.25, opponent_seed=OPP_SEED, league_law_prob=0.5)


def _evader_laws():
    from satrl import scripted as S
    return [S.evade(gain=0.5), S.ScriptedLaw(np.zeros((3, 18)), [0.4, -0.3, 0.2], 1.6)]


def _trainer(use_graphs=True, env_offset=0, flag=0, **kw):
    from satrl.trainer import VecTrainer
    return VecTrainer(_args(**kw), flag=flag, d_capture=15000.0, env_offset=env_offset, use_graphs=use_graphs)


def _league_trainer(use_graphs=True, env_offset=0, **kw):
    kw = dict(LEAGUE, **kw)
    kw.setdefault("league_laws", {"evader": _evader_laws()})
    return _trainer(use_graphs, env_offset, **kw)


def _fill_evader_pool(tr, n):
    P = tr.evader.P
    for j, d in enumerate(_perturbations(P.numel(), n)):
        tr.pools["evader"].add(P + d.to(DEV), {"agent": "evader", "iteration_count": -1 - j, "episodes": 0.0})


def _recount(tr, rows):
    """(episodes, captures) per league member from the rollout table and last_assignment, on the host."""
    from satrl.evaluate import capture_reward_of
    cap = np.float32(capture_reward_of(tr.env._p, tr.flag))
    rew, done = tr.buf.rew.cpu().numpy(), tr.buf.done.cpu().numpy()
    out = np.zeros((rows, 2), dtype=np.int64)
    for b, m in enumerate(tr.last_assignment.tolist()):
        d = done[:, 32 * b:32 * (b + 1)] != 0
        out[m + 1, 0] += d.sum()
        out[m + 1, 1] += (d & (rew[:, 32 * b:32 * (b + 1)] == cap)).sum()
    return out


@pytest.mark.parametrize("use_graphs", [True, False])
def test_trainer_plays_the_assigned_league_members(use_graphs):
    from satrl.pool import league_assign
    from satrl.scripted import scripted_act
    tr = _league_trainer(use_graphs)
    _fill_evader_pool(tr, 3)
    N, T, H, K = tr.N, tr.T, tr.pursuer.H, 4
    pool, laws = tr.pools["evader"], tr.league_laws("evader")
    assert len(laws) == 2 and laws[0].block(tr.device).data_ptr() == tr._league["evader"].storage.data_ptr()
    ptr0 = (tr.member.data_ptr(), pool.storage.data_ptr(), tr._league["evader"].storage.data_ptr())
    total = np.zeros((1 + K + 8, 2), dtype=np.int64)
    kinds, seen = set(), []
    for it in range(3):
        base = tr.rollout_steps
        tr.collect()
        torch.cuda.synchronize()
        want = league_assign(OPP_SEED, it, 0, 4, K, 3, 2, 0.25, 0.5)
        assert np.array_equal(tr.last_assignment, want) and np.array_equal(tr.member.cpu().numpy(), want), it
        sb = torch.tensor([base], dtype=torch.int64, device=DEV)
        obs = tr.buf.obs[T - 1]
        live = _plain(H, obs, tr.pursuer.P, tr.evader.P, tr.seed, tr.env_offset, T - 1, sb)
        for b, m in enumerate(want.tolist()):
            rows = _block_rows(b, N)
            assert _same(tr.buf.act[T - 1][rows], live[0][rows]), (it, b)        # the learner: its live parameters
            assert _same(tr.buf.logp[T - 1][rows], live[1][rows]), (it, b)
            if m >= K:
                kinds.add("law")
                assert _same(tr.other_a[rows], scripted_act(obs, laws[m - K])[rows]), (it, b, m)
                assert _is_pos_zero(tr.other_lp[rows]), (it, b, m)
            elif m >= 0:
                kinds.add("stored")
                ref = _plain(H, obs, tr.pursuer.P, pool.slot(m), tr.seed, tr.env_offset, T - 1, sb)
                assert _same(tr.other_a[rows], ref[2][rows]) and _same(tr.other_lp[rows], ref[3][rows]), (it, b, m)
                assert not _same(tr.other_a[rows], live[2][rows]), (it, b)
            else:
                kinds.add("live")
                assert _same(tr.other_a[rows], live[2][rows]) and _same(tr.other_lp[rows], live[3][rows]), (it, b)
        total += _recount(tr, 1 + K + 8)
        seen.append(len(tr._graphs))
        tr.finish_iteration()
        # league_table() is the host recount of the rollouts so far
        table = tr.league_table()
        assert [(r[0], r[1]) for r in table] == [(-1, "live"), (0, "stored"), (1, "stored"), (2, "stored"),
                                                  (K, "law"), (K + 1, "law")]
        assert [list(r[3:]) for r in table] == total[[0, 1, 2, 3, 1 + K, 2 + K]].tolist(), it
        assert np.array_equal(tr.league_counts["evader"], total) and not tr.league_counts["pursuer"].any()
        assert table[1][2]["iteration_count"] == -1 and table[4][2] == {"agent": "evader", "law": 0}
    assert kinds == {"live", "stored", "law"}                                 # the three kinds of opponent, mixed
    assert total[:, 0].sum() >= 3 * N                                         # every env finished episodes
    if use_graphs:
        assert seen == [(T + tr.chunk - 1) // tr.chunk] * 3                   # replayed, not recaptured
    assert ptr0 == (tr.member.data_ptr(), pool.storage.data_ptr(), tr._league["evader"].storage.data_ptr())


def test_league_rollout_and_counts_are_sharding_invariant():
    whole = _league_trainer(True, num_envs=128)
    parts = [_league_trainer(True, num_envs=64, env_offset=o) for o in (0, 64)]
    for tr in [whole] + parts:
        _fill_evader_pool(tr, 3)
    kinds = set()
    for it in range(2):
        for tr in [whole] + parts:
            tr.collect()
        torch.cuda.synchronize()
        a = whole.last_assignment
        kinds |= {("law" if m >= 4 else "stored" if m >= 0 else "live") for m in a.tolist()}
        for k, tr in enumerate(parts):
            assert np.array_equal(tr.last_assignment, a[2 * k:2 * k + 2]), (it, k)
            cols = slice(64 * k, 64 * (k + 1))
            for name in ("act", "logp", "obs", "rew", "done"):
                x, y = getattr(tr.buf, name), getattr(whole.buf, name)[:, cols]
                assert torch.equal(x.contiguous().view(torch.uint8).cpu(), y.contiguous().view(torch.uint8).cpu()), \
                    (it, k, name)
        for tr in [whole] + parts:
            tr.finish_iteration()
        both = parts[0].league_counts["evader"] + parts[1].league_counts["evader"]
        assert np.array_equal(whole.league_counts["evader"], both) and both.any(), it
    assert kinds == {"live", "stored", "law"}


@pytest.mark.parametrize("use_graphs", [True, False])
def test_trainer_without_league_keywords_collects_what_the_pooled_trainer_collects(use_graphs):
    """league_laws=None and uniform weighting: the pooled launch and
    satrl_opponent_assign, as a trainer built without the keywords."""
    import satrl.trainer as TR
    kw = dict(opponent_pool=4, opponent_latest_prob=0.5, opponent_seed=1)
    a = _trainer(use_graphs, league_laws=None, opponent_weighting="uniform", **kw)
    b = _trainer(use_graphs, **kw)
    calls = []
    league, assign = TR.policy_act_league, TR._pool.league_assign
    TR.policy_act_league = lambda *x, **k: calls.append("act") or league(*x, **k)
    TR._pool.league_assign = lambda *x, **k: calls.append("assign") or assign(*x, **k)
    try:
        for tr in (a, b):
            _fill_evader_pool(tr, 3)
        for it in range(2):
            for tr in (a, b):
                tr.collect()
            torch.cuda.synchronize()
            assert np.array_equal(a.last_assignment, b.last_assignment)
            if it == 0:                                      # live and stored opponents in this rollout
                assert (a.last_assignment >= 0).any() and (a.last_assignment == -1).any()
            for name in ("obs", "act", "logp", "rew", "done"):
                x, y = getattr(a.buf, name), getattr(b.buf, name)
                assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (it, name)
            assert _same(a.other_a, b.other_a) and _same(a.other_lp, b.other_lp)
            for tr in (a, b):
                tr.finish_iteration()
    finally:
        TR.policy_act_league, TR._pool.league_assign = league, assign
    assert calls == []                                       # neither the league kernel nor the league rule ran


def test_pfsp_assignment_follows_the_counts():
    from satrl.pool import league_assign, pfsp_weights
    K, filled, nb = 4, 3, 4
    counts = np.zeros((1 + K + 8, 2), dtype=np.int64)
    counts[1:4] = [[400, 399], [400, 1], [400, 398]]              # the pursuer wins against slots 0 and 2, loses to 1
    w = pfsp_weights(counts[1:4, 0], counts[1:4, 1], 2)
    assert w[1] > 100 * w[0] and w[1] > 100 * w[2]
    # a seed, found on the host, under which the weighted and the uniform rule differ at iteration 0
    seed = next(s for s in range(64)
                if not np.array_equal(league_assign(s, 0, 0, nb, K, filled, 2, 0.0, 0.25, w),
                                      league_assign(s, 0, 0, nb, K, filled, 2, 0.0, 0.25, None)))
    tr = _league_trainer(True, opponent_latest_prob=0.0, league_law_prob=0.25, opponent_weighting="pfsp",
                         opponent_seed=seed)
    _fill_evader_pool(tr, filled)
    d = tr.state_dict()
    assert d["league"]["weighting"] == "pfsp" and not d["league"]["counts"]["evader"].any()
    d["league"]["counts"]["evader"] = counts
    tr.load_state_dict(d)
    assert np.array_equal(tr.league_counts["evader"], counts)
    tr.collect()
    torch.cuda.synchronize()
    want = league_assign(seed, 0, 0, nb, K, filled, 2, 0.0, 0.25, w)
    assert np.array_equal(tr.last_assignment, want)
    assert not np.array_equal(want, league_assign(seed, 0, 0, nb, K, filled, 2, 0.0, 0.25, None))
    stored = want[(want >= 0) & (want < K)]
    assert (stored == 1).all()                               # what the learner loses to
    tr.finish_iteration()
    # the learner's wins under Flag 1 are the episodes that did not end in a capture
    ev = _league_trainer(True, flag=1, opponent_weighting="pfsp", league_laws={"pursuer": ["intercept"]})
    c = np.array([[10, 7], [4, 0]])
    assert ev._learner_wins(c).tolist() == [3, 4] and tr._learner_wins(c).tolist() == [7, 0]
    # a slot the ring overwrites starts again at zero
    tr.league_counts["pursuer"][1:3] = 5
    assert tr.snapshot_opponent() == 0 and tr.league_counts["pursuer"][1].tolist() == [0, 0]
    assert tr.league_counts["pursuer"][2].tolist() == [5, 5]


def _snap(tr):
    torch.cuda.synchronize()
    out = {"iteration_count": np.asarray(tr.iteration_count), "episodes": np.asarray(tr.episodes),
           "obs0": tr.buf.obs[0].cpu().numpy(), "member": tr.last_assignment.copy()}
    for name, L in (("pursuer", tr.pursuer), ("evader", tr.evader)):
        for k in ("P", "M", "V", "steps"):
            out[f"{name}.{k}"] = getattr(L, k).cpu().numpy()
    for name in ("obs", "act", "logp", "rew", "done"):
        out["buf." + name] = getattr(tr.buf, name).cpu().numpy()
    for k, v in tr.env.full_state().items():
        out["env." + k] = v
    for agent in ("pursuer", "evader"):
        out["counts." + agent] = tr.league_counts[agent].copy()
        out["pool." + agent] = tr.pools[agent].storage.cpu().numpy()
        out["laws." + agent] = tr._league[agent].storage.cpu().numpy()
    return out


def test_checkpoint_resumes_a_league_run_bitwise(tmp_path):
    kw = dict(num_envs=64, batch_size=512, opponent_snapshot_every=1, opponent_weighting="pfsp", pfsp_power=3,
              opponent_latest_prob=0.25, league_law_prob=0.5)

    def make(**over):
        tr = _league_trainer(True, **dict(kw, **over))
        _fill_evader_pool(tr, 2)
        return tr

    A = make()
    for _ in range(3):
        A.iteration()
    want = _snap(A)
    B = make()
    B.iteration()
    B.save_checkpoint(tmp_path / "ck")
    one = _snap(B)
    # a fresh trainer built WITHOUT the laws and with other league settings: the checkpoint carries them
    C = make(league_laws=None, league_law_prob=0.125, opponent_weighting="uniform", pfsp_power=2)
    C.load_checkpoint(tmp_path / "ck")
    assert (C.league_law_prob, C.opponent_weighting, C.pfsp_power) == (0.5, "pfsp", 3)
    assert len(C.league_laws("evader")) == 2 and C.league_laws("pursuer") == []
    got = _snap(C)
    for k in ("counts.evader", "counts.pursuer", "laws.evader", "pool.evader", "pool.pursuer", "evader.P", "pursuer.P",
              "obs0"):
        assert np.array_equal(got[k], one[k]), k
    assert one["counts.evader"].any()
    for _ in range(2):
        C.iteration()
    got = _snap(C)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k
    assert want["counts.evader"][:, 0].sum() > one["counts.evader"][:, 0].sum()
    # a reader of another sharding reads the same global counts
    D = _league_trainer(True, **dict(kw, num_envs=32, batch_size=256, env_offset=32))
    D.load_checkpoint(tmp_path / "ck", global_envs=64)
    for agent in ("pursuer", "evader"):
        assert np.array_equal(D.league_counts[agent], one["counts." + agent]), agent


def test_evaluate_pool_gains_a_row_per_law():
    tr = _league_trainer(True)
    _fill_evader_pool(tr, 2)
    plain = _trainer(True, opponent_pool=4, opponent_seed=1)
    _fill_evader_pool(plain, 2)
    laws = tr.league_laws()
    table, base = tr.evaluate_pool(), plain.evaluate_pool()
    assert len(base) == 2 and len(table) == 4
    assert [m for m, _ in table[:2]] == [m for m, _ in base]
    assert [repr(s) for _, s in table[:2]] == [repr(s) for _, s in base]           # the first rows are unchanged
    assert [m for m, _ in table[2:]] == [{"agent": "evader", "law": 0}, {"agent": "evader", "law": 1}]
    for j, law in enumerate(laws):
        assert repr(table[2 + j][1]) == repr(tr.evaluate(opponent=law).summary()), j
    assert repr(table[2][1]) != repr(table[3][1])


def test_set_league_laws_keeps_the_graphs_unless_the_launch_changes():
    from satrl import scripted as S
    tr = _league_trainer(True)
    _fill_evader_pool(tr, 2)
    tr.collect()
    tr.finish_iteration()
    n = len(tr._graphs)
    assert n == (tr.T + tr.chunk - 1) // tr.chunk
    first = next(iter(tr._graphs.values()))
    keep = tr.league_laws("evader")[1]
    row1 = keep.block(tr.device).data_ptr()
    before = repr(tr.evaluate(opponent=keep).summary())                            # an evaluator graph on keep's row
    tr.set_league_laws("evader", [keep, S.evade(gain=0.25), "intercept"])          # 2 -> 3 laws: the same launch
    assert len(tr._graphs) == n and next(iter(tr._graphs.values())) is first
    # keep moved from row 1 to row 0: the evaluator's graphs were dropped with the move and read the new row
    assert keep.block(tr.device).data_ptr() == row1 - S.LAW_BYTES
    assert repr(tr.evaluate(opponent=keep).summary()) == before
    assert repr(tr.evaluate(opponent=tr.league_laws("evader")[1]).summary()) != before
    used = S.coast()
    used.block(tr.device)                                                          # a law that owns a block already
    with pytest.raises(ValueError, match="already owns"):
        tr.set_league_laws("evader", [used])
    assert len(tr.league_laws("evader")) == 3                                      # a refused set changes nothing
    assert not tr.league_counts["evader"][5:].any()
    tr.collect()
    torch.cuda.synchronize()
    assert (tr.last_assignment < 4 + 3).all()
    tr.finish_iteration()
    tr.set_league_laws("evader", None)                                             # to zero: the pooled launch
    assert tr._graphs == {} and tr.league_laws("evader") == []
    with pytest.raises(ValueError, match="not supported"):
        tr.set_scripted_opponent("evader", "coast")                                # still refused on a pooled trainer
    with pytest.raises(ValueError):
        _trainer(True).set_league_laws("evader", ["coast"])                        # no pool


def test_a_state_without_a_league_entry_keeps_the_constructors_settings():
    """A state written before league play has no "league" entry: the laws, the
    law probability, the weighting and the power stay what the trainer was
    built with, and the counts are zero."""
    tr = _league_trainer(True, opponent_weighting="pfsp", pfsp_power=3)
    _fill_evader_pool(tr, 2)
    tr.iteration()
    assert tr.league_counts["evader"].any()
    d = tr.state_dict()
    assert "league" in d
    del d["league"]
    laws = tr.league_laws("evader")
    tr.load_state_dict(d)
    assert (tr.league_law_prob, tr.opponent_weighting, tr.pfsp_power) == (0.5, "pfsp", 3)
    got = tr.league_laws("evader")
    assert len(got) == 2 and all(x is y for x, y in zip(got, laws))
    assert not tr.league_counts["evader"].any() and not tr.league_counts["pursuer"].any()
    tr.iteration()                                                                 # and the run goes on
    assert tr.league_counts["evader"].any()
