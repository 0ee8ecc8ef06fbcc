"""The exploration noise on the MI355X against its NumPy restatement
(sample_reference.py, checked on its own in test_sample_cpu.py): the z of
philox_normal4 through satrl_gaussian_sample, gaussian_act's clamp and
log-prob at their edges, the same draw through the fused policy kernels, and
the key of every action VecTrainer.collect() stores.

Tolerances come from the number formats, not from the kernels: the z of the
kernel against the f64 z of the restatement (whose angle is the kernel's f32
angle bit for bit) within 16 * 2^-24 * max(1, r), twice the sum of the device
library's documented bounds (logf 3 ulp, cosf / sinf 4 ulp, sqrtf 1 ulp, two
product roundings); a log-prob against the f64 Normal log-density at the
kernel's own action within 2^-20 * (q + |log_std| + 1), q = (a - mean)^2 / 2 var.
"""
import itertools

import numpy as np
import pytest
import torch

import sample_reference as SR
from sample_reference import EDGE_IDS, R_MAX_IDS, R_ZERO_IDS

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32_1P6 = np.float32(1.6)
SEED_HI = (0x9E3779B9 << 32) | 7          # a non-zero high word: k1 depends on it
TRAINER_SEED = (5 << 32) | 7              # ... and one whose multiples VecTrainer's torch generators still take


def _args(**kw):
    from satrl.trainer import args_param
    a = args_param(chkpt_dir="/tmp", **kw)
    a.state_dim, a.action_dim, a.max_action = 18, 3, 1.6
    return a


def _z_gpu(n, seed, agent, env_offset, step, step_base=None):
    """The kernel's z[:, :3]: mean 0, log_std 0 (expf(0) == 1, 0 + 1 * z == z), no clamp."""
    from satrl.ppo import gaussian_sample
    mean = torch.zeros((n, 3), device=DEV)
    sb = None if step_base is None else torch.tensor([step_base], dtype=torch.int64, device=DEV)
    a, lp = gaussian_sample(mean, torch.zeros(3, device=DEV), 1e30, seed, agent, env_offset, step, step_base=sb)
    return a.cpu().numpy(), lp.cpu().numpy()


def _check_z(got, seed, agent, gids, step, what):
    """got f32 [n, 3] within the z tolerance of the restatement; returns max |dz| / max(1, r)."""
    z, r0, r1 = SR.normals(seed, agent, gids, step)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - z[:, :3]) / np.maximum(1.0, SR.radius3(r0, r1))
    worst = float(err.max())
    print(f"{what}: max |dz| / max(1, r) = {worst / 2.0 ** -24:.3f} * 2^-24 (tolerance 16)")
    assert worst <= SR.Z_TOL, (what, worst, int(err.argmax()))
    return worst


def _check_logp(lp, a, mean, log_std, what, show=True):
    """lp f32 within the log-prob tolerance of the f64 density at the kernel's own action a."""
    ref = SR.logp_of(a, mean, log_std)
    ratio = np.abs(lp.astype(np.float64) - ref) / SR.logp_tol(a, mean, log_std)
    worst = float(ratio.max())
    if show:
        print(f"{what}: max log-prob error / tolerance = {worst:.3f}")
    assert worst <= 1.0, (what, worst, int(ratio.argmax()))
    return worst


# (seed, agent, env_offset, N, step, device step_base)
Z_CASES = {
    "n4099": (7, 0, 0, 4099, 3, None),
    "agent1": (7, 1, 0, 257, 3, None),
    "gid_low_word_wraps": (7, 0, 2 ** 32 - 16, 33, 3, None),
    "gid_2p40": (7, 1, 2 ** 40 + 5, 33, 3, None),
    "step_carries_into_word3": (7, 0, 11, 33, 2 ** 32 - 1, 2),
    "step_2p33": (7, 1, 11, 33, 2 ** 33, None),
    "seed_high_word": (SEED_HI, 0, 11, 33, 3, 0),
}


@pytest.mark.parametrize("case", list(Z_CASES))
def test_z_matches_the_restatement(case):
    """philox_normal4's z[0:3] through satrl_gaussian_sample: 4099 envs (16
    full workgroups and a ragged one) and short launches at the counter's
    edges -- an env id whose low word wraps, one above 2^40, a step + *step_base
    that carries into the counter's fourth word, a step of 2^33, a seed with a
    high word, both agents.  Measured on the MI355X: max |dz| / max(1, r) =
    2.45 * 2^-24 over all cases (at N 4099; tolerance 16 * 2^-24)."""
    seed, agent, off, n, step, sb = Z_CASES[case]
    got, lp = _z_gpu(n, seed, agent, off, step, sb)
    gids = [off + i for i in range(n)]
    _check_z(got, seed, agent, gids, step + (sb or 0), case)
    _check_logp(lp, got, 0.0, 0.0, case)
    if case == "seed_high_word":
        low, _ = _z_gpu(n, seed & 0xFFFFFFFF, agent, off, step, sb)
        assert not np.array_equal(low, got)


def test_step_base_none_is_a_device_zero():
    a, lp = _z_gpu(33, 7, 0, 2 ** 32 - 16, 2 ** 32 - 1, None)
    b, lq = _z_gpu(33, 7, 0, 2 ** 32 - 16, 2 ** 32 - 1, 0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(lp.view(np.uint32), lq.view(np.uint32))
    # and step + *step_base is one 64-bit sum: (2^32 - 1) + 2 == 2^32 + 1
    c, _ = _z_gpu(33, 7, 0, 2 ** 32 - 16, 2 ** 32 - 1, 2)
    d, _ = _z_gpu(33, 7, 0, 2 ** 32 - 16, 2 ** 32 + 1, None)
    assert np.array_equal(c.view(np.uint32), d.view(np.uint32))
    assert not np.array_equal(a, c)


def test_z_at_the_extreme_radii():
    """The env ids of test_sample_cpu.EDGE_IDS (seed 7, agent 0, step 3):
    u0 = 2^-24, the largest radius sqrt(2 ln 2^24), within the z tolerance;
    u0 = 1, r = 0: z0 and z1 exactly zero (logf(1) == 0, sqrtf(-0) == -0)."""
    for gid in EDGE_IDS:
        got, lp = _z_gpu(2, 7, 0, gid, 3)
        _check_z(got, 7, 0, [gid, gid + 1], 3, f"env id {gid}")
        _check_logp(lp, got, 0.0, 0.0, f"env id {gid}")
        if gid in R_ZERO_IDS:
            assert got[0, 0] == 0.0 and got[0, 1] == 0.0, (gid, got[0])
        else:
            assert gid in R_MAX_IDS
            assert abs(np.hypot(float(got[0, 0]), float(got[0, 1])) - 5.768107) < 1e-4, (gid, got[0])


LOG_STDS = [-5.0, -3.0, -0.5, 0.0, 0.4, 2.0]
MEANS = [-2.0, -1.6, -1.0, 0.0, 0.3, 1.6, 2.0]


def _log_std_triples():
    """Every triple of the six values: 216."""
    return list(itertools.product(LOG_STDS, repeat=3))


def test_clamp_and_logprob_edges():
    """gaussian_act over log_std in {-5 .. 2} per dimension and means on and
    outside the +-1.6 box (4096 rows per log_std triple, all 216 triples): the
    action against clamp(mean + sd * z_ref) within sd * tol_z + 2^-23 *
    max(|a|, |mean|) (the z error scaled by sd, one ulp for the add), a
    clamped action bitwise +-1.6f, and the log-prob against the f64 density at
    the kernel's own action within 2^-20 * (q + |log_std| + 1); q reaches
    ~1800 at log_std -5.  Measured on the MI355X: max log-prob error /
    tolerance = 0.184; max action error / tolerance = 0.476."""
    from satrl.ppo import gaussian_sample
    n, seed, step = 4096, 7, 5
    rng = np.random.default_rng(21)
    worst_lp, worst_a, q_max, clamped = 0.0, 0.0, 0.0, 0
    lim = float(F32_1P6)
    for k, tri in enumerate(_log_std_triples()):
        mean = (rng.choice(MEANS, (n, 3)) + rng.normal(0.0, 1e-3, (n, 3))).astype(np.float32)
        ls = np.float32(tri)
        off = k * n
        a, lp = gaussian_sample(torch.tensor(mean, device=DEV), torch.tensor(ls, device=DEV), 1.6, seed, k & 1, off,
                                step)
        a, lp = a.cpu().numpy(), lp.cpu().numpy()
        z, r0, r1 = SR.normals(seed, k & 1, np.arange(off, off + n), step)
        m64, sd = mean.astype(np.float64), np.exp(ls.astype(np.float64))
        raw = m64 + sd * z[:, :3]
        ref, _ = SR.act_logp(mean, ls, z[:, :3], 1.6)
        tol = sd * SR.z_tol(r0, r1) + 2.0 ** -23 * np.maximum(np.abs(a.astype(np.float64)), np.abs(m64))
        ea = np.abs(a.astype(np.float64) - ref) / tol
        worst_a = max(worst_a, float(ea.max()))
        assert ea.max() <= 1.0, (tri, float(ea.max()), int(ea.argmax()))
        assert (np.abs(a) <= F32_1P6).all()
        hi, lo = raw > lim + tol, raw < -lim - tol             # clamped beyond any doubt
        assert np.array_equal(a[hi].view(np.uint32), np.full(int(hi.sum()), F32_1P6).view(np.uint32))
        assert np.array_equal(a[lo].view(np.uint32), np.full(int(lo.sum()), -F32_1P6).view(np.uint32))
        clamped += int(hi.sum() + lo.sum())
        q = (a.astype(np.float64) - m64) ** 2 / (2.0 * sd ** 2)
        q_max = max(q_max, float(q.max()))
        worst_lp = max(worst_lp, _check_logp(lp, a, mean, ls, f"log_std {tri}", show=False))
    print(f"clamp / log-prob edges: max log-prob error / tolerance {worst_lp:.3f}, max action error / tolerance "
          f"{worst_a:.3f}; {clamped} clamped actions, q up to {q_max:.0f}")
    assert clamped > 1000 and q_max > 1000.0                   # the grid reaches what it is there for


def _zeroed_pair(H):
    """A pursuer / evader PPOLearner pair whose actors' mean is 0 and std 1
    whatever the observation (mean layer and log_std zeroed in P)."""
    from satrl.ppo import PPOLearner
    torch.manual_seed(5)
    args = _args(hidden_width=H)
    pair = [PPOLearner(args, who, use_graph=False) for who in ("pursuer", "evader")]
    for L in pair:
        _zero_mean_layer(L)
    return pair


def _zero_mean_layer(L):
    with torch.no_grad():
        L.actor.mean_layer.weight.zero_()
        L.actor.mean_layer.bias.zero_()
        L.actor.log_std.zero_()
    v = L.flat_views(L.P)
    assert not v["actor.mean_layer.weight"].any() and not v["actor.log_std"].any()     # views into P


@pytest.mark.parametrize("H", [64, 128, 256])
def test_policy_kernels_draw_the_same_z(H):
    """satrl_policy_act at every width, one full 32-row workgroup and a ragged
    one, at an env id whose low word wraps and a step + *step_base that carries:
    with a zero mean layer and max_action 1e30 the actions are z, agent 0's
    from key (seed, 0) and agent 1's from (seed, 1).  At H 64 satrl_policy_eval's
    sampled agent is bitwise policy_act's."""
    from satrl.ppo import policy_act, policy_eval
    Lp, Le = _zeroed_pair(H)
    n, off, step, sb = 33, 2 ** 32 - 16, 2 ** 32 - 1, 2
    g = torch.Generator(device=DEV).manual_seed(2)
    obs = torch.randn((n, 18), device=DEV, generator=g)
    base = torch.tensor([sb], dtype=torch.int64, device=DEV)
    out = [torch.full((n, 3), float("nan"), device=DEV) for _ in range(4)]
    policy_act(H, obs, Lp.P, Le.P, 1e30, SEED_HI, off, step, *out, step_base=base)
    gids = [off + i for i in range(n)]
    for agent in (0, 1):
        a, lp = out[2 * agent].cpu().numpy(), out[2 * agent + 1].cpu().numpy()
        _check_z(a, SEED_HI, agent, gids, step + sb, f"policy_act H {H} agent {agent}")
        _check_logp(lp, a, 0.0, 0.0, f"policy_act H {H} agent {agent}")
    assert not torch.equal(out[0], out[2])
    if H == 64:
        for det_mask in (1, 2):                                # the other agent samples
            ev = [torch.full((n, 3), float("nan"), device=DEV) for _ in range(2)]
            policy_eval(H, obs, Lp.P, Le.P, 1e30, det_mask, SEED_HI, off, step, ev[0], ev[1], step_base=base)
            s = 2 - det_mask                                   # det_mask 1 -> agent 1, 2 -> agent 0
            assert torch.equal(ev[s].view(torch.int32), out[2 * s].view(torch.int32))
            assert not ev[1 - s].any()                         # the deterministic agent: its mean, 0


def _noise_trainer(use_graphs, flag, num_envs, env_offset):
    from satrl.trainer import VecTrainer
    args = _args(hidden_width=64, num_envs=num_envs, horizon=5, rollout_graph_chunk=2, max_episode_steps=12,
                 batch_size=5 * num_envs, mini_batch_size=5 * num_envs, seed=TRAINER_SEED)
    tr = VecTrainer(args, flag=flag, d_capture=15000.0, env_offset=env_offset, use_graphs=use_graphs)
    for L in (tr.pursuer, tr.evader):
        _zero_mean_layer(L)
    return tr


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("use_graphs", [True, False])
def test_trainer_noise_stream(use_graphs, flag):
    """The key of every action collect() stores: (seed, the learner's agent id,
    env_offset + j, the count of rollout steps before step t), through the
    captured rollout graphs (chunks of 2 over a horizon of 5) and eagerly.  70
    envs: two full 32-row workgroups and a ragged one.  With zeroed mean layers
    buf.act[t, j] is clamp(z, +-1.6); the second collect() continues the step
    count, so no iteration explores with an earlier one's noise; a trainer of
    envs 64..69 alone draws those envs' rows bit for bit."""
    T, N = 5, 70
    tr = _noise_trainer(use_graphs, flag, N, 0)
    sub = _noise_trainer(use_graphs, flag, 6, 64)
    gids = np.arange(N)
    acts = []
    for call in range(2):
        before = tr.rollout_steps
        assert before == call * T
        tr.collect()
        sub.collect()
        torch.cuda.synchronize()
        act, logp = tr.buf.act.cpu().numpy(), tr.buf.logp.cpu().numpy()
        for t in range(T):
            z, r0, r1 = SR.normals(TRAINER_SEED, flag, gids, before + t)
            ref, _ = SR.act_logp(np.zeros((N, 3)), np.zeros(3), z[:, :3], 1.6)
            err = np.abs(act[t].astype(np.float64) - ref) / SR.z_tol(r0, r1)
            assert err.max() <= 1.0, (call, t, float(err.max()), int(err.argmax()))
            assert (np.abs(act[t]) <= F32_1P6).all()
            _check_logp(logp[t], act[t], 0.0, 0.0, f"collect {call} step {t}", show=False)
        z, r0, r1 = SR.normals(TRAINER_SEED, 1 - flag, gids, before + T - 1)
        ref, _ = SR.act_logp(np.zeros((N, 3)), np.zeros(3), z[:, :3], 1.6)
        err = np.abs(tr.other_a.cpu().numpy().astype(np.float64) - ref) / SR.z_tol(r0, r1)
        assert err.max() <= 1.0, (call, "other agent", float(err.max()))
        assert torch.equal(sub.buf.act.view(torch.int32), tr.buf.act[:, 64:].view(torch.int32))
        assert torch.equal(sub.buf.logp.view(torch.int32), tr.buf.logp[:, 64:].view(torch.int32))
        assert torch.equal(sub.other_a.view(torch.int32), tr.other_a[64:].view(torch.int32))
        acts.append(act)
    assert tr.rollout_steps == 2 * T
    assert (acts[0] != acts[1]).mean() > 0.9                   # clamped components may coincide
    assert tr.env.check_errors() == 0
