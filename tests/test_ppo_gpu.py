"""GPU parity of the learning-side kernels and the update.

Tolerances (DESIGN.md "Parity"):
  * GAE scan: bit-exact vs the oracle restatement on identical inputs
  * Gaussian log-prob: <= 1e-6 abs vs torch.distributions.Normal.log_prob
  * policy forward (one_layer checkpoint): <= 1e-5 rel (GEMM order)
  * one reference update(): adv / v_target <= 1e-5 rel; parameters after
    24 Adam steps within 1e-3 rel + 2*lr*steps*1% abs (Adam's m/sqrt(v) turns
    ulp-level gradient noise into up-to-lr-sized steps on near-zero grads)
"""
import numpy as np
import pytest
import torch

from conftest import golden
from update_replay import h64_case, h256_case, run_reference_update

pytestmark = pytest.mark.gpu


def test_gae_kernel_bitexact(oracle):
    from satrl.ppo import gae
    rng = np.random.default_rng(0)
    T, N = 97, 33
    r = rng.normal(0, 3, (T, N)).astype(np.float32)
    v = rng.normal(0, 10, (T + 1, N)).astype(np.float32)
    d = (rng.uniform(size=(T, N)) < 0.05).astype(np.uint8)
    adv, vt = gae(torch.tensor(r, device="cuda"), torch.tensor(d, device="cuda"), torch.tensor(v, device="cuda"),
                  0.99, 0.95)
    ref = oracle.gae_time_major(r, v[:-1], v[1:], d.astype(np.float32), d.astype(np.float32))
    assert np.array_equal(adv.cpu().numpy(), ref)
    assert np.array_equal(vt.cpu().numpy(), (ref + v[:-1]).astype(np.float32))


def test_gae_kernel_bitexact_full_size(oracle):
    """BASELINE configs[2]'s buffer (T 2048 x 16384 envs) through the HIP
    scan, bit for bit against the oracle's vectorised scan."""
    from satrl.ppo import gae
    rng = np.random.default_rng(1)
    T, N = 2048, 16384
    r = rng.normal(0, 3, (T, N)).astype(np.float32)
    v = rng.normal(0, 10, (T + 1, N)).astype(np.float32)
    d = (rng.uniform(size=(T, N)) < 0.002).astype(np.uint8)
    adv, vt = gae(torch.tensor(r, device="cuda"), torch.tensor(d, device="cuda"), torch.tensor(v, device="cuda"),
                  0.99, 0.95)
    ref = oracle.gae_time_major_vec(r, v[:-1], v[1:], d.astype(np.float32), d.astype(np.float32))
    assert np.array_equal(adv.cpu().numpy(), ref)
    assert np.array_equal(vt.cpu().numpy(), (ref + v[:-1]).astype(np.float32))


def test_gae_kernel_on_reference_buffer():
    """update_case: the reference's flat buffer as one env column."""
    from satrl.ppo import _gae_explicit
    u = golden("update_case")
    dev = "cuda"
    adv, vt = _gae_explicit(torch.tensor(u["r"].reshape(-1), device=dev), torch.tensor(u["vs"].reshape(-1), device=dev),
                            torch.tensor(u["vs_"].reshape(-1), device=dev), torch.tensor(u["dw"].reshape(-1), device=dev),
                            torch.tensor(u["done"].reshape(-1), device=dev), 0.99, 0.95)
    assert np.array_equal(adv.cpu().numpy(), u["adv"].reshape(-1))
    assert np.array_equal(vt.cpu().numpy(), u["v_target"].reshape(-1))


TANH_MAX_ULP = 2


def test_tanh_f32_ulp():
    """The MLP kernels' activation (ppo_kernels.hip tanh_f32, torch.tanh at
    ppo_continuous.py:61-134) over EVERY non-negative f32 incl. +inf: within
    TANH_MAX_ULP of tanh evaluated in f64 and rounded once to f32.  It is odd
    by construction: negatives spot-checked bitwise, NaN propagates."""
    import satrl._lib as _L
    lib, sp = _L.lib(), _L.stream_ptr()
    top = 0x7F800000                                                   # +inf
    n = 1 << 27
    y = torch.empty(n, device="cuda")
    worst, worst_x = 0, 0.0
    for c in range(0, top + 1, n):
        bits = torch.arange(c, min(c + n, top + 1), dtype=torch.int32, device="cuda")
        x = bits.view(torch.float32)
        m = x.numel()
        assert lib.satrl_ppo_tanh(m, _L.ptr(x), _L.ptr(y), sp) == 0
        ref = torch.tanh(x.double()).float()
        d = (y[:m].view(torch.int32) - ref.view(torch.int32)).abs()
        k = int(d.argmax())
        if int(d[k]) > worst:
            worst, worst_x = int(d[k]), float(x[k])
    print(f"tanh_f32: max {worst} ulp (at x = {worst_x!r})")
    assert worst <= TANH_MAX_ULP, (worst, worst_x)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(1 << 20, device="cuda", generator=g) * 4
    yp, yn = torch.empty_like(x), torch.empty_like(x)
    assert lib.satrl_ppo_tanh(x.numel(), _L.ptr(x), _L.ptr(yp), sp) == 0
    xn = -x
    assert lib.satrl_ppo_tanh(x.numel(), _L.ptr(xn), _L.ptr(yn), sp) == 0
    assert torch.equal(yn, -yp)
    nan = torch.tensor([float("nan"), float("-inf")], device="cuda")
    out = torch.empty_like(nan)
    assert lib.satrl_ppo_tanh(2, _L.ptr(nan), _L.ptr(out), sp) == 0
    assert torch.isnan(out[0]) and float(out[1]) == -1.0


def test_gaussian_sample_logprob_and_stats():
    from satrl.ppo import gaussian_sample
    N = 200000
    mean = torch.zeros((N, 3), device="cuda")
    mean[:, 1] = 0.7
    log_std = torch.tensor([[-0.5, 0.1, 0.4]], device="cuda")
    a, lp = gaussian_sample(mean, log_std, 1.6, seed=7, agent=0, env_offset=0, step=3)
    std = log_std.exp()
    ref = torch.distributions.Normal(mean, std.expand_as(mean)).log_prob(a)
    assert torch.allclose(lp, ref, atol=1e-6, rtol=0)
    assert float(a.abs().max()) <= float(torch.tensor(1.6, dtype=torch.float32))
    m = a[:, 0].mean().item(); s = a[:, 0].std().item()
    assert abs(m) < 0.01 and abs(s - float(std[0, 0])) < 0.01
    # deterministic, keyed by (seed, agent, env id, step); sharding-invariant
    a2, _ = gaussian_sample(mean, log_std, 1.6, seed=7, agent=0, env_offset=0, step=3)
    assert torch.equal(a, a2)
    a3, _ = gaussian_sample(mean[1000:], log_std, 1.6, seed=7, agent=0, env_offset=1000, step=3)
    assert torch.equal(a[1000:], a3)
    a4, _ = gaussian_sample(mean, log_std, 1.6, seed=7, agent=1, env_offset=0, step=3)
    assert not torch.equal(a, a4)


def _args(**kw):
    from satrl.trainer import args_param
    a = args_param(chkpt_dir="/tmp", **kw)
    a.state_dim, a.action_dim, a.max_action = 18, 3, 1.6
    return a


def test_policy_forward_one_layer_checkpoint():
    from satrl.ppo import Actor_Gaussian, Critic
    g = golden("policy_one_layer")
    args = _args()
    actor = Actor_Gaussian(args, "pursuer")
    critic = Critic(args, "pursuer")
    actor.load_state_dict({k[6:]: torch.tensor(g[k]) for k in g.files if k.startswith("actor.")})
    critic.load_state_dict({k[7:]: torch.tensor(g[k]) for k in g.files if k.startswith("critic.")})
    actor.cuda(); critic.cuda()
    obs = torch.tensor(g["obs"], device="cuda")
    with torch.no_grad():
        mean = actor(obs).cpu().numpy()
        v = critic(obs).cpu().numpy()
    np.testing.assert_allclose(mean, g["mean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(v, g["value"], rtol=1e-5, atol=1e-4)


def test_update_matches_reference():
    """ppo_continuous.py:191-250 with the reference's own buffer and
    minibatch permutations (captured), through the drop-in PPO_continuous.
    5e-5 absolute: about 1 % of the movement 24 Adam steps at lr 2e-4 can
    make (lr * nsteps = 4.8e-3), 2.8x the measured worst (1.8e-5, the f32
    gradient sums adding in another order than torch's).  The buffer is a
    real env rollout, states at the env's raw metre scale (~1e5): fc1's
    pre-activations are sums of large terms cancelling to O(1), so any f32
    summation order moves tanh' and dW1 visibly -- the well-conditioned
    captures at the product's shapes (update_h64.npz / update_h256.npz,
    below) hold every width to 1e-6."""
    u = golden("update_case")
    run_reference_update({k: u[k] for k in u.files})


@pytest.mark.parametrize("case", ["kx", "short", "ragged", "k10"])
def test_update_matches_reference_h256(case):
    """The product's own update kernels pinned to the reference's update() at
    H = 256 (tests/golden/capture_update_h256.py): "kx" B 8192 / mb 4096 (the
    32-row rowpass with k-packed planes and dw2_kx, the bench's path), "short"
    B 2048 / mb 512 (configs[3]'s per-rank minibatch, the 16-row rowpass),
    "ragged" B 4873 / mb 4096 (a kx minibatch and a 777-row tail).  1e-6
    absolute after 4 (short: 8) Adam steps that move a parameter by up to
    8e-4 (1.6e-3): 0.1 % of the update, 8x the measured worst (1.27e-7 on
    MI355X; the f32 sums in another order than torch's CPU ones -- on the CPU
    the same cases move by <= 8e-8 when fc1 is summed in f64 instead)."""
    run_reference_update(h256_case(case), atol=1e-6)


@pytest.mark.parametrize("case", ["cfg1", "short", "ragged", "k10"])
def test_update_matches_reference_h64_configs1(case):
    """The reference's own update() at H = 64 (tests/golden/capture_update_h256.py,
    update_h64.npz): "cfg1" B 8192 / mb 4096 (configs[1]'s minibatch: the
    rowpass with the dW2 product fused in, reduce, Adam), "short" mb 512,
    "ragged" B 4873 (a 777-row tail), two epochs each, through the drop-in
    PPO_continuous with the captured minibatch orders.  Bar 1e-6 absolute
    on every parameter after the update (f32 MFMA chains against the
    reference's CPU f32 GEMMs)."""
    run_reference_update(h64_case(case), atol=1e-6)


@pytest.mark.parametrize("H,split,mb", [(64, False, 512), (256, False, 512), (256, True, 512),
                                         (256, False, 777), (64, False, 100),
                                         (256, False, 4096), (64, False, 4096),
                                         (128, False, 512), (128, False, 100)])
def test_fused_step_vs_torch_autograd(H, split, mb):
    """The product's minibatch step (H 64: rowpass_dw2 + reduce + Adam; H 128:
    rowpass + dw2 + reduce + Adam; H 256:
    rowpass_kx + dw2_kx + reduce + Adam, 16-row blocks at mb <= 1024) vs plain
    torch fp32 autograd + clip_grad_norm_ + torch.optim.Adam on the same
    minibatch; mb 777 / 100 are ragged (the last BatchSampler minibatch with
    drop_last=False, a partial row block and split-K remainder); split: the
    actor and critic chains on two streams."""
    from satrl.ppo import PPOLearner
    from torch_reference import reference_step
    torch.manual_seed(11)
    args = _args(hidden_width=H, mini_batch_size=mb, batch_size=4096)
    L = PPOLearner(args, "pursuer", use_graph=False)
    with torch.no_grad():                      # non-trivial weights (reference init has mean_layer gain 0.01)
        for p in list(L.actor.parameters()) + list(L.critic.parameters()):
            p.add_(torch.randn_like(p) * 0.05)
    B = 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    src = torch.zeros((B, 32), device="cuda")
    src[:, 0:18] = torch.randn((B, 18), device="cuda", generator=g)
    src[:, 18:21] = torch.rand((B, 3), device="cuda", generator=g) * 3.2 - 1.6
    src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
    src[:, 24] = torch.randn(B, device="cuda", generator=g)
    src[:, 25] = torch.randn(B, device="cuda", generator=g) * 5
    idx = torch.randperm(B, device="cuda", generator=g)[:mb]
    grads, params = reference_step(L.actor, L.critic, src[idx], lr=args.lr_a)
    L.sync_w2t()
    from satrl.ppo import FusedMinibatch
    st = FusedMinibatch(L, mb, 1, use_graph=False, split_chains=split)
    st.step(src, idx)
    torch.cuda.synchronize()
    G = L.flat_views(L.G)
    P = L.flat_views(L.P)
    for k, ref in grads.items():
        got = G[k].reshape(ref.shape)
        scale = ref.abs().max().item() + 1e-12
        err = (got - ref).abs().max().item() / scale
        assert err < 2e-4, (k, err)
    for k, ref in params.items():
        got = P[k].reshape(ref.shape)
        assert torch.allclose(got, ref, rtol=1e-5, atol=2e-7), (k, (got - ref).abs().max().item())
    assert L.steps.cpu().tolist() == [1.0, 1.0]
    # Adam also refreshed the fc2 operand image (fc2.weight^T): bitwise the image of P
    from satrl.ppo import w2x_image
    assert torch.equal(L.W2T.view(torch.int32), w2x_image(L.P[:2 * H * H], H).view(torch.int32))
    assert torch.equal(L.w2t_f32(), L.P[:2 * H * H].view(2, H, H).transpose(1, 2))


def _packed_rows(B, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    src = torch.zeros((B, 32), device="cuda")
    src[:, 0:18] = torch.randn((B, 18), device="cuda", generator=g)
    src[:, 18:21] = torch.rand((B, 3), device="cuda", generator=g) * 3.2 - 1.6
    src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
    src[:, 24] = torch.randn(B, device="cuda", generator=g)
    src[:, 25] = torch.randn(B, device="cuda", generator=g) * 5
    return src, g


def _reference_epoch(actor, critic, src, perm, mb, lr, eps=1e-5):
    """BatchSampler(drop_last=False) minibatches of one epoch on plain torch
    fp32 modules with persistent Adam state (ppo_continuous.py:212-239)."""
    import copy
    from torch_reference import actor_loss, critic_loss
    actor, critic = copy.deepcopy(actor), copy.deepcopy(critic)
    for p in list(actor.parameters()) + list(critic.parameters()):
        p.data = p.data.contiguous().clone()
        p.requires_grad_(True)
    oa = torch.optim.Adam(actor.parameters(), lr=lr, eps=eps)
    oc = torch.optim.Adam(critic.parameters(), lr=lr, eps=eps)
    for k in range(0, perm.numel(), mb):
        rows = src[perm[k:k + mb]]
        s, a, lp, adv, vt = rows[:, 0:18], rows[:, 18:21], rows[:, 21:24], rows[:, 24:25], rows[:, 25:26]
        oa.zero_grad()
        actor_loss(actor, s, a, lp, adv, 0.1, 0.01).backward()
        torch.nn.utils.clip_grad_norm_(actor.parameters(), 0.5)
        oa.step()
        oc.zero_grad()
        critic_loss(critic, s, vt).backward()
        torch.nn.utils.clip_grad_norm_(critic.parameters(), 0.5)
        oc.step()
    params = {"actor." + n: p.detach().clone() for n, p in actor.named_parameters()}
    params.update({"critic." + n: p.detach().clone() for n, p in critic.named_parameters()})
    return params


@pytest.mark.parametrize("H,mb,B,graph", [(128, 1056, 2080, False), (64, 4128, 8192, False),
                                          (256, 4096, 4873, True), (64, 4096, 4873, True)])
def test_epoch_with_ragged_tail_vs_torch(H, mb, B, graph):
    """One epoch (full minibatches, graphed or eager, then the ragged
    BatchSampler tail) vs plain torch fp32 autograd + clip + Adam with
    persistent optimiser state.  (128, 1056, 2080) and (64, 4128, 8192) are
    shapes whose tail has more dW2 splits than the full minibatch (the p2
    slabs are sized for the largest split count)."""
    from satrl.ppo import PPOLearner
    torch.manual_seed(5)
    args = _args(hidden_width=H, mini_batch_size=mb, batch_size=B, K_epochs=1, use_lr_decay=False)
    L = PPOLearner(args, "pursuer", use_graph=graph, graph_group=1)
    with torch.no_grad():
        for p in list(L.actor.parameters()) + list(L.critic.parameters()):
            p.add_(torch.randn_like(p) * 0.05)
    src, g = _packed_rows(B, seed=1)
    perm = torch.randperm(B, device="cuda", generator=g)
    ref = _reference_epoch(L.actor, L.critic, src, perm, mb, args.lr_a)
    L.update_packed(src, 0, perms=[perm])
    torch.cuda.synchronize()
    P = L.flat_views(L.P)
    nsteps = -(-B // mb)
    for k, r in ref.items():
        got = P[k].reshape(r.shape)
        assert torch.allclose(got, r, rtol=1e-5, atol=2e-7 * nsteps), (k, (got - r).abs().max().item())
    assert L.steps.cpu().tolist() == [float(nsteps)] * 2


def test_lr_decay_is_clamped_at_the_budget():
    """ppo_continuous.py:244-250 with the engine's episode count past
    max_train_steps: lr stops at 0 instead of turning negative (a negative
    lr would make Adam ascend), and VecTrainer.train stops at the budget."""
    from satrl.ppo import PPOLearner
    from satrl.trainer import VecTrainer
    args = _args(hidden_width=64, max_train_steps=100)
    L = PPOLearner(args, "pursuer", use_graph=False)
    L.lr_decay(50)
    assert L.lr_now[0] == pytest.approx(1e-4, rel=1e-6)
    L.lr_decay(100)
    assert L.lr_now == (0.0, 0.0)
    L.lr_decay(10 ** 6)
    assert L.lr_now == (0.0, 0.0)
    args = _args(batch_size=64 * 32, mini_batch_size=512, hidden_width=64, K_epochs=1, num_envs=64, horizon=32,
                 max_episode_steps=10, seed=3, rollout_graph_chunk=8, update_graph_group=2, max_train_steps=300)
    tr = VecTrainer(args, flag=0, d_capture=15000.0)
    stats = tr.train(max_iterations=20)
    assert tr.budget_reached and len(stats) < 20
    assert tr.episodes >= 300
    la, lc = tr.learner.lr_now
    assert 0.0 <= la < args.lr_a and 0.0 <= lc < args.lr_c
    tr.update()                                   # one more update past the budget: lr 0, not negative
    assert tr.learner.lr_now == (0.0, 0.0)


def test_vec_trainer_iteration_and_determinism():
    from satrl.trainer import VecTrainer
    outs = []
    for _ in range(2):
        args = _args(batch_size=64 * 32, mini_batch_size=256, hidden_width=64, K_epochs=2, num_envs=64, horizon=32,
                     max_episode_steps=20, seed=3, rollout_graph_chunk=8, update_graph_group=4)
        tr = VecTrainer(args, flag=0, d_capture=15000.0)
        st = tr.iteration()
        st = tr.iteration()
        torch.cuda.synchronize()
        assert tr.env.check_errors() == 0
        outs.append((tr.buf.obs.clone(), tr.buf.rew.clone(), tr.buf.act.clone(),
                     [p.detach().clone() for p in tr.learner.actor.parameters()], st))
    (o1, r1, a1, p1, s1), (o2, r2, a2, p2, s2) = outs
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(a1, a2)
    for x, y in zip(p1, p2):
        assert torch.equal(x, y)
    assert s1[0] > 0           # episodes finished (max_episode_steps=20 < 64 steps)


def test_full_size_iteration_is_bitwise_reproducible():
    """BASELINE configs[2] as the bench runs it (16384 envs x 2048 steps,
    H 256, minibatch 4096, 10 epochs = 81 920 Adam steps through the update's
    graphs): two trainers from the same seed end the iteration with the same
    parameters, Adam moments and buffer bit for bit (no atomics, pinned dW2
    plan), and the update moved the parameters."""
    import gc
    from satrl.trainer import VecTrainer
    outs = []
    for _ in range(2):
        args = _args(batch_size=16384 * 2048, mini_batch_size=4096, hidden_width=256, K_epochs=10, num_envs=16384,
                     horizon=2048, max_episode_steps=1000, seed=11, rollout_graph_chunk=64, update_graph_group=64)
        tr = VecTrainer(args, flag=0, d_capture=15000.0)
        p0 = tr.learner.P.clone()
        st = tr.iteration()
        torch.cuda.synchronize()
        assert tr.env.check_errors() == 0
        outs.append((p0, tr.learner.P.clone(), tr.learner.M.clone(), tr.learner.V.clone(), tr.buf.rew.clone(), st))
        del tr
        gc.collect()
        torch.cuda.empty_cache()
    (p0a, pa, ma, va, ra, sa), (p0b, pb, mb_, vb, rb, sb) = outs
    assert torch.equal(p0a, p0b)
    assert torch.equal(pa, pb) and torch.equal(ma, mb_) and torch.equal(va, vb) and torch.equal(ra, rb)
    assert not torch.equal(pa, p0a) and torch.isfinite(pa).all()
    assert sa[0] > 0           # episodes finished (max_episode_steps 1000 < 2048 steps)


def test_vec_trainer_graph_vs_eager_rollout():
    from satrl.trainer import VecTrainer
    res = []
    for graphs in (True, False):
        args = _args(batch_size=32 * 24, mini_batch_size=128, hidden_width=64, K_epochs=1, num_envs=32, horizon=24,
                     max_episode_steps=10, seed=1, rollout_graph_chunk=8)
        tr = VecTrainer(args, flag=1, d_capture=15000.0, use_graphs=graphs)
        tr.collect()
        torch.cuda.synchronize()
        res.append((tr.buf.obs.clone(), tr.buf.rew.clone(), tr.buf.done.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_rowpass_contiguous_rows_match_gather():
    """satrl_ppo_rowpass with idx=NULL on pre-gathered rows == the indexed gather (bitwise)."""
    from satrl.ppo import PPOLearner
    torch.manual_seed(3)
    args = _args(hidden_width=128, mini_batch_size=1000, batch_size=8192)
    L = PPOLearner(args, "pursuer", use_graph=False)
    L.sync_w2t()
    g = torch.Generator(device="cuda").manual_seed(5)
    src = torch.randn((8192, 32), device="cuda", generator=g)
    idx = torch.randperm(8192, device="cuda", generator=g)[:1000]
    st = L.stepper(1000)
    outs = []
    for s_, i_ in ((src, idx), (src[idx].contiguous(), None)):
        # (slab slots past the launched blocks are never written: a finite
        # sentinel there, not torch.empty's bytes, which may hold NaNs)
        st.ptail.fill_(7.0)
        st.pw1.fill_(7.0)
        H1, dZ2 = st.rowpass(s_, i_)
        torch.cuda.synchronize()
        outs.append((H1.clone(), dZ2.clone(), st.ptail.clone(), st.pw1.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_short_rowpass_rows_match_long():
    """At H = 256 a minibatch of <= 1024 rows runs 16-row workgroups
    (rowpass_kernel<256, 16, 16>), a longer one 32-row workgroups; every
    row's arithmetic is the same, so tanh(fc1) (H1) of a 1024-row minibatch
    equals the first 1024 rows of a 1056-row one bit for bit, for both nets
    (the forward's later phases share this code; the fused-step tests at
    mb 512 / 777 / 100 check the short kernel's gradients against torch)."""
    from satrl.ppo import PPOLearner
    torch.manual_seed(8)
    args = _args(hidden_width=256, mini_batch_size=1024, batch_size=8192)
    L = PPOLearner(args, "pursuer", use_graph=False)
    L.sync_w2t()
    g = torch.Generator(device="cuda").manual_seed(9)
    src = torch.randn((1056, 32), device="cuda", generator=g)
    src[:, 21:24] = -1.0 - torch.rand((1056, 3), device="cuda", generator=g)
    H = 256
    h1 = {}
    for mb in (1024, 1056):
        H1, _ = L.stepper(mb).rowpass(src, None, mb)
        torch.cuda.synchronize()
        h1[mb] = H1.view(2, mb, H).clone()
    assert torch.equal(h1[1024], h1[1056][:, :1024])


def test_update_graph_groups_equal_eager():
    """FusedMinibatch.run: graph replays that walk the permutation through the
    device group counter (satrl_ppo_stage / satrl_ppo_group_advance), then
    the eager remainder groups and the ragged tail minibatch == the same epoch
    stepped eagerly, bitwise (parameters, Adam moments, step counters), over
    two epochs (the counter restarts per epoch)."""
    from satrl.ppo import PPOLearner
    mb, G = 256, 4
    B = (2 * G + 3) * mb + 17                      # 2 graph groups, 3 eager minibatches, a 17-row tail
    res = []
    for use_graph in (True, False):
        torch.manual_seed(11)
        args = _args(hidden_width=64, mini_batch_size=mb, batch_size=B)
        L = PPOLearner(args, "pursuer", graph_group=G, use_graph=use_graph)
        g = torch.Generator(device="cuda").manual_seed(2)
        src = torch.randn((B, 32), device="cuda", generator=g)
        src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
        perms = [torch.randperm(B, device="cuda", generator=g) for _ in range(2)]
        L.sync_w2t()
        st = L.stepper(mb)
        for p in perms:
            st.run(src, p)
        torch.cuda.synchronize()
        if use_graph:
            assert st.graph is not None and int(st.grp.item()) == 2
        res.append((L.P.clone(), L.M.clone(), L.V.clone(), L.steps.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("H,N", [(256, 1000), (256, 65536), (64, 4096), (64, 65536), (128, 1000)])
def test_policy_act_and_value_kernels(H, N):
    """satrl_policy_act / satrl_policy_value vs the torch modules + satrl_gaussian_sample
    (same Philox draw); every row independent of N and of its position (bitwise).
    N 65536: configs[3]'s total env count in one launch; H 64 at N 4096:
    configs[1]'s rollout kernels (policy_kernel<64, 4, 0/1>,
    ppo_continuous.py:61-101, 176-189)."""
    from satrl.ppo import PPOLearner, gaussian_sample, policy_act, policy_value
    torch.manual_seed(5)
    args = _args(hidden_width=H)
    Lp = PPOLearner(args, "pursuer", use_graph=False)
    Le = PPOLearner(args, "evader", use_graph=False)
    with torch.no_grad():
        for L in (Lp, Le):
            for p in list(L.actor.parameters()) + list(L.critic.parameters()):
                p.add_(torch.randn_like(p) * 0.05)
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randn((N, 18), device="cuda", generator=g)
    sb = torch.tensor([7], dtype=torch.int64, device="cuda")
    out = [torch.empty((N, 3), device="cuda") for _ in range(4)]
    policy_act(H, obs, Lp.P, Le.P, 1.6, 123, 4096, 5, *out, step_base=sb)
    with torch.no_grad():
        for k, L in enumerate((Lp, Le)):
            mean = L.actor(obs)
            a_ref, lp_ref = gaussian_sample(mean, L.actor.log_std, 1.6, 123, k, 4096, 5 + 7)
            assert torch.allclose(out[2 * k], a_ref, rtol=1e-5, atol=1e-5)
            assert torch.allclose(out[2 * k + 1], lp_ref, rtol=1e-4, atol=1e-4)
        v = torch.empty(N, device="cuda")
        policy_value(H, obs, Lp.P, v)
        assert torch.allclose(v, Lp.critic(obs).reshape(-1), rtol=1e-5, atol=1e-5)
    # rows are independent of N / position: a sub-block with the matching env offset
    sub = [torch.empty((37, 3), device="cuda") for _ in range(4)]
    policy_act(H, obs[100:137].contiguous(), Lp.P, Le.P, 1.6, 123, 4096 + 100, 5, *sub, step_base=sb)
    for a, b in zip(out, sub):
        assert torch.equal(a[100:137], b)
    v2 = torch.empty(37, device="cuda")
    policy_value(H, obs[100:137].contiguous(), Lp.P, v2)
    assert torch.equal(v[100:137], v2)


def test_self_play_alternates_learner_and_flag():
    """VecTrainer.self_play: phase 1 trains the pursuer under Flag 0, phase 2
    the evader under Flag 1 (every env restarted with Flag 1); the idle
    agent's parameters do not move."""
    from satrl.env import unpack_bits
    from satrl.trainer import VecTrainer
    args = _args(batch_size=64 * 16, mini_batch_size=256, hidden_width=64, K_epochs=1, num_envs=64, horizon=16,
                 max_episode_steps=12, seed=4, rollout_graph_chunk=8, update_graph_group=2)
    tr = VecTrainer(args, flag=0, d_capture=15000.0)
    p0 = tr.pursuer.P.clone(); e0 = tr.evader.P.clone()
    tr.self_play(1, 1)
    torch.cuda.synchronize()
    assert not torch.equal(tr.pursuer.P, p0) and torch.equal(tr.evader.P, e0)
    p1 = tr.pursuer.P.clone()
    tr.set_flag(1)
    _, i32 = tr.env.get_state()
    assert all(unpack_bits(int(b))["flag"] == 1 for b in i32[2].cpu().tolist())
    tr.iteration()
    torch.cuda.synchronize()
    assert torch.equal(tr.pursuer.P, p1) and not torch.equal(tr.evader.P, e0)
    _, i32 = tr.env.get_state()
    assert all(unpack_bits(int(b))["flag"] == 1 for b in i32[2].cpu().tolist())   # autoreset keeps Flag 1
    assert tr.env.check_errors() == 0
    stats = tr.self_play(2, 1)            # continues with Flag 1, then switches back to 0
    assert [f for f, _ in stats] == [1, 0] and tr.learner is tr.pursuer


@pytest.mark.parametrize("H,mb", [(64, 4096), (128, 1000), (256, 4096), (256, 777)])
def test_dw2_kernel_vs_torch(H, mb):
    """satrl_ppo_dw2 (split-K LDS-DMA MFMA kernel) summed over its slabs ==
    dZ2^T @ H1 per net in fp64, within f32 accumulation error."""
    from satrl import _lib
    g = torch.Generator(device="cuda").manual_seed(H + mb)
    H1 = torch.randn(2 * mb * H, device="cuda", generator=g)
    dZ2 = torch.randn(2 * mb * H, device="cuda", generator=g)
    S = _lib.lib().satrl_ppo_dw2_splits(H, mb)
    assert S >= 1
    p2 = torch.full((2 * S * H * H,), float("nan"), device="cuda")
    _lib.check(_lib.lib().satrl_ppo_dw2(H, mb, -1, S, _lib.ptr(H1), _lib.ptr(dZ2), _lib.ptr(p2), p2.numel(),
                                        _lib.stream_ptr()), "satrl_ppo_dw2")
    got = p2.view(2, S, H, H).double().sum(1)
    ref = torch.bmm(dZ2.view(2, mb, H).double().transpose(1, 2), H1.view(2, mb, H).double())
    err = (got - ref).abs().max().item()
    assert err <= 1e-5 * ref.abs().max().item() + 1e-4, err


@pytest.mark.parametrize("mb,contig", [(4096, True), (777, False), (256, True)])
def test_fused_dw2_rowpass_bitwise_equals_separate(mb, contig):
    """H 64 (configs[1]): satrl_ppo_rowpass_dw2 writes each 32-row block's
    dW2 partial out of LDS as split-K slab `row block` of p2 -- bitwise the
    slabs satrl_ppo_rowpass + satrl_ppo_dw2 write at S = the row-block count
    -- and the same [dW1|db1] / tail slabs, so the reduced G is bitwise the
    four-launch step's (ppo_continuous.py:227-239).  777: a ragged last
    block on the index-gather path; 4096 / 256: staged contiguous rows."""
    import satrl._lib as _L
    from satrl.ppo import PPOLearner
    torch.manual_seed(3)
    B = 8192
    args = _args(hidden_width=64, mini_batch_size=mb, batch_size=B)
    L = PPOLearner(args, "pursuer", use_graph=False)
    with torch.no_grad():
        for p in list(L.actor.parameters()) + list(L.critic.parameters()):
            p.add_(torch.randn_like(p) * 0.05)
    L.sync_w2t()
    g = torch.Generator(device="cuda").manual_seed(4)
    src = torch.randn((B, 32), device="cuda", generator=g)
    src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
    idx = None if contig else torch.randperm(B, device="cuda", generator=g)[:mb]
    st = L.stepper(mb)
    assert st.fused_dw2 and st.S == (mb + 31) // 32
    lib, sp, S = _L.lib(), _L.stream_ptr(), st.S
    outs = []
    for fused in (False, True):
        for b in (st.p2, st.ptail, st.pw1):
            b.fill_(float("nan"))
        if fused:
            st.rowpass_dw2(src, idx)
        else:
            H1, dZ2 = st.rowpass(src, idx)
            _L.check(lib.satrl_ppo_dw2(64, mb, -1, S, _L.ptr(H1), _L.ptr(dZ2), _L.ptr(st.p2), st.p2.numel(), sp),
                     "satrl_ppo_dw2")
        G = torch.full_like(L.G, float("nan"))
        nsq = torch.zeros_like(st.nsq[0])
        _L.check(lib.satrl_ppo_reduce(64, mb, -1, S, 3, _L.ptr(st.p2), st.p2.numel(), _L.ptr(st.pw1),
                                      _L.ptr(st.ptail), _L.ptr(G), _L.ptr(nsq), _L.ptr(L.steps), sp),
                 "satrl_ppo_reduce")
        torch.cuda.synchronize()
        outs.append([st.p2[:2 * S * 64 * 64].clone(), st.ptail[:S * (6 * 64 + 12)].clone(),
                     st.pw1[:S * 2 * 64 * 20].clone(), G, nsq])
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("H,mb", [(64, 4096), (256, 4096), (256, 512)])
def test_rollout_logp_equals_update_recomputation(H, mb):
    """The rollout's stored log-probs (policy_kernel, satrl_policy_act) are
    what the update's first recomputation gives, bit for bit: on the first
    minibatch of the first epoch, before any Adam step, every row's ratio
    exp(logp - logp_old) is exactly 1.0f (ppo_continuous.py:176-189 stores
    a_logprob, :216-220 recomputes it).  Both the staged-row and the
    index-gather paths of the rowpass; H 256 mb 512 runs the 16-row kernel."""
    from satrl.trainer import VecTrainer
    N, T = 1024, 16
    args = _args(batch_size=N * T, mini_batch_size=mb, hidden_width=H, K_epochs=1, num_envs=N, horizon=T,
                 max_episode_steps=12, seed=9, rollout_graph_chunk=8, update_graph_group=2)
    tr = VecTrainer(args, flag=0, d_capture=15000.0)
    tr.collect()
    tr.compute_advantages()
    perm = tr.epoch_perm()
    L = tr.learner
    L.sync_w2t()
    st = L.stepper(mb)
    idx = perm[:mb].contiguous()
    staged = tr.buf.packed[idx].contiguous()
    for src, ix in ((tr.buf.packed, idx), (staged, None)):
        ratio = torch.full((mb,), float("nan"), device="cuda")
        st.rowpass_ratio(src, ix, ratio)
        torch.cuda.synchronize()
        bad = (ratio != 1.0).nonzero().reshape(-1)
        assert bad.numel() == 0, (bad[:8].tolist(), ratio[bad[:8]].tolist())




@pytest.mark.parametrize("mb,contig", [(4096, True), (1500, False), (512, True), (777, False), (520, True),
                                       (288, True), (100, False)])
def test_kx_rowpass_planes_and_dw2(mb, contig):
    """H 256: satrl_ppo_rowpass_kx writes H1 / dZ2 as k-packed bf16 planes
    whose sum hi + mid + lo is bitwise the f32 rowpass's H1 / dZ2 (rows past
    the minibatch zero), with the same [dW1|db1] / tail slabs; satrl_ppo_dw2_kx
    sums dZ2^T H1 from them on the split-bf16 MFMA within the f32 bound of an
    f64 reference (ppo_continuous.py:227-233: fc2.weight.grad).  1500: a ragged
    last chunk on the index-gather path.  512 / 777 / 520: the 16-row rowpass
    (configs[3]'s per-rank minibatch, ragged tails), whose last block zero-fills
    the padded half of its 32-row chunk (777: rows 784-799, 520: 528-543).
    Every size up to 1024 runs the column-split kernel (four workgroups per
    row block and net exchanging partials inside the launch; 288: a last
    window of 32 blocks with whole groups past the grid, 100: index gather,
    a ragged block); its exchange reports no timeout."""
    import satrl._lib as _L
    from satrl.ppo import PPOLearner
    torch.manual_seed(5)
    H, B = 256, 8192
    args = _args(hidden_width=H, mini_batch_size=mb, batch_size=B)
    L = PPOLearner(args, "pursuer", use_graph=False)
    with torch.no_grad():
        for p in list(L.actor.parameters()) + list(L.critic.parameters()):
            p.add_(torch.randn_like(p) * 0.05)
    L.sync_w2t()
    g = torch.Generator(device="cuda").manual_seed(6)
    src = torch.randn((B, 32), device="cuda", generator=g)
    src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
    idx = None if contig else torch.randperm(B, device="cuda", generator=g)[:mb]
    st = L.stepper(mb)
    assert st.kx(mb)
    # (slab slots past the launched blocks are never written: a finite sentinel
    # there, not torch.empty's bytes, which may hold NaNs that compare unequal)
    st.ptail.fill_(7.0)
    st.pw1.fill_(7.0)
    H1, dZ2 = st.rowpass(src, idx)
    torch.cuda.synchronize()
    H1, dZ2 = H1.clone().view(2, mb, H), dZ2.clone().view(2, mb, H)
    tail, w1 = st.ptail.clone(), st.pw1.clone()
    st.H1x.fill_(-1)
    st.dZ2x.fill_(-1)
    st.ptail.fill_(7.0)
    st.pw1.fill_(7.0)
    st.rowpass_kx(src, idx)
    torch.cuda.synchronize()
    assert torch.equal(st.ptail, tail) and torch.equal(st.pw1, w1)
    rows = (mb + 31) // 32 * 32

    def decode(x):
        p = x.view(2, 3, rows // 8, H, 8).view(torch.bfloat16).float()
        v = (p[:, 0] + p[:, 1]) + p[:, 2]                           # [2][rows/8][H][8]
        return v.permute(0, 1, 3, 2).reshape(2, rows, H)
    h1x, dz2x = decode(st.H1x), decode(st.dZ2x)
    assert torch.equal(h1x[:, :mb], H1) and torch.equal(dz2x[:, :mb], dZ2)
    assert not h1x[:, mb:].any() and not dz2x[:, mb:].any()
    S = st.S
    st.p2.fill_(float("nan"))
    st.dw2_kx(mb, S)
    torch.cuda.synchronize()
    got = st.p2[:2 * S * H * H].view(2, S, H, H).double().sum(1)
    ref = torch.einsum("brn,brm->bnm", dZ2.double(), H1.double())
    mag = torch.einsum("brn,brm->bnm", dZ2.double().abs(), H1.double().abs())
    err = ((got - ref).abs() / mag.clamp_min(1e-30)).max().item()
    assert err < 2e-6, err                 # per-slab split-bf16 sums (<= 2.2e-7 each) + f32 slab rounding
    from satrl.ppo import rowpass_exchange_check
    rowpass_exchange_check()               # raises if a column-split exchange timed out


def test_column_split_exchange_timeout_is_reported():
    """The column-split rowpass's bounded wait (ppo_kernels.hip cs_handoff):
    a group whose exchange counter breaks its invariant (fault injection:
    satrl_ppo_rowpass_fault_inject) waits out its 0.5 s timeout and the
    launch still ends; satrl_ppo_rowpass_error then reports it (the learner
    raises) and re-arms the exchange, and the next launch's outputs are
    bitwise a clean launch's."""
    import time
    import satrl._lib as _L
    from satrl.ppo import PPOLearner, rowpass_exchange_check
    torch.manual_seed(5)
    H, B, mb = 256, 8192, 512
    args = _args(hidden_width=H, mini_batch_size=mb, batch_size=B)
    L = PPOLearner(args, "pursuer", use_graph=False)
    L.sync_w2t()
    g = torch.Generator(device="cuda").manual_seed(6)
    src = torch.randn((B, 32), device="cuda", generator=g)
    src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
    st = L.stepper(mb)
    rowpass_exchange_check()
    for t in (st.ptail, st.pw1):                  # (finite slots past the launched blocks)
        t.fill_(7.0)
    st.rowpass_kx(src, None)
    torch.cuda.synchronize()
    ref = [t.clone() for t in (st.H1x, st.dZ2x, st.ptail, st.pw1)]
    # group 0's counter at 5: its four workgroups pass the first hand-off but
    # wait for 16 at the second while the counter stops at 13
    assert _L.lib().satrl_ppo_rowpass_fault_inject(0, 5, _L.stream_ptr()) == 0
    t0 = time.time()
    st.rowpass_kx(src, None)
    torch.cuda.synchronize()
    assert time.time() - t0 < 10.0
    with pytest.raises(RuntimeError, match="timed out"):
        rowpass_exchange_check()
    rowpass_exchange_check()                      # re-armed: no error left
    for t in (st.ptail, st.pw1):
        t.fill_(7.0)
    st.rowpass_kx(src, None)
    torch.cuda.synchronize()
    rowpass_exchange_check()
    for a, b in zip((st.H1x, st.dZ2x, st.ptail, st.pw1), ref):
        assert torch.equal(a, b)


def test_exchange_check_is_bounded_by_its_deadline():
    """satrl_ppo_rowpass_error waits for the stream against a host deadline:
    behind a kernel that outlasts it the call raises (-2, "did not drain")
    instead of blocking -- the DP learner's guard against a stream stuck
    behind a dead peer's collective -- and the next call works."""
    import satrl._lib as _L
    from satrl.ppo import rowpass_exchange_check
    rowpass_exchange_check()
    torch.cuda._sleep(int(1e9))                   # a spin kernel of well over 10 ms
    with pytest.raises(_L.NativeError, match="did not drain"):
        rowpass_exchange_check(timeout_s=0.01)
    torch.cuda.synchronize()
    rowpass_exchange_check(timeout_s=5.0)


@pytest.mark.parametrize("mb,net", [(4096, -1), (777, -1), (100, -1), (4096, 0), (512, 0)])
def test_dw2_kx_w1_equals_dw2_kx_then_reduce(mb, net):
    """satrl_ppo_dw2_kx_w1 (the reduce's W1 / tail regions inside the dW2
    launch) + satrl_ppo_reduce(mode | 4) writes bitwise the slabs, G, norm
    pairs and step counters of satrl_ppo_dw2_kx + satrl_ppo_reduce(mode), for
    mode 3 and mode 1 (the data-parallel sum)."""
    import ctypes as C
    import satrl._lib as _L
    from satrl.ppo import PPOLearner
    from satrl._lib import ptr
    torch.manual_seed(5)
    H, B = 256, 8192
    args = _args(hidden_width=H, mini_batch_size=mb, batch_size=B)
    L = PPOLearner(args, "pursuer", use_graph=False)
    L.sync_w2t()
    g = torch.Generator(device="cuda").manual_seed(6)
    src = torch.randn((B, 32), device="cuda", generator=g)
    src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
    st = L.stepper(mb)
    st.rowpass_kx(src, None, mb, net)
    lib, sp = _L.lib(), _L.stream_ptr()
    S = lib.satrl_ppo_dw2_kx_splits(H, mb, net)
    assert S >= 1 and (1 if net == 0 else 2) * S * H * H <= st.p2.numel()     # (net 0: the first half)
    nsq = st.nsq[0]

    def run(fused, mode):
        st.p2.fill_(float("nan"))
        L.G.fill_(float("nan"))
        nsq.fill_(float("nan"))
        L.steps.zero_()
        if fused:
            assert lib.satrl_ppo_dw2_kx_w1(H, mb, net, S, ptr(st.H1x), ptr(st.dZ2x), st.H1x.numel(), ptr(st.p2),
                                           st.p2.numel(), mode, ptr(st.pw1), ptr(st.ptail), ptr(L.G),
                                           ptr(nsq) if mode & 2 else None, sp) == 0
        else:
            assert lib.satrl_ppo_dw2_kx(H, mb, net, S, ptr(st.H1x), ptr(st.dZ2x), st.H1x.numel(), ptr(st.p2),
                                        st.p2.numel(), sp) == 0
        assert lib.satrl_ppo_reduce(H, mb, net, S, mode | (4 if fused else 0), ptr(st.p2), st.p2.numel(),
                                    ptr(st.pw1), ptr(st.ptail), ptr(L.G), ptr(nsq) if mode & 2 else None,
                                    ptr(L.steps) if mode & 2 else None, sp) == 0
        torch.cuda.synchronize()
        return [t.clone() for t in (st.p2, L.G, nsq, L.steps)]

    for mode in (3, 1):
        ref, got = run(False, mode), run(True, mode)
        for a, b in zip(ref, got):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64),
                               b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int64))
        if net < 0:
            assert not torch.isnan(got[1]).any()          # every region of G written
