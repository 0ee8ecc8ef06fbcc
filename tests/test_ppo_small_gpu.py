"""The minibatch step (rowpass, dW2, reduce, Adam; ppo_continuous.py:213-239)
against an f64 reference at the smallest minibatches and every hidden width.

Inputs come from ppo_cases.py (checked on the CPU by
test_ppo_reference_cpu.py); the unused columns 26..31 of every packed row hold
1e30, so a kernel that read them would show it.

The bar of every gradient and dZ2 comparison (ppo_cases.bar): per tensor
err = max |got - ref64| / max |ref64|, measured against e32, the same quantity
of the f32 torch reference on the same inputs, and bounded by
max(8 * e32, 2^-20): 8x what torch's own f32 chain loses (another summation
order, the 2-ulp tanh), and never below 16 f32 ulps of the tensor's largest
element (at one or two rows e32 is an ulp or zero).  Each case prints err, e32
and err / bar.

One loosening, for the critic's gradient tensors (not its dZ2 rows), with its
error analysis in ppo_cases.critic_kappa: the floor is 2^-20 * kappa, kappa
the condition number of the loss head's v - v_target.  Every critic gradient
is linear in the rows' (2 / mb)(v_r - vt_r); the f32 rounding of v_r scales
with the magnitudes its 256-term (H-term) sum adds up, A_r = 3.7 .. 5 here,
not with the difference, so where one or two rows have v_r near vt_r, 16 ulps
of the gradient's largest element are far less than 16 ulps of what was
rounded.  Found at H 256, 2 contiguous rows (v - vt = +0.62, -0.25; fc3.bias
gradient 0.374 from operands summing to 10.1 in magnitude, kappa 27; the other
critic tensors kappa 8.9): the kernel's v_0 is off by 3.9e-7 = 1.7 f32 ulps
of A_0 (the 1-row case, where that factor is common to every critic tensor),
torch's own f32 v_0 by 2.2e-8, so the plain bar stood at 1.0e-6 and the
kernel's fc3.bias / fc2.bias gradients at 1.32e-6 / 1.30e-6 of their largest
element.  kappa comes from the f64 reference alone (never from a kernel's
output): 1.2 .. 1.3 from 15 rows on, 3 .. 9 at one or two rows, and 5 .. 10
for the one-element fc3.bias at every size (a sum of random signs)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ppo_cases as pc
from torch_reference import reference_full, reference_step_f64

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256)
SMALL_MBS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 65)


def _restore(L, P0):
    """The learner back at its initial parameters, Adam state and counters;
    G poisoned so that an element the step does not write shows."""
    L.P.copy_(P0)
    L.M.zero_()
    L.V.zero_()
    L.steps.zero_()
    L.G.fill_(float("nan"))
    L.sync_w2t()


def _refs(actor, critic, rows, **kw):
    """The f64 reference and the f32 measuring stick of one minibatch."""
    return (reference_step_f64(actor, critic, rows, **kw),
            reference_full(actor, critic, rows, dtype=torch.float32, **kw))


def _compare(tag, got, ref64, ref32, bad, kappa=1.0):
    """One bar-rule comparison: prints the figures, records a miss in `bad`,
    returns err / bar."""
    err, e32 = pc.rel_err(got, ref64), pc.rel_err(ref32, ref64)
    bar = pc.bar(e32, kappa)
    print(f"{tag}: err {err:.3e} e32 {e32:.3e} err/e32 {err / e32 if e32 else float('inf'):.2f} "
          f"kappa {kappa:.2f} err/bar {err / bar:.3f}")
    if not err <= bar:
        bad.append((tag, err, e32, bar))
    return err / bar


def _check_grads(tag, views, ref, r32, bad, names=None):
    worst = 0.0
    for k in (ref.grads if names is None else names):
        worst = max(worst, _compare(f"{tag} {k}", views[k], ref.grads[k], r32.grads[k], bad,
                                    pc.critic_kappa(ref, k)))
    return worst


def _check_pads(L, buf, tag):
    """The layout's pad elements (W1 column 19, b3a[3], ls[3], b3c[1:4]) are
    exactly zero."""
    H, o = L.H, L.off
    W1 = buf[o["W1"]:o["W1"] + 2 * H * 20].view(2, H, 20)
    pads = torch.cat([W1[:, :, 19].reshape(-1), buf[o["b3a"] + 3:o["b3a"] + 4], buf[o["ls"] + 3:o["ls"] + 4],
                      buf[o["b3c"] + 1:o["b3c"] + 4]])
    assert bool((pads == 0).all()), (tag, pads[pads != 0][:8].tolist())


@pytest.mark.parametrize("H", WIDTHS)
def test_small_minibatch_gradients(H):
    """Every tensor of G after one product-path step (FusedMinibatch.step: H 64
    rowpass_dw2, H 128 rowpass + dw2, H 256 rowpass_kx + dw2_kx_w1 + reduce
    with mode bit 4 on the column-split kernel) against the f64 gradients, at
    1 .. 65 rows: one partial row block, a plane chunk padded from 1 row,
    split-K with one chunk, a column-split window with 8 live workgroups,
    inv_mb = 1, one live lane in the loss head's row sums.  Index gather from
    256 rows and contiguous rows; the ragged-tail path as FusedMinibatch.run
    takes it (a stepper sized for 64 / 4096 rows stepping 1 and 17); at H 256
    also split_chains (per-net launches: the 16-row kernel without the column
    split).  Pads of G exactly zero, one step counted per net.
    Bar: the module's bar rule (critic tensors with kappa).  Measured on
    MI355X, worst err / bar: H 64 0.39, H 128 0.39, H 256 0.63 (actor
    mean_layer.bias, 17-row tail of a 4096-row stepper; without kappa H 256
    reached 1.39, the module docstring's case).  Worst err / e32 where the
    bar is 8 e32 (the floor below it): 1.6 (H 256, 17 rows gathered, critic
    fc1.bias, err 1.8e-6); where the floor holds, e32 is down to 3e-9 and the
    ratio says little (up to 52, H 64 fc3.bias, err 1.5e-7)."""
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check, step_plan
    L, actor, critic = pc.gpu_learner(H)
    P0 = L.P.clone()
    B = 256
    src_c = pc.packed_rows(B, seed=7)
    src = src_c.cuda()
    g = torch.Generator().manual_seed(H)
    cases = []
    for mb in SMALL_MBS:
        st = FusedMinibatch(L, mb, 1, use_graph=False)
        assert (st.fused_dw2, st.kx_on) == (H == 64, H == 256)
        plan = step_plan(H, mb)                          # the buffers are the library's plan
        assert (st.p2.numel(), st.ptail.numel(), st.pw1.numel()) == (plan.p2_floats, plan.ptail_floats, plan.pw1_floats)
        assert (st.S, st.p2_splits) == (plan.splits, plan.max_splits)
        cases.append((f"mb {mb} gather", st, mb, torch.randperm(B, generator=g)[:mb]))
        cases.append((f"mb {mb} contiguous", st, mb, None))
    for cap in (64, 4096):
        st = FusedMinibatch(L, cap, 1, use_graph=False)
        for t in (1, 17):
            cases.append((f"tail {t} of {cap}", st, t, torch.randperm(B, generator=g)[:t]))
    if H == 256:
        for mb in (1, 17):
            st = FusedMinibatch(L, mb, 1, use_graph=False, split_chains=True)
            assert st.split
            cases.append((f"mb {mb} split chains", st, mb, torch.randperm(B, generator=g)[:mb]))
    bad, worst = [], 0.0
    for tag, st, mb, idx in cases:
        rows = src_c[:mb] if idx is None else src_c[idx]
        ref, r32 = _refs(actor, critic, rows)
        _restore(L, P0)
        st.step(src, None if idx is None else idx.cuda(), mb=mb)
        torch.cuda.synchronize()
        worst = max(worst, _check_grads(f"H {H} {tag}", L.flat_views(L.G), ref, r32, bad))
        assert not bool(torch.isnan(L.G).any()), tag              # every element of G written
        _check_pads(L, L.G, tag)
        assert L.steps.cpu().tolist() == [1.0, 1.0], tag
    if H == 256:
        rowpass_exchange_check()
    print(f"H {H}: worst err / bar {worst:.3f}")
    assert not bad, bad


def _slab_sums(L, st, nrb):
    """The rowpass's [dW1|db1] and tail slabs of the nrb launched row blocks
    summed in f64 into a flat gradient image (W2 left zero)."""
    H, o = L.H, L.off
    flat = torch.zeros(o["total"], dtype=torch.float64, device=st.ptail.device)
    flat[o["W1"]:o["W1"] + 2 * H * 20] = st.pw1.view(-1, 2 * H * 20)[:nrb].double().sum(0)
    flat[o["b2"]:o["total"]] = st.ptail.view(-1, 6 * H + 12)[:nrb].double().sum(0)
    return flat


@pytest.mark.parametrize("H", WIDTHS)
def test_rowpass_rows_vs_f64(H):
    """satrl_ppo_rowpass's per-row outputs at 1, 17 and 33 rows (gather and
    contiguous) against the f64 reference, row by row:
      H1 = tanh(fc1(s)), element (r, n): |err| <= 2^-24 * (20 * sum_i |W1[n,i]|
        |s[r,i]| + |b1[n]| + 3): the 19-term f32 sum's first-order bound
        (19 roundings, rounded up to 20, on the magnitudes summed, evaluated
        in f64 from the inputs; tanh' <= 1 carries it through), plus
        TANH_MAX_ULP = 2 and the final rounding of a value of at most 1;
      dZ2 = d loss / d (fc2 pre-activation): the bar rule, per net;
      the [dW1|db1] and tail slabs of the launched row blocks, summed: the bar
        rule against the f64 gradients (every tensor but fc2.weight), pads 0.
    Slab slots past the launched blocks and H1 / dZ2 elements past 2 * mb * H
    (the stepper is sized for 128 rows) keep their sentinel.  At H 256 the
    k-packed launch (satrl_ppo_rowpass_kx) at 1 and 17 rows: its decoded
    planes are the f32 rows bit for bit, zero in the padded rows of the last
    32-row chunk, the same slabs, nothing written past the planes.
    Measured on MI355X, worst err / bar (dZ2, slabs): H 64 0.22, H 128 0.84
    (actor mean_layer.bias slabs, 17 rows gathered: err 8.0e-7, e32 9.8e-8,
    err / e32 8.2 under the floor), H 256 0.22; worst H1 error / bound: 0.09,
    0.12, 0.11."""
    import satrl._lib as _L
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check
    L, actor, critic = pc.gpu_learner(H)
    B, cap = 256, 128
    src_c = pc.packed_rows(B, seed=8)
    src = src_c.cuda()
    st = FusedMinibatch(L, cap, 1, use_graph=False)
    g = torch.Generator().manual_seed(100 + H)
    bad, worst, worst_h1 = [], 0.0, 0.0
    names = [k for k in L.flat_views(L.G) if not k.endswith("fc2.weight")]
    for mb in (1, 17, 33):
        for idx in (torch.randperm(B, generator=g)[:mb], None):
            tag = f"H {H} mb {mb} {'contiguous' if idx is None else 'gather'}"
            rows = src_c[:mb] if idx is None else src_c[idx]
            idx_d = None if idx is None else idx.cuda()
            ref, r32 = _refs(actor, critic, rows)
            for t in (st.H1, st.dZ2, st.ptail, st.pw1):
                t.fill_(7.0)
            st.rowpass(src, idx_d, mb)
            torch.cuda.synchronize()
            n = 2 * mb * H
            H1, dZ2 = st.H1[:n].view(2, mb, H).cpu(), st.dZ2[:n].view(2, mb, H).cpu()
            assert bool((st.H1[n:] == 7.0).all()) and bool((st.dZ2[n:] == 7.0).all()), tag
            nrb = _L.lib().satrl_ppo_row_blocks(H, mb)
            assert 1 <= nrb < st.nwg
            tail, w1 = st.ptail.clone(), st.pw1.clone()
            assert bool((tail.view(-1, 6 * H + 12)[nrb:] == 7.0).all()), tag
            assert bool((w1.view(-1, 2 * H * 20)[nrb:] == 7.0).all()), tag
            s = rows[:, 0:18].double()
            for k, net in enumerate((actor, critic)):
                mag = s.abs() @ net.fc1.weight.detach().double().abs().T
                bound = 2.0 ** -24 * (20.0 * mag + net.fc1.bias.detach().double().abs() + 3.0)
                q = float(((H1[k].double() - ref.H1[k]).abs() / bound).max())
                print(f"{tag} H1 net {k}: worst error / bound {q:.3f}")
                worst_h1 = max(worst_h1, q)
                if not q <= 1.0:
                    bad.append((tag, "H1", k, q))
                worst = max(worst, _compare(f"{tag} dZ2 net {k}", dZ2[k], ref.dZ2[k], r32.dZ2[k], bad))
            flat = _slab_sums(L, st, nrb)
            worst = max(worst, _check_grads(tag + " slabs", L.flat_views(flat), ref, r32, bad, names))
            _check_pads(L, flat, tag)
            if H == 256 and mb in (1, 17):
                st.H1x.fill_(-1)
                st.dZ2x.fill_(-1)
                st.ptail.fill_(7.0)
                st.pw1.fill_(7.0)
                st.rowpass_kx(src, idx_d, mb)
                torch.cuda.synchronize()
                assert torch.equal(st.ptail, tail) and torch.equal(st.pw1, w1), tag
                rp = (mb + 31) // 32 * 32
                ne = 2 * 3 * rp * H
                assert ne == _L.lib().satrl_ppo_kx_elems(H, mb)

                def decode(x):
                    p = x[:ne].view(2, 3, rp // 8, H, 8).view(torch.bfloat16).float()
                    v = (p[:, 0] + p[:, 1]) + p[:, 2]
                    return v.permute(0, 1, 3, 2).reshape(2, rp, H).cpu()
                h1x, dz2x = decode(st.H1x), decode(st.dZ2x)
                assert torch.equal(h1x[:, :mb], H1) and torch.equal(dz2x[:, :mb], dZ2), tag
                assert not bool(h1x[:, mb:].any()) and not bool(dz2x[:, mb:].any()), tag
                assert bool((st.H1x[ne:] == -1).all()) and bool((st.dZ2x[ne:] == -1).all()), tag
    if H == 256:
        rowpass_exchange_check()
    print(f"H {H}: worst err / bar {worst:.3f}, worst H1 error / bound {worst_h1:.3f}")
    assert not bad, bad


@pytest.mark.parametrize("H", WIDTHS)
def test_both_sides_of_the_gradient_clip(H):
    """Three consecutive steps on a 33-row minibatch whose f64 gradient norms
    lie on chosen sides of clip_grad_norm_'s max_norm 0.5 (ppo_cases.clip_rows:
    actor below / critic above, the reverse, both below; asserted here from
    the f64 reference, each norm a factor 2 or more from 0.5), with the clip
    on and with use_grad_clip off, against f64 clip + Adam.  Below 0.5 the
    clip coefficient is exactly 1; a coefficient applied unclamped would scale
    those gradients by 5, which moves every element whose |g| is within a few
    hundred Adam eps by far more than the tolerance.
    Tolerance: the suite's for parameters after Adam steps
    (test_fused_step_vs_torch_autograd / test_epoch_with_ragged_tail_vs_torch):
    rtol 1e-5, atol 2e-7 * nsteps.  Worst |dP| / (atol + rtol |P|) measured on
    MI355X: H 64 0.08, H 128 0.06, H 256 0.30."""
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check
    L, actor, critic = pc.gpu_learner(H, mb=33)
    P0 = L.P.clone()
    st = FusedMinibatch(L, 33, 1, use_graph=False)
    nsteps, worst, bad = 3, 0.0, []
    for case in pc.CLIP_CASES:
        rows = pc.clip_rows(actor, critic, case)
        src = rows.cuda()
        for clip in (True, False):
            ref = reference_step_f64(actor, critic, rows, lr=L.lr_a, clip=clip, nsteps=nsteps)
            assert pc.clip_sides(case, ref.norms), (case, ref.norms)
            _restore(L, P0)
            L.use_grad_clip = clip
            for _ in range(nsteps):
                st.step(src, None)
            torch.cuda.synchronize()
            P = L.flat_views(L.P)
            for k, r in ref.params.items():
                got = P[k].reshape(r.shape).double().cpu()
                q = float(((got - r).abs() / (2e-7 * nsteps + 1e-5 * r.abs())).max())
                worst = max(worst, q)
                print(f"H {H} {case} clip {clip} {k}: |dP| / tolerance {q:.3f}")
                if not q <= 1.0:
                    bad.append((case, clip, k, q))
            assert L.steps.cpu().tolist() == [float(nsteps)] * 2
    if H == 256:
        rowpass_exchange_check()
    print(f"H {H}: worst |dP| / tolerance {worst:.3f}")
    assert not bad, bad


@pytest.mark.parametrize("H", WIDTHS)
def test_loss_head_branches(H):
    """The loss head's branches on one constructed 32-row minibatch
    (ppo_cases.branch_rows, epsilon 0.1): ratio in {0.5, 0.95, 1.05, 2.0} x
    adv in {-1, 0, +1}, placed through the old log-probs from the f64
    reference's own log-prob, and eight tie rows whose actions and log-probs
    come from satrl_policy_act on the same parameters (ratio exactly 1.0f,
    so surr1 == surr2), adv of both signs.  Asserted here from the f64
    reference: every ratio at least 1e-3 from the clip edges 0.9 / 1.1.
      ratio (satrl_ppo_rowpass_ratio) matches f64 to 1e-5 relative, and is
        exactly 1.0f on the tie rows;
      the actor's dZ2 row == 0 where the surrogate gradient vanishes (ratio 2
        with adv > 0, ratio 0.5 with adv < 0, adv = 0);
      every other actor row, and the tie rows on their own (the full gradient,
        g1 + g2 * inside = 1): the bar rule against f64;
      the log_std gradient (entropy term on every row): the bar rule.
    Measured on MI355X: ratio within 4.2e-7 / 5.1e-7 / 5.6e-7 of f64 (H 64 /
    128 / 256); worst err / bar 0.23 / 0.13 / 0.29, worst err / e32 1.9 / 1.1
    / 2.7 (log_std)."""
    import satrl._lib as _L
    from satrl.ppo import FusedMinibatch, policy_act, rowpass_exchange_check
    L, actor, critic = pc.gpu_learner(H, mb=32)
    assert float(L.epsilon) == pc.EPSILON
    n, nt = 32, pc.N_TIE
    rows0, _, _ = pc.branch_rows(actor, critic)
    obs = rows0[n - nt:, 0:18].cuda().contiguous()
    act, lp = torch.empty((nt, 3), device="cuda"), torch.empty((nt, 3), device="cuda")
    policy_act(H, obs, L.P, None, L.max_action, 5, 0, 0, act, lp)
    torch.cuda.synchronize()
    rows, want, adv = pc.branch_rows(actor, critic, tie=(act, lp))
    assert torch.equal(rows[:, 0:18], rows0[:, 0:18])
    ref, r32 = _refs(actor, critic, rows, epsilon=pc.EPSILON)
    assert torch.allclose(ref.ratio, want, rtol=1e-5, atol=0), (ref.ratio / want - 1).abs().max()
    assert pc.branch_margin(ref.ratio) >= 1e-3
    zero = pc.grad_zero_rows(want, adv)
    assert int(zero.sum()) == 12 and not bool(zero[n - nt:].any())
    assert bool((ref.dZ2[0][zero] == 0).all()) and bool((ref.dZ2[0][~zero].abs().max(1).values > 0).all())
    st = FusedMinibatch(L, n, 1, use_graph=False)
    ratio = torch.full((n,), float("nan"), device="cuda")
    for t in (st.ptail, st.pw1):
        t.fill_(7.0)
    st.rowpass_ratio(rows.cuda(), None, ratio)
    torch.cuda.synchronize()
    ratio = ratio.cpu()
    q = float((ratio.double() / ref.ratio - 1).abs().max())
    print(f"H {H}: ratio worst relative error {q:.3e}")
    assert q <= 1e-5, q
    assert bool((ratio[n - nt:] == 1.0).all()), ratio[n - nt:].tolist()
    dZ2 = st.dZ2[:2 * n * H].view(2, n, H).cpu()
    assert bool((dZ2[0][zero] == 0).all()), (dZ2[0][zero] != 0).any(1).nonzero().reshape(-1).tolist()
    bad = []
    tie = torch.zeros(n, dtype=torch.bool)
    tie[n - nt:] = True
    worst = 0.0
    for what, sel in (("rows with a gradient", ~zero), ("tie rows", tie)):
        worst = max(worst, _compare(f"H {H} actor dZ2, {what}", dZ2[0][sel], ref.dZ2[0][sel], r32.dZ2[0][sel], bad))
    worst = max(worst, _compare(f"H {H} critic dZ2", dZ2[1], ref.dZ2[1], r32.dZ2[1], bad))
    flat = _slab_sums(L, st, _L.lib().satrl_ppo_row_blocks(H, n))
    worst = max(worst, _check_grads(f"H {H} slabs", L.flat_views(flat), ref, r32, bad, ["actor.log_std"]))
    if H == 256:
        rowpass_exchange_check()
    print(f"H {H}: worst err / bar {worst:.3f}")
    assert not bad, bad


def _critic_mask(o, H):
    """True on the critic's elements of the flat layout (net_of in
    ppo_kernels.hip: pads belong to the net of their segment)."""
    e = torch.arange(o["total"])
    return torch.where(e < o["W1"], e >= H * H,
                       torch.where(e < o["b2"], e - o["W1"] >= H * 20,
                                   torch.where(e < o["W3a"], e - o["b2"] >= H, e >= o["W3c"])))


def test_adam_kernel_alone():
    """satrl_ppo_adam on controlled flat buffers (H 64, direct C-ABI call):
    random G and M, random V >= 0 (a tenth of the elements with |g| near Adam's
    eps), zero pads, the norm partials written by hand so that one net's norm
    is 0.2 (coef exactly 1) and the other's 3 (coef 0.5 / 3.000001), the step
    counters set to k in {1, 2, 1000, bct_len - 1, bct_len, bct_len + 5}
    (adam_bias_table ends where both factors are exactly 1.0; past it the
    kernel uses 1.0), with and without use_clip, both nets and one net alone.

    Reference: _single_tensor_adam in f64,
        g' = g coef;  m' = m + (1 - b1)(g' - m);  v' = b2 v + (1 - b2) g'^2;
        p' = p - (lr / bc1) m' / (sqrt(v') / bc2s + eps),
    coef = min(0.5 / (norm + 1e-6), 1), (bc1, bc2s) = adam_bias_table[k] or
    (1, 1) past it; b1, b2, eps, lr and 1e-6 are the f32 values the C ABI
    carries (b2 = f32(0.999) = 0.99900001287: the kernel's 1 - b2 is exact in
    f32 and is its weight of g'^2, so each moment stays an average with
    weights summing to 1; torch's f32 Adam multiplies by f32(0.999) and adds
    f32(1 - 0.999) = 0.001 g'^2, a V increment 1.3e-5 larger, which moves p'
    by 6e-6 of a step: inside the parameter tolerances, outside this bound,
    hence the betas as carried).

    Bound, from the roundings of adam_elem (u = 2^-24 per f32 operation,
    -ffp-contract=off; first order, times 1.01):
      g' = g coef: f32(norm), + 1e-6, the division, the product: |dg'| <= c |g'|,
        c = 4u (c = 0 where coef is clamped to 1.0f or use_clip is off)
      m': g' - m (u), w1 * (u), m + (u)          -> E_m = u (|m'| + 2 w1 |g' - m|) + c w1 |g'|
      v': g'g' (2c + u), w2 * (u), v b2 (u), + (u)
                                                 -> E_v = u (|v'| + b2 v + 2 w2 g'^2) + 2c w2 g'^2
      denom: sqrt (E_v / 2v' + u), / f32(bc2s) (2u), + eps (u)
                                                 -> E_d = (sqrt(v')/bc2s)(E_v / 2v' + 3u) + u denom
      q = m' / denom (u)                         -> E_q = |q| (E_d / denom + u) + E_m / denom
      step = f32(lr / bc1) q (2u)                -> E_s = 2u |step| + (lr / bc1) E_q
      p' = p + step (u)                          -> E_p = u |p'| + E_s
    i.e. half an ulp of p' plus a few ulps of the step.
    Bitwise: lr = 0 leaves P unchanged; pad elements (g = m = v = p = 0) stay
    0 in P, M and V; a one-net call leaves the other net's P, M, V and W2X
    untouched; W2X is w2x_image(P') afterwards.
    Worst error / bound measured on MI355X: P' 0.98, M' 0.95, V' 0.95 (the
    half-ulp terms are attained)."""
    import satrl._lib as _L
    from satrl.ppo import PPOLearner, adam_bias_table, ppo_layout, w2x_floats, w2x_image
    H, mb = 64, 64
    lib, sp = _L.lib(), _L.stream_ptr()
    o = ppo_layout(H)
    total, HH = o["total"], H * H
    shell = SimpleNamespace(H=H, off=o)
    used = torch.zeros(total)
    for v in PPOLearner.flat_views(shell, used).values():
        v.fill_(1.0)
    pad = used == 0
    assert int(pad.sum()) == 2 * H + 1 + 1 + 3
    crit = _critic_mask(o, H)
    nblk = C.c_int64()
    assert lib.satrl_ppo_sizes(H, mb, None, C.byref(nblk)) == 0 and nblk.value >= 3
    bct = adam_bias_table(0.9, 0.999)
    n_bct = bct.shape[0]
    assert bct[-1].tolist() == [1.0, 1.0] and bct[-2].tolist() != [1.0, 1.0]
    bct_d = bct.cuda()
    f32 = lambda x: float(np.float32(x))
    b1, b2, eps, tiny = f32(0.9), f32(0.999), f32(1e-5), f32(1e-6)
    w1, w2 = 1.0 - b1, 1.0 - b2
    assert f32(w1) == w1 and f32(w2) == w2
    u = 2.0 ** -24
    g = torch.Generator().manual_seed(17)
    G = torch.randn(total, generator=g) * 1e-2
    small = torch.rand(total, generator=g) < 0.1
    G[small] *= 1e-3                                                    # |g| ~ eps: the eps term matters
    M = torch.randn(total, generator=g) * 1e-2
    V = torch.rand(total, generator=g) * 1e-4
    P = torch.randn(total, generator=g) * 0.1
    for t in (G, M, V, P):
        t[pad] = 0.0
    ks = [1, 2, 1000, n_bct - 1, n_bct, n_bct + 5]
    worst = {"P": 0.0, "M": 0.0, "V": 0.0}
    bad = []
    runs = [(ka, ks[(i + 3) % 6], 1, -1, (0.2, 3.0) if i % 2 == 0 else (3.0, 0.2), (2e-4, 1e-4))
            for i, ka in enumerate(ks)]
    runs += [(2, 1000, 0, -1, (3.0, 3.0), (2e-4, 1e-4)),                # use_clip off: coef 1 at any norm
             (1000, 2, 1, 0, (3.0, 0.2), (2e-4, 1e-4)),                 # the actor alone
             (2, n_bct, 1, 1, (0.2, 3.0), (2e-4, 1e-4)),                # the critic alone
             (3, 7, 1, -1, (3.0, 0.2), (0.0, 0.0))]                     # lr 0
    for ka, kc, use_clip, net, norms, lrs in runs:
        tag = f"k ({ka}, {kc}) clip {use_clip} net {net} norms {norms} lr {lrs}"
        nsq = torch.zeros((nblk.value, 2), dtype=torch.float64)
        for j, f in enumerate((0.5, 0.3, 0.2)):                          # three partials per net
            nsq[j, 0], nsq[j, 1] = f * norms[0] ** 2, f * norms[1] ** 2
        steps = torch.tensor([float(ka), float(kc)], dtype=torch.float64)
        lr = torch.tensor(lrs, dtype=torch.float32)
        d = [t.clone().cuda() for t in (G, P, M, V)]
        W2X = torch.full((w2x_floats(H),), 3.0, device="cuda")
        nsq_d, steps_d, lr_d = nsq.cuda(), steps.cuda(), lr.cuda()
        assert lib.satrl_ppo_adam(H, mb, net, _L.ptr(nsq_d), _L.ptr(steps_d), _L.ptr(bct_d), n_bct, _L.ptr(lr_d),
                                  b1, b2, eps, 0.5, use_clip, _L.ptr(d[0]), _L.ptr(d[1]), _L.ptr(d[2]), _L.ptr(d[3]),
                                  _L.ptr(W2X), sp) == 0, tag
        torch.cuda.synchronize()
        Pn, Mn, Vn = (t.cpu() for t in d[1:])
        assert torch.equal(d[0].cpu(), G) and torch.equal(steps_d.cpu(), steps), tag     # inputs untouched
        # the f64 statement, per element with its net's constants
        sel = lambda a, c: torch.where(crit, torch.tensor(c, dtype=torch.float64), torch.tensor(a, dtype=torch.float64))
        nrm = [float(nsq[:, j].sum().sqrt()) for j in (0, 1)]
        coefs = [min(0.5 / (x + tiny), 1.0) if use_clip else 1.0 for x in nrm]
        bc = [bct[k].tolist() if k < n_bct else [1.0, 1.0] for k in (ka, kc)]
        coef, bc1, bc2s = sel(*coefs), sel(bc[0][0], bc[1][0]), sel(bc[0][1], bc[1][1])
        ss = sel(float(lr[0]), float(lr[1])) / bc1
        g64, m64, v64, p64 = G.double(), M.double(), V.double(), P.double()
        gc = g64 * coef
        m1 = m64 + w1 * (gc - m64)
        v1 = b2 * v64 + w2 * gc * gc
        den = v1.sqrt() / bc2s + eps
        q = m1 / den
        step = ss * q
        p1 = p64 - step
        cu = (coef < 1.0).double() * 4.0 * u                             # c: the clamped coef (1.0f) is exact
        E_m = u * (m1.abs() + 2 * w1 * (gc - m64).abs()) + w1 * cu * gc.abs()
        E_v = u * (v1.abs() + b2 * v64 + 2 * w2 * gc * gc) + w2 * 2 * cu * gc * gc
        E_d = (v1.sqrt() / bc2s) * 3 * u + E_v / (2 * v1.sqrt()).clamp_min(1e-300) / bc2s + u * den
        E_q = q.abs() * (E_d / den + u) + E_m / den
        E_s = 2 * u * step.abs() + ss * E_q
        E_p = u * p1.abs() + E_s
        live = torch.ones(total, dtype=torch.bool) if net < 0 else (crit == bool(net))
        for name, got, ref, E, old in (("P", Pn, p1, E_p, P), ("M", Mn, m1, E_m, M), ("V", Vn, v1, E_v, V)):
            assert torch.equal(got[~live], old[~live]), (tag, name)      # the other net untouched, bitwise
            assert bool((got[pad] == 0).all()), (tag, name)
            err, bound = (got.double() - ref).abs()[live & ~pad], 1.01 * E[live & ~pad]
            qq = float((err / bound).max())
            worst[name] = max(worst[name], qq)
            print(f"{tag} {name}': worst error / bound {qq:.3f}")
            if not bool((err <= bound).all()):
                bad.append((tag, name, qq))
        if lrs == (0.0, 0.0):
            assert torch.equal(Pn, P), tag
        img, W2Xc = w2x_image(Pn[:2 * HH], H), W2X.cpu()
        for k in (0, 1):
            want = img[k * HH:(k + 1) * HH] if net < 0 or net == k else torch.full((HH,), 3.0)
            assert torch.equal(W2Xc[k * HH:(k + 1) * HH].view(torch.int32), want.view(torch.int32)), (tag, k)
    print(f"worst error / bound: {worst}")
    assert not bad, bad
