"""The f64 reference of the minibatch step (torch_reference.reference_step_f64)
and the constructed inputs of test_ppo_small_gpu.py (ppo_cases.py), checked on
the CPU before a GPU sees them: the reference against the two f32 statements
the project already trusts (torch_reference.reference_step and the host
drop-in's HostLearner._minibatch), and every input builder against the
condition its GPU test relies on."""
import pytest
import torch

import ppo_cases as pc
from torch_reference import reference_full, reference_step, reference_step_f64

WIDTHS = (64, 128, 256)


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("mb", (1, 17, 100))
def test_f64_reference_vs_f32_statements(H, mb):
    """reference_step_f64 vs f32 reference_step and HostLearner._minibatch
    (ppo_continuous.py:216-239 on torch's CPU autograd) on the same rows.

    Gradients: per tensor max |g32 - g64| / max |g64| <= (H + mb + 32) * 2^-24,
    the first-order bound of an f32 sum as long as the longest chain behind
    any gradient element (H terms of a hidden-layer dot product, mb rows, the
    18 + 3 + small terms of the thin layers), taken against the tensor's
    largest element.  Parameters after clip + Adam: rtol 1e-5 / atol 2e-7, the
    suite's tolerance for this quantity (test_fused_step_vs_torch_autograd).
    reference_full in f32 restates the forward layer by layer to tap the fc2
    pre-activation: its gradients are reference_step's bit for bit."""
    from satrl.ppo import HostLearner
    actor, critic = pc.cpu_nets(H)
    rows = pc.packed_rows(256, seed=3)[torch.randperm(256, generator=torch.Generator().manual_seed(mb))[:mb]]
    ref = reference_step_f64(actor, critic, rows, lr=2e-4)
    g32, p32 = reference_step(actor, critic, rows, lr=2e-4)
    r32 = reference_full(actor, critic, rows, lr=2e-4, dtype=torch.float32)
    host = HostLearner(pc.make_args(H, mb), "pursuer")
    host.actor.load_state_dict(actor.state_dict())
    host.critic.load_state_dict(critic.state_dict())
    host._minibatch(rows)
    hostp = {"actor." + n: p.detach() for n, p in host.actor.named_parameters()}
    hostp.update({"critic." + n: p.detach() for n, p in host.critic.named_parameters()})
    assert set(ref.grads) == set(g32) == set(hostp)
    bound = (H + mb + 32) * 2.0 ** -24
    for k, g64 in ref.grads.items():
        assert g64.dtype == torch.float64
        assert torch.equal(r32.grads[k], g32[k]), k
        e32 = pc.rel_err(g32[k], g64)
        assert e32 <= bound, (k, e32, bound)
        for name, p in (("reference_step", p32[k]), ("HostLearner", hostp[k])):
            assert torch.allclose(p.double(), ref.params[k], rtol=1e-5, atol=2e-7), (name, k)
    # the per-row taps are the quantities their names say
    s = rows[:, 0:18].double()
    for n, net in enumerate((actor, critic)):
        h1 = torch.tanh(s @ net.fc1.weight.double().T + net.fc1.bias.double())
        assert torch.allclose(ref.H1[n], h1, rtol=0, atol=1e-14)
        # dW2 = dZ2^T H1 and db2 = sum of the dZ2 rows
        name = ("actor", "critic")[n]
        assert torch.allclose(ref.dZ2[n].T @ ref.H1[n], ref.grads[name + ".fc2.weight"], rtol=1e-12, atol=1e-15)
        assert torch.allclose(ref.dZ2[n].sum(0), ref.grads[name + ".fc2.bias"], rtol=1e-12, atol=1e-15)
    assert ref.H1.shape == ref.dZ2.shape == (2, mb, H) and ref.ratio.shape == (mb,)
    assert pc.rel_err(r32.dZ2, ref.dZ2) <= bound


def test_f64_reference_clip_switch_and_steps():
    """clip=False leaves the gradients alone; nsteps continues one Adam state."""
    actor, critic = pc.cpu_nets(64)
    rows = pc.packed_rows(40, seed=5)
    on = reference_step_f64(actor, critic, rows)
    off = reference_step_f64(actor, critic, rows, clip=False)
    assert on.norms["actor"] > 0.5 and on.norms["critic"] > 0.5          # random rows: both clipped
    assert all(torch.equal(on.grads[k], off.grads[k]) for k in on.grads)
    assert any(not torch.equal(on.params[k], off.params[k]) for k in on.params)
    three = reference_step_f64(actor, critic, rows, nsteps=3)
    assert all(torch.equal(on.grads[k], three.grads[k]) for k in on.grads)
    moved = [float((three.params[k] - on.params[k]).abs().max()) for k in on.params]
    assert min(moved) > 0.0 and max(moved) < 2 * 2e-4 * 1.2              # about lr per step and element


@pytest.mark.parametrize("H", WIDTHS)
def test_critic_kappa_stays_small(H):
    """ppo_cases.critic_kappa on the contiguous rows test_small_minibatch_gradients
    steps: 1 for the actor, at least 1 for the critic, and never so large that
    the bar's floor 2^-20 * kappa stops meaning f32 accuracy (<= 32: 3e-5)."""
    actor, critic = pc.cpu_nets(H)
    src = pc.packed_rows(256, seed=7)
    for mb in (1, 2, 15, 16, 17, 31, 32, 33, 47, 65):
        ref = reference_step_f64(actor, critic, src[:mb])
        assert ref.v_mag.shape == ref.v_diff.shape == (mb,)
        assert torch.allclose(ref.v_diff, ref.v - src[:mb, 25].double(), rtol=0, atol=1e-15)
        for k in ref.grads:
            kappa = pc.critic_kappa(ref, k)
            assert kappa == 1.0 if k.startswith("actor.") else 1.0 <= kappa <= 32.0, (mb, k, kappa)
        assert pc.bar(0.0, 4.0) == 4 * pc.bar(0.0) == 2.0 ** -18 and pc.bar(1e-3, 4.0) == 8e-3


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("case", pc.CLIP_CASES)
def test_clip_rows_are_on_their_sides(H, case):
    """ppo_cases.clip_rows: each net's unclipped f64 norm is at least a factor
    2 from max_norm 0.5 on the intended side, for three consecutive steps'
    first gradient (the later steps move the parameters by <= 3 lr)."""
    actor, critic = pc.cpu_nets(H)
    rows = pc.clip_rows(actor, critic, case)
    norms = reference_step_f64(actor, critic, rows).norms
    assert pc.clip_sides(case, norms), (case, norms)
    assert rows.shape == (33, 32) and bool((rows[:, 26:] == pc.SENTINEL).all())
    assert bool(torch.isfinite(rows).all())


@pytest.mark.parametrize("H", WIDTHS)
def test_branch_rows_meet_their_margins(H):
    """ppo_cases.branch_rows: the f64 reference's ratio of every constructed
    row is the intended one (f32 rounding of the stored log-probs apart), at
    least 1e-3 from the clip edges 0.9 / 1.1; every (ratio, adv) combination
    and both tie signs are present; the rows whose surrogate gradient must
    vanish have an exactly zero f64 dZ2 row, every other row a non-zero one."""
    actor, critic = pc.cpu_nets(H)
    rows, want, adv = pc.branch_rows(actor, critic)
    ref = reference_step_f64(actor, critic, rows, epsilon=pc.EPSILON)
    assert torch.allclose(ref.ratio, want, rtol=1e-5, atol=0)
    assert pc.branch_margin(ref.ratio) >= 1e-3
    seen = {(round(float(r), 2), float(a)) for r, a in zip(want[:24], adv[:24])}
    assert seen == {(r, a) for r in pc.BRANCH_RATIOS for a in pc.BRANCH_ADVS}
    assert sorted(adv[24:].tolist()) == [-1.0] * 4 + [1.0] * 4 and bool((want[24:] == 1).all())
    zero = pc.grad_zero_rows(want, adv)
    assert int(zero.sum()) == 2 * (2 + 4) and not bool(zero[24:].any())
    dz = ref.dZ2[0]
    assert bool((dz[zero] == 0).all())
    assert bool((dz[~zero].abs().max(1).values > 0).all())
    assert bool((rows[:, 26:] == pc.SENTINEL).all())
