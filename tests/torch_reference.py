"""Plain PyTorch references of the PPO minibatch step
(ppo_continuous.py:216-239), used only to check the fused HIP kernels:
reference_step in fp32 (the measuring stick of what an f32 chain loses) and
reference_step_f64 in fp64 on the CPU, with the per-row intermediates the
rowpass hands to the dW2 product."""
import copy
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F


def actor_loss(actor, s, a, lp_old, adv, epsilon, entropy_coef):
    mean = actor(s)
    std = torch.exp(actor.log_std.expand_as(mean))
    dist = torch.distributions.Normal(mean, std, validate_args=False)
    dist_entropy = dist.entropy().sum(1, keepdim=True)
    a_logprob_now = dist.log_prob(a)
    ratios = torch.exp(a_logprob_now.sum(1, keepdim=True) - lp_old.sum(1, keepdim=True))
    surr1 = ratios * adv
    surr2 = torch.clamp(ratios, 1 - epsilon, 1 + epsilon) * adv
    return (-torch.min(surr1, surr2) - entropy_coef * dist_entropy).mean()


def critic_loss(critic, s, vt):
    return F.mse_loss(vt, critic(s))


def reference_step(actor, critic, rows, epsilon=0.1, entropy_coef=0.01, lr=2e-4, eps=1e-5, clip=True):
    """One reference minibatch step on copies of the modules; returns
    (grads dict, params-after dict) keyed like PPOLearner.flat_views."""
    actor = copy.deepcopy(actor)
    critic = copy.deepcopy(critic)
    for p in list(actor.parameters()) + list(critic.parameters()):
        p.data = p.data.contiguous().clone()
        p.requires_grad_(True)
    s, a, lp, adv, vt = rows[:, 0:18], rows[:, 18:21], rows[:, 21:24], rows[:, 24:25], rows[:, 25:26]
    oa = torch.optim.Adam(actor.parameters(), lr=lr, eps=eps)
    oc = torch.optim.Adam(critic.parameters(), lr=lr, eps=eps)
    oa.zero_grad()
    actor_loss(actor, s, a, lp, adv, epsilon, entropy_coef).backward()
    grads = {"actor." + n: p.grad.detach().clone() for n, p in actor.named_parameters()}
    if clip:
        torch.nn.utils.clip_grad_norm_(actor.parameters(), 0.5)
    oa.step()
    oc.zero_grad()
    critic_loss(critic, s, vt).backward()
    grads.update({"critic." + n: p.grad.detach().clone() for n, p in critic.named_parameters()})
    if clip:
        torch.nn.utils.clip_grad_norm_(critic.parameters(), 0.5)
    oc.step()
    params = {"actor." + n: p.detach().clone() for n, p in actor.named_parameters()}
    params.update({"critic." + n: p.detach().clone() for n, p in critic.named_parameters()})
    return grads, params


def _forward_taps(net, s, actor):
    """net(s) restated layer by layer (Actor_Gaussian / Critic.forward), with
    H1 = tanh(fc1(s)) and the fc2 pre-activation z2 kept for retain_grad."""
    h1 = net.activate_func(net.fc1(s))
    z2 = net.fc2(h1)
    h2 = net.activate_func(z2)
    out = net.max_action * torch.tanh(net.mean_layer(h2)) if actor else net.fc3(h2)
    return out, h1, z2


def reference_full(actor, critic, rows, epsilon=0.1, entropy_coef=0.01, lr=2e-4, eps=1e-5, clip=True, nsteps=1,
                   dtype=torch.float64):
    """`nsteps` consecutive minibatch steps on the same rows, on `dtype` CPU
    copies of the modules (the losses of actor_loss / critic_loss, then
    clip_grad_norm_(0.5) where `clip`, then Adam(eps), all in `dtype`).
    Returns a namespace; everything but `params` is the first step's:
      grads   {name: tensor} keyed like PPOLearner.flat_views
      norms   {"actor": float, "critic": float}, the unclipped gradient norms
      H1      [2][mb][H]  tanh(fc1(s)) per net (actor, critic) and row
      dZ2     [2][mb][H]  d loss / d (fc2 pre-activation) per net and row
      ratio   [mb]        the actor's exp(logp(a|s) - logp_old)
      logp    [mb][3]     the actor's per-dimension log-prob of the row's action
      v       [mb]        the critic's value; v_diff = v - v_target; v_mag = the
                          magnitudes the subtraction's operands are summed from,
                          sum_k |fc3.weight[k] h2[k]| + |fc3.bias| + |v_target|
      params {name: tensor} after the last step"""
    nets = []
    for net in (actor, critic):
        net = copy.deepcopy(net).to("cpu")
        for p in net.parameters():
            p.data = p.data.to(dtype).contiguous().clone()
            p.requires_grad_(True)
        nets.append(net)
    actor, critic = nets
    rows = rows.detach().to("cpu", dtype)
    s, a, lp, adv, vt = rows[:, 0:18], rows[:, 18:21], rows[:, 21:24], rows[:, 24:25], rows[:, 25:26]
    oa = torch.optim.Adam(actor.parameters(), lr=lr, eps=eps)
    oc = torch.optim.Adam(critic.parameters(), lr=lr, eps=eps)
    out = SimpleNamespace()
    for step in range(nsteps):
        oa.zero_grad()
        mean, h1a, z2a = _forward_taps(actor, s, True)
        z2a.retain_grad()
        std = torch.exp(actor.log_std.expand_as(mean))
        dist = torch.distributions.Normal(mean, std, validate_args=False)
        dist_entropy = dist.entropy().sum(1, keepdim=True)               # (actor_loss's order of operations)
        logp = dist.log_prob(a)
        ratios = torch.exp(logp.sum(1, keepdim=True) - lp.sum(1, keepdim=True))
        surr1 = ratios * adv
        surr2 = torch.clamp(ratios, 1 - epsilon, 1 + epsilon) * adv
        (-torch.min(surr1, surr2) - entropy_coef * dist_entropy).mean().backward()
        oc.zero_grad()
        v, h1c, z2c = _forward_taps(critic, s, False)
        z2c.retain_grad()
        F.mse_loss(vt, v).backward()
        if step == 0:
            out.grads = {"actor." + n: p.grad.detach().clone() for n, p in actor.named_parameters()}
            out.grads.update({"critic." + n: p.grad.detach().clone() for n, p in critic.named_parameters()})
            out.norms = {k: math.sqrt(sum(float((g.double() ** 2).sum()) for n, g in out.grads.items()
                                          if n.startswith(k + "."))) for k in ("actor", "critic")}
            out.H1 = torch.stack([h1a.detach(), h1c.detach()])
            out.dZ2 = torch.stack([z2a.grad.detach().clone(), z2c.grad.detach().clone()])
            out.ratio = ratios.detach().reshape(-1).clone()
            out.logp = logp.detach().clone()
            with torch.no_grad():
                out.v = v.detach().reshape(-1).clone()
                out.v_mag = ((torch.tanh(z2c).abs() @ critic.fc3.weight.abs().T).reshape(-1)
                             + critic.fc3.bias.abs() + vt.reshape(-1).abs())
                out.v_diff = (v - vt).detach().reshape(-1).clone()
        for net, opt in ((actor, oa), (critic, oc)):
            if clip:
                torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
            opt.step()
    out.params = {"actor." + n: p.detach().clone() for n, p in actor.named_parameters()}
    out.params.update({"critic." + n: p.detach().clone() for n, p in critic.named_parameters()})
    return out


def reference_step_f64(actor, critic, rows, **kw):
    """reference_full in fp64: what the kernels are measured against."""
    return reference_full(actor, critic, rows, dtype=torch.float64, **kw)
