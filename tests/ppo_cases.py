"""Constructed inputs of the minibatch-step tests (test_ppo_reference_cpu.py
checks them with the f64 reference alone, test_ppo_small_gpu.py feeds them to
the kernels): networks, packed rows with a sentinel in the unused columns, the
minibatches on either side of the gradient clip and the loss-head branch rows.
Everything is built on the CPU from seeded generators, so both files see the
same numbers."""
import math

import torch

from torch_reference import reference_step_f64

SENTINEL = 1e30                       # columns 26..31 of a packed row: never read by a kernel
EPSILON = 0.1                         # the PPO clip range (args_param default)
BRANCH_RATIOS = (0.5, 0.95, 1.05, 2.0)
BRANCH_ADVS = (-1.0, 0.0, 1.0)
N_TIE = 8                             # tie rows of the branch minibatch (rows 24..31)


def make_args(H, mb=64, B=4096, **kw):
    from satrl.trainer import args_param
    a = args_param(chkpt_dir="/tmp", hidden_width=H, mini_batch_size=mb, batch_size=B, **kw)
    a.state_dim, a.action_dim, a.max_action = 18, 3, 1.6
    return a


def _noise(nets, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=g) * 0.05 for net in nets for p in net.parameters()]


def cpu_nets(H, seed=11):
    """(actor, critic) f32 on the CPU: the reference init from torch's global
    generator (actor first), every weight perturbed by randn * 0.05 (the
    reference init has mean_layer gain 0.01)."""
    from satrl.ppo import Actor_Gaussian, Critic
    torch.manual_seed(seed)
    args = make_args(H)
    nets = (Actor_Gaussian(args, "pursuer"), Critic(args, "pursuer"))
    with torch.no_grad():
        for p, n in zip([p for net in nets for p in net.parameters()], _noise(nets, seed + 1)):
            p.add_(n)
    return nets


def gpu_learner(H, mb=64, B=4096, seed=11):
    """A PPOLearner whose weights are cpu_nets(H, seed)'s bit for bit, and
    those nets."""
    from satrl.ppo import PPOLearner
    torch.manual_seed(seed)
    L = PPOLearner(make_args(H, mb, B), "pursuer", use_graph=False)
    nets = (L.actor, L.critic)
    with torch.no_grad():
        for p, n in zip([p for net in nets for p in net.parameters()], _noise(nets, seed + 1)):
            p.add_(n.to(p.device))
    L.sync_w2t()
    actor, critic = cpu_nets(H, seed)
    for a, b in zip(list(L.actor.parameters()) + list(L.critic.parameters()),
                    list(actor.parameters()) + list(critic.parameters())):
        assert torch.equal(a.detach().cpu(), b.detach())
    return L, actor, critic


def packed_rows(B, seed=0):
    """Packed transition rows [B][32] f32 on the CPU: s(18) a(3) logp(3) adv
    v_target, and SENTINEL in the six unused columns."""
    g = torch.Generator().manual_seed(seed)
    src = torch.full((B, 32), SENTINEL)
    src[:, 0:18] = torch.randn((B, 18), generator=g)
    src[:, 18:21] = torch.rand((B, 3), generator=g) * 3.2 - 1.6
    src[:, 21:24] = -1.0 - torch.rand((B, 3), generator=g)
    src[:, 24] = torch.randn(B, generator=g)
    src[:, 25] = torch.randn(B, generator=g) * 5
    return src


def _near_policy_rows(actor, critic, mb, seed):
    """Rows whose actions lie within 1.5 std of the actor's mean and whose old
    log-probs are the actor's own (ratio 1 up to rounding), adv ~ N(0, 1),
    v_target = the critic's value + N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.full((mb, 32), SENTINEL)
    rows[:, 0:18] = torch.randn((mb, 18), generator=g)
    with torch.no_grad():
        mean = actor(rows[:, 0:18])
        std = torch.exp(actor.log_std.detach()).expand_as(mean)
        rows[:, 18:21] = mean + std * (torch.rand((mb, 3), generator=g) * 3.0 - 1.5)
        rows[:, 24] = torch.randn(mb, generator=g)
        rows[:, 25] = critic(rows[:, 0:18]).reshape(-1) + torch.randn(mb, generator=g)
    rows[:, 21:24] = 0.0
    ref = reference_step_f64(actor, critic, rows)
    rows[:, 21:24] = ref.logp.float()
    return rows


CLIP_CASES = ("actor_below", "critic_below", "both_below")
CLIP_LOW, CLIP_HIGH = 0.1, 2.0        # target norms either side of max_norm 0.5


def clip_rows(actor, critic, case, mb=33, seed=21):
    """A minibatch on a chosen side of clip_grad_norm_(0.5) for each net:
    "actor_below": actor norm < 0.5 < critic norm; "critic_below": the
    reverse; "both_below".  The critic's gradient is linear in v_target - v,
    the actor's in adv apart from the entropy term, so the rows of
    _near_policy_rows are scaled to the target norms CLIP_LOW / CLIP_HIGH
    (the old log-probs a little off the actor's own, so ratios differ from 1).
    The caller asserts clip_sides(case, norms) on the f64 reference."""
    rows = _near_policy_rows(actor, critic, mb, seed)
    g = torch.Generator().manual_seed(seed + 1)
    rows[:, 21:24] += 0.02 * torch.randn((mb, 3), generator=g)
    with torch.no_grad():
        v = critic(rows[:, 0:18]).reshape(-1)
    n0 = reference_step_f64(actor, critic, rows).norms
    ta = CLIP_LOW if case in ("actor_below", "both_below") else CLIP_HIGH
    tc = CLIP_LOW if case in ("critic_below", "both_below") else CLIP_HIGH
    rows[:, 24] *= ta / n0["actor"]
    rows[:, 25] = v + (rows[:, 25] - v) * (tc / n0["critic"])
    return rows


def clip_sides(case, norms):
    """True when each net's unclipped norm is at least a factor 2 away from
    max_norm 0.5 on the side `case` names."""
    want_a = case in ("actor_below", "both_below")
    want_c = case in ("critic_below", "both_below")
    ok_a = norms["actor"] < 0.25 if want_a else norms["actor"] > 1.0
    ok_c = norms["critic"] < 0.25 if want_c else norms["critic"] > 1.0
    return ok_a and ok_c


def branch_rows(actor, critic, seed=31, tie=None):
    """The 32-row loss-head minibatch.  Rows 0..23: every (ratio, adv) of
    BRANCH_RATIOS x BRANCH_ADVS twice, the ratio placed by setting the old
    log-probs to the f64 reference's own log-prob minus log(ratio) / 3 per
    dimension.  Rows 24..31 (tie rows): adv +1 / -1 alternating; `tie` =
    (actions [8][3], log-probs [8][3]) as the rollout kernel produced them for
    these rows' states (ratio exactly 1.0f in the kernels), None = the
    reference's own log-probs of near-mean actions.
    Returns (rows, want_ratio [32] f64, adv [32])."""
    n = 32
    rows = _near_policy_rows(actor, critic, n, seed)
    combos = [(r, a) for r in BRANCH_RATIOS for a in BRANCH_ADVS] * 2
    want = torch.ones(n, dtype=torch.float64)
    for k, (r, a) in enumerate(combos):
        want[k] = r
        rows[k, 24] = a
    for k in range(len(combos), n):
        rows[k, 24] = 1.0 if k % 2 == 0 else -1.0
    if tie is not None:
        rows[n - N_TIE:, 18:21] = tie[0].detach().cpu()
    rows[:, 21:24] = 0.0
    logp = reference_step_f64(actor, critic, rows).logp                  # f64 [32][3]
    rows[:, 21:24] = (logp - (want.log() / 3.0)[:, None]).float()
    if tie is not None:
        rows[n - N_TIE:, 21:24] = tie[1].detach().cpu()
    return rows, want, rows[:, 24].clone()


def branch_margin(ratio):
    """Smallest distance of the ratios from the clip edges 1 -+ EPSILON."""
    r = ratio.double()
    return float(torch.minimum((r - (1 - EPSILON)).abs(), (r - (1 + EPSILON)).abs()).min())


def grad_zero_rows(want_ratio, adv):
    """Rows whose surrogate gradient vanishes: clipped on the side torch.min
    selects (ratio above 1 + eps with adv > 0, below 1 - eps with adv < 0),
    and every adv = 0 row."""
    return ((want_ratio > 1 + EPSILON) & (adv > 0)) | ((want_ratio < 1 - EPSILON) & (adv < 0)) | (adv == 0)


def bar(e32, kappa=1.0):
    """The gradient / dZ2 bar: 8 x the f32 torch reference's own error, at
    least 16 f32 ulps of the tensor's largest element (times kappa >= 1, the
    condition number of a subtraction the tensor is proportional to:
    critic_kappa)."""
    return max(8.0 * e32, 2.0 ** -20 * max(kappa, 1.0))


def critic_kappa(ref, name):
    """The factor by which the bar's floor understates f32 rounding for a
    critic gradient tensor at a handful of rows.  Every critic gradient element
    is linear in the rows' d mse / d v = (2 / mb)(v_r - vt_r), and any f32
    evaluation of v_r (torch's as much as a kernel's) carries a rounding error
    that scales with the magnitudes summed, A_r = sum_k |fc3.weight_k h2_rk| +
    |fc3.bias| (+ |vt_r| for the subtraction's other operand), not with the
    difference: 16 ulps of A_r are kappa x 16 ulps of the gradient's scale,
        kappa = max_r (A_r + |vt_r|) / max_r |v_r - vt_r|
    and for fc3.bias, the plain sum (2 / mb) sum_r (v_r - vt_r) whose terms
    also cancel among the rows,
        kappa = sum_r (A_r + |vt_r|) / |sum_r (v_r - vt_r)|.
    From the f64 reference alone.  On the rows of test_ppo_small_gpu.py: 1.2 ..
    1.3 from 15 rows on (v_target spreads over +-5 against A_r of 3 .. 5), 3 ..
    9 at one or two rows; fc3.bias 5 .. 10 at every size (a sum of random
    signs), 27 at the two rows v - vt = (+0.62, -0.25) of H 256."""
    if not name.startswith("critic."):
        return 1.0
    if name == "critic.fc3.bias":
        return max(1.0, float(ref.v_mag.sum() / ref.v_diff.sum().abs()))
    return max(1.0, float(ref.v_mag.max() / ref.v_diff.abs().max()))


def rel_err(got, ref64):
    """max |got - ref64| / max |ref64| (0 for an all-zero reference that is met)."""
    ref64 = ref64.double()
    d = float((got.double().cpu().reshape(ref64.shape) - ref64).abs().max())
    m = float(ref64.abs().max())
    return d / m if m > 0 else (0.0 if d == 0 else math.inf)
