"""The MLP kernels' data-dependent short cuts (ppo_kernels.hip) leave every
output bit where it was:

  tanh_f32_n   a wave whose fc1 values are all on one side of |x| = 0.625
               runs one arm of tanh_f32 only (kTanhArms: the forward pass of
               the H 256 kernels);
  phase E      a wave whose dZ1 = dH1 (1 - H1^2) is all +-0, in a block whose
               gathered rows are finite, stores +0.0 instead of multiplying
               (kZeroSkip: the 32-row H 256 rowpass).
The other kernels run the same cases: whatever kernel a shape reaches, the
outputs are the f64 reference's within the bounds and the slabs' bytes are
those the products give.

Rowpass shapes: the smallest that reach every kernel and path -- at H 256 the
32-row kernel in both sync forms (satrl_ppo_rowpass_kx32) at one full block
(32), a ragged block ending in its first 16-row tile (40) and in its second
(55); the column-split and the 16-row kernels at one block (16) and a ragged
second one (24); H 64 and H 128 (f32 rows, and at H 64 the fused-dW2 kernel)
at 32 and 40.  Three observation scalings each:
  "sat"    x 1e5, rows scaled up further until every fc1 pre-activation of
           both nets is beyond +-100 (asserted from the f64 reference's
           weights): tanh(fc1) = +-1 exactly, every wave in the exp/rcp arm
           (a ragged block's zero rows make its waves mixed);
  "small"  x 1e-3: every |fc1 pre-activation| < 0.625 (asserted): the
           polynomial arm alone;
  "alt"    rows alternating between the two, and one all-zero row: every
           wave holds both kinds.
Bounds: test_ppo_small_gpu.py's -- the bar rule (ppo_cases.bar, critic tensors
with kappa) for dZ2 and the slab sums, and for H1 its first-order bound
2^-24 (20 sum |W1||s| + |b1| + 3).  The f64 reference of a (H, mb, scaling)
is computed once and shared."""
import functools

import pytest
import torch

import ppo_cases as pc
from torch_reference import reference_full, reference_step_f64

pytestmark = pytest.mark.gpu

SCALINGS = ("sat", "small", "alt")
B = 64                                  # rows of a source table


# ---------------------------------------------------------------------------
# tanh_f32 against tanh_f32_n
# ---------------------------------------------------------------------------
def _tanh_inputs():
    """2^20 values = 2048 waves of 64 threads x 8 values (a wave is 512
    consecutive values).  Wave k is of kind k % 4: 0 all big (|x| >= 0.625,
    log-uniform up to 1e6), 1 all small (log-uniform down to 1e-6), 2 all big
    but ONE value of one lane, 3 each value big or small at random.  The
    special values go into the first waves of each kind that admits them."""
    g = torch.Generator().manual_seed(3)
    nw = 2048
    u = torch.rand((nw, 512), generator=g)
    sign = torch.where(torch.rand((nw, 512), generator=g) < 0.5, -1.0, 1.0)
    big = 0.625 * torch.exp(u * 14.3)                              # 0.625 .. 1e6
    small = 0.625 * torch.exp(-u * 13.4) * (1 - 2.0 ** -20)        # 1e-6 .. below 0.625
    assert bool((big.float() >= 0.625).all()) and bool((small.float() < 0.625).all())
    kind = torch.arange(nw) % 4
    pick_small = torch.zeros((nw, 512), dtype=torch.bool)
    pick_small[kind == 1] = True
    pick_small[kind == 3] = torch.rand((int((kind == 3).sum()), 512), generator=g) < 0.5
    one = (kind == 2).nonzero().reshape(-1)
    pick_small[one, torch.randint(0, 512, (one.numel(),), generator=g)] = True
    x = (torch.where(pick_small, small, big) * sign).float()
    e = torch.tensor(0.625)
    up, down = torch.nextafter(e, torch.tensor(1.0)), torch.nextafter(e, torch.tensor(0.0))
    sm = [0.0, -0.0, float(down), -float(down), 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 3e-41]
    bg = [0.625, -0.625, float(up), -float(up), float("inf"), -float("inf"), float("nan"), 88.0, -104.0]
    # (values 1.. of a wave: its value 0 may be kind 2's one small value)
    for k, vals in ((0, bg), (1, sm), (2, bg), (3, bg + sm)):
        for w in range(4):                                         # the first four waves of the kind
            pos = 1 + torch.randperm(511, generator=g)[:len(vals)]
            keep = ~pick_small[4 * w + k, pos] if k == 2 else torch.ones(len(vals), dtype=torch.bool)
            x[4 * w + k, pos[keep]] = torch.tensor(vals)[keep]
    # the kinds are what they claim
    xs = x.abs() < 0.625
    assert not bool(xs[kind == 0].any()) and bool(xs[kind == 1].all())
    assert bool((xs[kind == 2].sum(1) == 1).all())
    return x.reshape(-1)


def test_tanh_forms_bitwise():
    """satrl_tanh_forms: the per-wave arm selection returns tanh_f32's bits on
    whole waves of each kind, +-0, +-0.625 and its neighbours, +-inf, NaN and
    denormals among them; and form 0 is satrl_ppo_tanh's function."""
    import satrl._lib as _L
    lib, sp = _L.lib(), _L.stream_ptr()
    x = _tanh_inputs().cuda()
    n = x.numel()
    assert n == 1 << 20
    y0, y1, y2 = (torch.full_like(x, 7.0) for _ in range(3))
    assert lib.satrl_tanh_forms(_L.ptr(x), _L.ptr(y0), n, 0, sp) == 0
    assert lib.satrl_tanh_forms(_L.ptr(x), _L.ptr(y1), n, 1, sp) == 0
    assert lib.satrl_ppo_tanh(n, _L.ptr(x), _L.ptr(y2), sp) == 0
    torch.cuda.synchronize()
    assert lib.satrl_tanh_forms(_L.ptr(x), _L.ptr(y0), n - 1, 0, sp) == -1     # whole threads only
    assert lib.satrl_tanh_forms(_L.ptr(x), _L.ptr(y0), n, 2, sp) == -1
    b0, b1, b2 = (t.view(torch.int32) for t in (y0, y1, y2))
    assert torch.equal(b0, b2)
    diff = (b0 != b1).nonzero().reshape(-1)
    assert diff.numel() == 0, [(int(i), float(x[i]), float(y0[i]), float(y1[i])) for i in diff[:8]]
    # and they are tanh: the oracle is not trivially equal to its input or constant
    fin = torch.isfinite(x)
    assert float((y0[fin].double() - torch.tanh(x[fin].double())).abs().max()) < 3e-7
    assert bool(torch.isnan(y0[torch.isnan(x)]).all())


# ---------------------------------------------------------------------------
# rowpass
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _learner(H):
    return pc.gpu_learner(H)


@functools.lru_cache(maxsize=None)
def _table(H, scaling):
    """B packed rows (CPU) whose states are scaled as `scaling` says, for the
    weights of _learner(H); the claims of the module docstring asserted in
    f64 from those weights."""
    _, actor, critic = _learner(H)
    rows = pc.packed_rows(B, seed=40 + H)
    s = rows[:, 0:18]

    def z1_abs():                                                   # [2][B][H]
        return torch.stack([(s.double() @ n.fc1.weight.detach().double().T + n.fc1.bias.detach().double()).abs()
                            for n in (actor, critic)])
    sat = torch.ones(B, dtype=torch.bool) if scaling == "sat" else \
        (torch.arange(B) % 2 == 0) if scaling == "alt" else torch.zeros(B, dtype=torch.bool)
    s[sat] *= 1e5
    s[~sat] *= 1e-3
    for _ in range(40):                                             # saturated rows: every |z1| > 100
        low = sat & (z1_abs().amin((0, 2)) <= 100.0)
        if not bool(low.any()):
            break
        s[low] *= 1.7
    if scaling == "alt":
        s[13] = 0.0                                                 # (a small row: z1 = b1)
    z = z1_abs()
    assert bool((z[:, sat].amin() > 100.0)) if bool(sat.any()) else True
    assert bool((z[:, ~sat] < 0.625).all())
    return rows


@functools.lru_cache(maxsize=None)
def _refs(H, scaling, mb, gather):
    rows_all = _table(H, scaling)
    _, actor, critic = _learner(H)
    g = torch.Generator().manual_seed(1000 * H + mb)
    idx = torch.randperm(B, generator=g)[:mb] if gather else None
    rows = rows_all[:mb] if idx is None else rows_all[idx]
    return (rows, idx, reference_step_f64(actor, critic, rows),
            reference_full(actor, critic, rows, dtype=torch.float32))


def _compare(tag, got, ref64, ref32, bad, kappa=1.0):
    err, e32 = pc.rel_err(got, ref64), pc.rel_err(ref32, ref64)
    bar = pc.bar(e32, kappa)
    print(f"{tag}: err {err:.3e} e32 {e32:.3e} err/bar {err / bar:.3f}")
    if not err <= bar:
        bad.append((tag, err, e32, bar))


def _check_rows_and_slabs(tag, H, L, nets, rows, ref, r32, H1, dZ2, pw1, ptail, nrb, bad):
    """H1, dZ2 [2][mb][H] (CPU) and the slabs of the nrb launched row blocks
    against the f64 reference."""
    s = rows[:, 0:18].double()
    for k, net in enumerate(nets):
        mag = s.abs() @ net.fc1.weight.detach().double().abs().T
        bound = 2.0 ** -24 * (20.0 * mag + net.fc1.bias.detach().double().abs() + 3.0)
        q = float(((H1[k].double() - ref.H1[k]).abs() / bound).max())
        print(f"{tag} H1 net {k}: worst error / bound {q:.3f}")
        if not q <= 1.0:
            bad.append((tag, "H1", k, q))
        _compare(f"{tag} dZ2 net {k}", dZ2[k], ref.dZ2[k], r32.dZ2[k], bad)
    o = L.off
    flat = torch.zeros(o["total"], dtype=torch.float64, device=pw1.device)
    flat[o["W1"]:o["W1"] + 2 * H * 20] = pw1.view(-1, 2 * H * 20)[:nrb].double().sum(0)
    flat[o["b2"]:o["total"]] = ptail.view(-1, 6 * H + 12)[:nrb].double().sum(0)
    views = L.flat_views(flat)
    for name in views:
        if not name.endswith("fc2.weight"):
            _compare(f"{tag} slabs {name}", views[name], ref.grads[name], r32.grads[name], bad,
                     pc.critic_kappa(ref, name))


def _w1_slabs_are_plus_zero(pw1, H, nrb):
    """The [dW1|db1] slabs of the launched blocks are +0.0 as bytes: columns
    0..18 (dW1, db1) and the pad column 19."""
    return bool((pw1.view(-1, 2 * H * 20)[:nrb].view(torch.int32) == 0).all())


def _decode(x, mb, H):
    rp = (mb + 31) // 32 * 32
    p = x[:2 * 3 * rp * H].view(2, 3, rp // 8, H, 8).view(torch.bfloat16).float()
    v = (p[:, 0] + p[:, 1]) + p[:, 2]
    return v.permute(0, 1, 3, 2).reshape(2, rp, H)[:, :mb].cpu()


def _fill(st):
    for t, v in ((st.ptail, 7.0), (st.pw1, 7.0), (st.H1, 7.0), (st.dZ2, 7.0)):
        t.fill_(v)
    if hasattr(st, "H1x"):
        st.H1x.fill_(-1)
        st.dZ2x.fill_(-1)


def _kx32(L, st, src, idx, mb, ratio):
    import satrl._lib as _L
    from satrl._lib import check, ptr
    check(_L.lib().satrl_ppo_rowpass_kx32(256, mb, -1, ptr(src), None if idx is None else ptr(idx), ptr(L.P),
                                          ptr(L.W2T), float(L.epsilon), float(L.entropy_coef), float(L.max_action),
                                          ptr(st.H1x), ptr(st.dZ2x), st.H1x.numel(), ptr(st.ptail), ptr(st.pw1),
                                          ptr(ratio), _L.stream_ptr()), "satrl_ppo_rowpass_kx32")


@pytest.fixture()
def sync_switch():
    from satrl.ppo import rowpass_sync
    prev = rowpass_sync()
    yield rowpass_sync
    rowpass_sync(prev)


@pytest.mark.parametrize("scaling", SCALINGS)
@pytest.mark.parametrize("mb", (32, 40, 55))
def test_rowpass32_h256(sync_switch, mb, scaling):
    """The 32-row H 256 kernel, barrier and hand-off forms: the hand-off
    form's planes, slabs and ratio are the barrier form's bytes; the decoded
    H1 / dZ2 and the slab sums meet the f64 bounds; saturated, the [dW1|db1]
    slabs are +0.0 as bytes."""
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check
    H = 256
    L, actor, critic = _learner(H)
    rows, idx, ref, r32 = _refs(H, scaling, mb, mb == 55)
    src = (_table(H, scaling) if idx is not None else rows).cuda()
    idx_d = None if idx is None else idx.cuda()
    st = FusedMinibatch(L, 64, 1, use_graph=False)
    rowpass_exchange_check()
    outs = []
    for mode in (0, 1):
        sync_switch(mode)
        _fill(st)
        ratio = torch.full((mb,), 7.0, device="cuda")
        _kx32(L, st, src, idx_d, mb, ratio)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (st.H1x, st.dZ2x, st.pw1, st.ptail, ratio)])
    rowpass_exchange_check()
    for name, a, b in zip(("H1 planes", "dZ2 planes", "[dW1|db1] slabs", "tail slabs", "ratio"), *outs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b), name
    H1x, dZ2x, pw1, ptail, ratio = outs[1]
    nrb = (mb + 31) // 32
    bad = []
    _check_rows_and_slabs(f"H 256 mb {mb} {scaling}", H, L, (actor, critic), rows, ref, r32, _decode(H1x, mb, H),
                          _decode(dZ2x, mb, H), pw1, ptail, nrb, bad)
    q = float((ratio.cpu().double() / ref.ratio - 1).abs().max())
    print(f"ratio worst relative error {q:.3e}")
    assert q <= 1e-5
    if scaling == "sat":
        assert _w1_slabs_are_plus_zero(pw1, H, nrb)
    else:
        assert not _w1_slabs_are_plus_zero(pw1, H, nrb)
    assert not bad, bad


@pytest.mark.parametrize("scaling", SCALINGS)
@pytest.mark.parametrize("mb", (16, 24))
def test_rowpass16_h256(mb, scaling):
    """The 16-row kernels at H 256: the column split (both nets in one
    k-packed launch), the 16-wave kernel with planes (per-net launches) and
    with f32 rows.  The three agree (slabs as bytes, rows by value) and meet
    the f64 bounds."""
    import satrl._lib as _L
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check, step_plan
    H = 256
    L, actor, critic = _learner(H)
    rows, idx, ref, r32 = _refs(H, scaling, mb, mb == 24)
    src = (_table(H, scaling) if idx is not None else rows).cuda()
    idx_d = None if idx is None else idx.cuda()
    st = FusedMinibatch(L, 64, 1, use_graph=False)
    assert step_plan(H, mb).rowpass == _L.RP_CS
    nrb = (mb + 15) // 16
    rowpass_exchange_check()
    got = []
    for form in ("cs", "wg16 planes", "wg16 rows"):
        _fill(st)
        if form == "cs":
            st.rowpass_kx(src, idx_d, mb)
        elif form == "wg16 planes":
            st.rowpass_kx(src, idx_d, mb, net=0)
            st.rowpass_kx(src, idx_d, mb, net=1)
        else:
            st.rowpass(src, idx_d, mb)
        torch.cuda.synchronize()
        if form == "wg16 rows":
            n = 2 * mb * H
            H1, dZ2 = st.H1[:n].view(2, mb, H).cpu(), st.dZ2[:n].view(2, mb, H).cpu()
        else:
            H1, dZ2 = _decode(st.H1x, mb, H), _decode(st.dZ2x, mb, H)
        got.append((H1, dZ2, st.pw1.view(-1, 2 * H * 20)[:nrb].clone(), st.ptail.view(-1, 6 * H + 12)[:nrb].clone()))
    rowpass_exchange_check()
    for other in got[1:]:
        # (H1 / dZ2 by value: a plane triple decodes -0.0 to +0.0; the slabs as bytes)
        for name, a, b in zip(("H1", "dZ2"), got[0], other):
            assert torch.equal(a, b), name
        for name, a, b in zip(("[dW1|db1] slabs", "tail slabs"), got[0][2:], other[2:]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    H1, dZ2, pw1, ptail = got[0]
    bad = []
    _check_rows_and_slabs(f"H 256 mb {mb} {scaling}", H, L, (actor, critic), rows, ref, r32, H1, dZ2, pw1, ptail, nrb,
                          bad)
    assert _w1_slabs_are_plus_zero(pw1, H, nrb) == (scaling == "sat")
    assert not bad, bad


@pytest.mark.parametrize("scaling", SCALINGS)
@pytest.mark.parametrize("mb", (32, 40))
@pytest.mark.parametrize("H", (64, 128))
def test_rowpass_h64_h128(H, mb, scaling):
    """H 64 / H 128 (f32 rows); at H 64 also the fused-dW2 kernel, whose
    [dW1|db1] and tail slabs are the f32-rows kernel's bytes."""
    from satrl.ppo import FusedMinibatch
    L, actor, critic = _learner(H)
    rows, idx, ref, r32 = _refs(H, scaling, mb, mb == 40)
    src = (_table(H, scaling) if idx is not None else rows).cuda()
    idx_d = None if idx is None else idx.cuda()
    st = FusedMinibatch(L, 64, 1, use_graph=False)
    nrb = (mb + 31) // 32
    _fill(st)
    st.rowpass(src, idx_d, mb)
    torch.cuda.synchronize()
    n = 2 * mb * H
    H1, dZ2 = st.H1[:n].view(2, mb, H).cpu(), st.dZ2[:n].view(2, mb, H).cpu()
    pw1, ptail = st.pw1.clone(), st.ptail.clone()
    bad = []
    _check_rows_and_slabs(f"H {H} mb {mb} {scaling}", H, L, (actor, critic), rows, ref, r32, H1, dZ2, pw1, ptail, nrb,
                          bad)
    assert _w1_slabs_are_plus_zero(pw1, H, nrb) == (scaling == "sat")
    if H == 64:
        _fill(st)
        st.rowpass_dw2(src, idx_d, mb)
        torch.cuda.synchronize()
        assert torch.equal(st.pw1.view(torch.int32), pw1.view(torch.int32))
        assert torch.equal(st.ptail.view(torch.int32), ptail.view(torch.int32))
    assert not bad, bad


@pytest.mark.parametrize("scaling", SCALINGS)
@pytest.mark.parametrize("H", (64, 128, 256))
def test_rollout_ratio_is_one(H, scaling):
    """A rollout of 64 envs x 4 steps (satrl_policy_act on the scaled
    observations), then satrl_ppo_rowpass_ratio on its transitions: the ratio
    is exactly 1.0f on every row, so the arm selection cannot split the policy
    kernel's forward from the rowpass's."""
    from satrl.ppo import FusedMinibatch, policy_act
    L, _, _ = _learner(H)
    n, T = 64, 4
    g = torch.Generator().manual_seed(7 + H)
    rows = torch.full((n * T, 32), pc.SENTINEL)
    tab = _table(H, scaling)[:, 0:18]
    for t in range(T):                                              # the table's rows in another order each step
        rows[t * n:(t + 1) * n, 0:18] = tab[torch.randperm(B, generator=g)[:n]]
    rows[:, 24] = torch.randn(n * T, generator=g)
    rows[:, 25] = torch.randn(n * T, generator=g)
    rows = rows.cuda()
    for t in range(T):
        obs = rows[t * n:(t + 1) * n, 0:18].contiguous()
        act, lp = torch.empty((n, 3), device="cuda"), torch.empty((n, 3), device="cuda")
        policy_act(H, obs, L.P, None, L.max_action, 5, 0, t, act, lp)
        rows[t * n:(t + 1) * n, 18:21] = act
        rows[t * n:(t + 1) * n, 21:24] = lp
    st = FusedMinibatch(L, n * T, 1, use_graph=False)
    ratio = torch.full((n * T,), float("nan"), device="cuda")
    st.rowpass_ratio(rows, None, ratio)
    torch.cuda.synchronize()
    assert bool((ratio == 1.0).all()), ratio[ratio != 1.0][:8].tolist()


# ---------------------------------------------------------------------------
# phase E's guards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bad_value", (float("nan"), float("inf"), -float("inf")))
@pytest.mark.parametrize("kernel", ("wg32 barrier", "wg32 handoff", "cs", "h64"))
def test_phase_e_nonfinite_rows(sync_switch, kernel, bad_value):
    """One non-finite observation (row 5, state column 3) in a saturated
    block keeps the block on the MFMA path, with the straight path's slab
    bits, derived here:
      NaN   fc1 of row 5 is NaN in every column, so dZ1[5][n] = NaN and every
            element of the block's [dW1|db1] slab of both nets is NaN (NaN x
            S[5][k'], the pad column included: NaN x 0);
      inf   fc1 of row 5 is +-inf where W1[n][3] != 0 (every n), H1 = +-1
            exactly, dZ1 = +-0 in every lane -- the wave-uniform zero test
            passes, and only the finite-rows guard keeps the MFMAs: column 3
            of every slab row is 0 x inf = NaN; every other column is the sum
            of +-0 x finite onto +0: +0.0 as bytes.  The MFMA path giving +0.0
            there is the measured basis of the short cut.
    The second block of the launch (its rows finite) takes the short cut in
    the 32-row kernels and multiplies in the others: +0.0 bytes throughout."""
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check
    H = 64 if kernel == "h64" else 256
    mb = 24 if kernel == "cs" else 40
    R = 16 if kernel == "cs" else 32
    L, actor, critic = _learner(H)
    rows = _table(H, "sat")[:mb].clone()
    for net in (actor, critic):
        assert bool((net.fc1.weight.detach()[:, 3] != 0).all())
    rows[5, 3] = bad_value
    src = rows.cuda()
    st = FusedMinibatch(L, 64, 1, use_graph=False)
    _fill(st)
    if kernel.startswith("wg32"):
        sync_switch(int(kernel.endswith("handoff")))
        _kx32(L, st, src, None, mb, torch.empty((mb,), device="cuda"))
    elif kernel == "cs":
        st.rowpass_kx(src, None, mb)
    else:
        st.rowpass(src, None, mb)
    torch.cuda.synchronize()
    if H == 256:
        rowpass_exchange_check()
    nrb = (mb + R - 1) // R
    slab = st.pw1.view(-1, 2, H, 20)[:nrb].cpu()
    first, rest = slab[0], slab[1:]
    assert bool((rest.view(torch.int32) == 0).all())
    nan = torch.isnan(first)
    if bad_value != bad_value:
        assert bool(nan.all())
    else:
        assert bool(nan[:, :, 3].all()), "0 x inf: the MFMAs ran"
        others = torch.ones(20, dtype=torch.bool)
        others[3] = False
        assert bool((first[:, :, others].view(torch.int32) == 0).all()), "+-0 x finite + (+0) is +0.0 on the MFMA path"
