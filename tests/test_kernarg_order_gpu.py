"""Every launcher whose kernel's argument order is laid out for kernarg
preload (rowpass, dW2, reduce, Adam), each argument reached at
the smallest shapes that do so.  Two pointers of one type swapped between a
kernel's signature and its launch compile cleanly; here they cannot pass:
every output buffer starts as NaN (the bf16 planes as 0xFFFF, a bf16 NaN),
every value written is compared with the f64 reference of
test_ppo_small_gpu.py at that file's tolerances (its bar rule for dZ2 and
gradients, its H1 bound, its parameter tolerance after an Adam step), every
buffer or region a call must not write still holds its NaNs, and the inputs
are bitwise what they were.

Shapes: H 256 at 33 rows (ragged: two 32-row chunks of planes, three 16-row
blocks) and 16 rows, both nets in one launch (the column-split kernel) and
one net per launch (the 16-row kernel, net_sel >= 0); H 256 at 1057 rows (the
32-row kernel of the long minibatches: 34 blocks, the last with one row); H 64
at 33 rows (the rowpass that multiplies dW2 itself, and the plain one)."""
import functools

import pytest
import torch

import ppo_cases as pc
import test_ppo_small_gpu as small

pytestmark = pytest.mark.gpu

NAN = float("nan")
B = 2048


@functools.lru_cache(maxsize=None)
def _setup(H):
    L, actor, critic = pc.gpu_learner(H)
    src_c = pc.packed_rows(B, seed=31)
    return L, actor, critic, L.P.clone(), src_c, src_c.cuda()


@functools.lru_cache(maxsize=None)
def _case(H, mb):
    """The rows of a case (gathered through idx), and their references."""
    L, actor, critic, _, src_c, _ = _setup(H)
    idx = torch.randperm(B, generator=torch.Generator().manual_seed(1000 * H + mb))[:mb]
    ref, r32 = small._refs(actor, critic, src_c[idx], lr=L.lr_a)
    return idx.cuda(), ref, r32


def _poison(L, st):
    for t in (st.H1, st.dZ2, st.ptail, st.pw1, st.p2, L.G):
        t.fill_(NAN)
    st.nsq.fill_(NAN)
    if st.kx_on:
        st.H1x.fill_(-1)
        st.dZ2x.fill_(-1)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _inputs_intact(L, P0, W0, src, tag):
    src_c = _setup(L.H)[4]
    assert torch.equal(L.P, P0) and torch.equal(L.W2T, W0), tag
    assert torch.equal(src.cpu().view(torch.int32), src_c.view(torch.int32)), tag


def _decode(x, rp, H):
    """The f32 rows [2][rp][H] of k-packed planes u16 [2][3][rp / 8][H][8]."""
    p = x[:2 * 3 * rp * H].view(2, 3, rp // 8, H, 8).view(torch.bfloat16).float()
    return ((p[:, 0] + p[:, 1]) + p[:, 2]).permute(0, 1, 3, 2).reshape(2, rp, H).cpu()


def _net_names(L, net, skip_w2=False):
    names = [k for k in L.flat_views(L.G) if not (skip_w2 and k.endswith("fc2.weight"))]
    return [k for k in names if net < 0 or k.startswith("critic." if net else "actor.")]


def _check_rows(tag, H, mb, net, H1, dZ2, rows, ref, r32, actor, critic, bad):
    """H1 against test_rowpass_rows_vs_f64's bound, dZ2 against the bar rule."""
    s = rows[:, 0:18].double()
    for k, m in enumerate((actor, critic)):
        if net >= 0 and k != net:
            continue
        mag = s.abs() @ m.fc1.weight.detach().double().abs().T
        bound = 2.0 ** -24 * (20.0 * mag + m.fc1.bias.detach().double().abs() + 3.0)
        q = float(((H1[k].double() - ref.H1[k]).abs() / bound).max())
        print(f"{tag} H1 net {k}: worst error / bound {q:.3f}")
        if not q <= 1.0:
            bad.append((tag, "H1", k, q))
        small._compare(f"{tag} dZ2 net {k}", dZ2[k], ref.dZ2[k], r32.dZ2[k], bad)


@pytest.mark.parametrize("H,mb", [(256, 33), (256, 16), (256, 1057), (64, 33)])
def test_rowpass_arguments(H, mb):
    """satrl_ppo_rowpass_ratio (f32 rows, every output pointer of
    rowpass_kernel but p2) for both nets and for each net alone, then at H 256
    satrl_ppo_rowpass_kx (planes) and at H 64 satrl_ppo_rowpass_dw2 (p2 slabs)
    the same three ways.  Per launch: H1, dZ2 (rows or decoded planes), the
    summed slabs, the ratio and the dW2 slabs against f64; the other net's
    half of H1 / dZ2, the slab slots past the launched row blocks, the
    elements past the rows, p2 where the launch has no dW2, G, and the planes
    of a row launch (the rows of a plane launch) keep their NaNs."""
    import satrl._lib as _L
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check
    L, actor, critic, P0, src_c, src = _setup(H)
    small._restore(L, P0)
    W0 = L.W2T.clone()
    idx, ref, r32 = _case(H, mb)
    rows = src_c[idx.cpu()]
    st = FusedMinibatch(L, mb + 32, 1, use_graph=False)
    nrb = _L.lib().satrl_ppo_row_blocks(H, mb)
    assert 1 <= nrb < st.nwg
    n, HH, bad = 2 * mb * H, H * H, []
    tail_w, w1_w = 6 * H + 12, 2 * H * 20
    for net in (-1, 0, 1):
        tag = f"H {H} mb {mb} net {net}"
        names = _net_names(L, net, skip_w2=True)
        # ---- f32 rows, ratio ----
        _poison(L, st)
        ratio = torch.full((mb,), NAN, device="cuda")
        st.rowpass_ratio(src, idx, ratio, mb, net)
        torch.cuda.synchronize()
        H1, dZ2 = st.H1[:n].view(2, mb, H).cpu(), st.dZ2[:n].view(2, mb, H).cpu()
        _check_rows(tag, H, mb, net, H1, dZ2, rows, ref, r32, actor, critic, bad)
        for k in (0, 1):
            if net >= 0 and k != net:
                assert _all_nan(H1[k]) and _all_nan(dZ2[k]), tag
        assert _all_nan(st.H1[n:]) and _all_nan(st.dZ2[n:]), tag
        assert _all_nan(st.ptail.view(-1, tail_w)[nrb:]) and _all_nan(st.pw1.view(-1, w1_w)[nrb:]), tag
        assert _all_nan(st.p2) and _all_nan(L.G) and _all_nan(st.nsq), tag
        if st.kx_on:
            assert bool((st.H1x == -1).all()) and bool((st.dZ2x == -1).all()), tag
        flat = torch.nan_to_num(small._slab_sums(L, st, nrb), nan=0.0) if net >= 0 else small._slab_sums(L, st, nrb)
        small._check_grads(tag + " slabs", L.flat_views(flat), ref, r32, bad, names)
        if net != 1:
            q = float((ratio.cpu().double() / ref.ratio - 1).abs().max())
            print(f"{tag}: ratio worst relative error {q:.3e}")
            assert q <= 1e-5, (tag, q)                                   # (test_loss_head_branches' bound)
        else:
            assert _all_nan(ratio), tag                                  # the actor's ratio: not the critic's launch
        tail, w1 = st.ptail.clone(), st.pw1.clone()
        _inputs_intact(L, P0, W0, src, tag)
        # ---- planes (H 256) ----
        if st.kx_on:
            _poison(L, st)
            st.rowpass_kx(src, idx, mb, net)
            torch.cuda.synchronize()
            rp = (mb + 31) // 32 * 32
            ne = 2 * 3 * rp * H
            assert ne == _L.lib().satrl_ppo_kx_elems(H, mb)
            assert bool((st.H1x[ne:] == -1).all()) and bool((st.dZ2x[ne:] == -1).all()), tag
            for name, x, want in (("H1", st.H1x, H1), ("dZ2", st.dZ2x, dZ2)):
                pl = x[:ne].view(2, 3 * rp * H)
                for k in (0, 1):
                    if net >= 0 and k != net:
                        assert bool((pl[k] == -1).all()), (tag, name, k)   # the other net's planes untouched
                        continue
                    got = _decode(x, rp, H)[k]
                    assert torch.equal(got[:mb], want[k]), (tag, name, k)  # the f32 launch's rows bit for bit
                    assert not bool(got[mb:].any()), (tag, name, k)        # the chunk's padding rows: zero
            eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert eq(st.ptail, tail) and eq(st.pw1, w1), tag              # the same slabs, NaN slots included
            assert _all_nan(st.H1) and _all_nan(st.dZ2) and _all_nan(st.p2) and _all_nan(L.G), tag
            _inputs_intact(L, P0, W0, src, tag)
        # ---- the rowpass's own dW2 slabs (H 64) ----
        if st.fused_dw2:
            _poison(L, st)
            st.rowpass_dw2(src, idx, mb, net)
            torch.cuda.synchronize()
            eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert eq(st.ptail, tail) and eq(st.pw1, w1), tag
            assert _all_nan(st.H1) and _all_nan(st.dZ2) and _all_nan(L.G), tag
            # p2 [2][S][H][H], S = the row blocks; a one-net launch writes its net's half
            slabs = st.p2[:2 * nrb * HH].view(2, nrb, HH)
            assert _all_nan(st.p2[2 * nrb * HH:]), tag
            for k in (0, 1):
                if net >= 0 and k != net:
                    assert _all_nan(slabs[k]), (tag, k)
                    continue
                name = ("actor", "critic")[k] + ".fc2.weight"
                small._compare(f"{tag} dW2 {name}", slabs[k].double().sum(0).cpu(), ref.grads[name],
                               r32.grads[name], bad, pc.critic_kappa(ref, name))
            _inputs_intact(L, P0, W0, src, tag)
    if H == 256:
        rowpass_exchange_check()
    assert not bad, bad


@pytest.mark.parametrize("S", [2, 1])
def test_dw2_arguments(S):
    """satrl_ppo_dw2_kx and satrl_ppo_dw2_kx_w1 at H 256, 33 rows (two 32-row
    plane chunks): S = 2 splits of one chunk and S = 1 split of two, both nets
    and each net alone.  dw2_kx writes the slabs p2 [2][S][H][H] (a one-net
    launch its net's half) and nothing else; dw2_kx_w1 (mode 3) the same slabs bit for bit, G outside
    fc2.weight (bar rule against f64) and the squared-norm pairs of exactly
    its own blocks, which add up to the squares of what it put into G."""
    import satrl._lib as _L
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check
    H, mb = 256, 33
    L, actor, critic, P0, src_c, src = _setup(H)
    small._restore(L, P0)
    idx, ref, r32 = _case(H, mb)
    st = FusedMinibatch(L, mb + 32, 1, use_graph=False)
    HH, bad = H * H, []
    crit = small._critic_mask(L.off, H).cuda()
    for net in (-1, 0, 1):
        tag = f"S {S} net {net}"
        nn = 2 if net < 0 else 1
        _poison(L, st)
        st.rowpass_kx(src, idx, mb, net)
        h1x, dzx = st.H1x.clone(), st.dZ2x.clone()
        st.p2.fill_(NAN)
        st.dw2_kx(mb, S, net)
        torch.cuda.synchronize()
        p2 = st.p2.clone()
        assert _all_nan(p2[2 * S * HH:]) and _all_nan(L.G) and _all_nan(st.nsq), tag
        for k in (0, 1):
            slab = p2[:2 * S * HH].view(2, S, HH)[k]
            if net >= 0 and k != net:
                assert _all_nan(slab), (tag, k)                           # a one-net launch: its net's half
                continue
            name = ("actor", "critic")[k] + ".fc2.weight"
            small._compare(f"{tag} dW2 {name}", slab.double().sum(0).cpu(), ref.grads[name], r32.grads[name], bad,
                           pc.critic_kappa(ref, name))
        st.p2.fill_(NAN)
        nsq = st.nsq[max(net, 0)]
        assert st.dw2_kx_w1(mb, S, net, 3, nsq) is None                  # (the fused launch, always: no fallback to report)
        torch.cuda.synchronize()
        assert torch.equal(st.p2.view(torch.int32), p2.view(torch.int32)), tag
        assert torch.equal(st.H1x, h1x) and torch.equal(st.dZ2x, dzx), tag
        G = L.G.clone()
        assert _all_nan(G[:2 * HH]), tag                                  # fc2.weight is the reduce's
        live = ~torch.isnan(G)
        assert bool((live[2 * HH:] == ((crit[2 * HH:] == bool(net)) if net >= 0 else True)).all()), tag
        small._check_grads(tag + " G", L.flat_views(torch.nan_to_num(G, nan=0.0)), ref, r32, bad,
                           _net_names(L, net, skip_w2=True))
        small._check_pads(L, torch.nan_to_num(G, nan=0.0), tag)
        # the norm pairs: the W2 blocks' (nb2 = nn H H / 4 / 64 of them) are the reduce's
        nb2 = nn * HH // 4 // 64
        pairs = nsq.view(-1, 2)
        assert _all_nan(pairs[:nb2]) and _all_nan(st.nsq[1 - max(net, 0)]), tag
        done = pairs[nb2:][~torch.isnan(pairs[nb2:, 0])]
        sq = torch.nan_to_num(G, nan=0.0).double() ** 2
        want = torch.stack([sq[~crit].sum(), sq[crit].sum()])
        assert torch.allclose(done.sum(0), want, rtol=1e-12, atol=0), (tag, done.sum(0), want)
    rowpass_exchange_check()
    assert not bad, bad


@pytest.mark.parametrize("H", [256, 64])
def test_reduce_adam_one_net(H):
    """One chain of the split-chains step (FusedMinibatch._net_step: rowpass,
    dW2, reduce, Adam with net_sel = the net) at 33 rows, the actor alone and
    the critic alone, from NaN-filled G, slabs and norm partials.  The net's
    gradients in G against f64 (bar rule), its parameters after the step
    against f64 clip + Adam (rtol 1e-5, atol 2e-7: the suite's tolerance for
    parameters after a step), its M and V finite, its fc2 operand image the
    transpose of the new fc2.weight, one step counted; the other net's G still
    NaN, its P, M, V, operand image and step counter bitwise untouched."""
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check, w2x_image
    mb = 33
    L, actor, critic, P0, src_c, src = _setup(H)
    idx, ref, r32 = _case(H, mb)
    st = FusedMinibatch(L, mb + 32, 1, use_graph=False)
    HH, bad = H * H, []
    crit = small._critic_mask(L.off, H).cuda()
    for net in (0, 1):
        tag = f"H {H} net {net}"
        small._restore(L, P0)
        L.use_grad_clip = True
        other = crit != bool(net)
        L.M[other] = 3.0                                                 # the other net's state: sentinels
        L.V[other] = 5.0
        W0 = L.W2T.clone()
        _poison(L, st)
        st._net_step(src, idx, mb, net)
        torch.cuda.synchronize()
        G = L.G.clone()
        assert _all_nan(G[other]) and not bool(torch.isnan(G[~other]).any()), tag
        small._check_grads(tag + " G", L.flat_views(torch.nan_to_num(G, nan=0.0)), ref, r32, bad, _net_names(L, net))
        small._check_pads(L, torch.nan_to_num(G, nan=0.0), tag)
        assert L.steps.cpu().tolist() == [1.0 - net, float(net)], tag
        assert torch.equal(L.P[other], P0[other]), tag
        assert bool((L.M[other] == 3.0).all()) and bool((L.V[other] == 5.0).all()), tag
        assert bool(torch.isfinite(L.M[~other]).all()) and bool(torch.isfinite(L.V[~other]).all()), tag
        assert bool((L.V[~other] >= 0).all()), tag
        P = L.flat_views(L.P)
        for k in _net_names(L, net):
            r = ref.params[k]
            q = float(((P[k].reshape(r.shape).double().cpu() - r).abs() / (2e-7 + 1e-5 * r.abs())).max())
            print(f"{tag} {k}: |dP| / tolerance {q:.3f}")
            if not q <= 1.0:
                bad.append((tag, k, q))
        img = w2x_image(L.P[:2 * HH].cpu(), H)
        W = L.W2T.cpu()
        for k in (0, 1):
            want = img[k * HH:(k + 1) * HH] if k == net else W0[k * HH:(k + 1) * HH].cpu()
            assert torch.equal(W[k * HH:(k + 1) * HH].view(torch.int32), want.view(torch.int32)), (tag, k)
        assert torch.equal(src.cpu().view(torch.int32), src_c.view(torch.int32)), tag
    if H == 256:
        rowpass_exchange_check()
    small._restore(L, P0)
    assert not bad, bad
