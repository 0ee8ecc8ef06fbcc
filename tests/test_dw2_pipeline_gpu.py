"""dW2 at H 256 (dw2_kx_body in ppo_kernels.hip): the chunk loop is a software
pipeline -- chunk c's MFMAs from one register set while chunk c+1's LDS reads
fill the other and the LDS-DMA stream runs further chunks ahead through the
ring -- so the shapes here are the ones at which its prologue, the ring's wrap
and the tail's reloads differ: one to nine 32-row chunks per split, splits of
unequal length, ragged rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 256
# (mb, S): chunks per split
CASES = [(32, 1),     # one chunk: the prologue only
         (64, 1),     # two chunks
         (96, 1),     # three: one full ring
         (128, 1),    # four: the ring wraps
         (288, 1),    # nine: three laps
         (160, 2),    # 3 + 2
         (160, 3),    # 2 + 2 + 1
         (160, 5),    # 1 each
         (100, 1)]    # ragged rows, zero-filled in the planes

_planes = {}


def _setup(mb):
    """A learner at H 256 with perturbed weights, its stepper for mb, the
    planes the rowpass wrote and their f32 decode (once per mb)."""
    if mb in _planes:
        return _planes[mb]
    from satrl.ppo import PPOLearner
    from satrl.trainer import args_param
    torch.manual_seed(5)
    B = 8192
    args = args_param(chkpt_dir="/tmp", hidden_width=H, mini_batch_size=mb, batch_size=B)
    args.state_dim, args.action_dim, args.max_action = 18, 3, 1.6
    L = PPOLearner(args, "pursuer", use_graph=False)
    with torch.no_grad():
        for p in list(L.actor.parameters()) + list(L.critic.parameters()):
            p.add_(torch.randn_like(p) * 0.05)
    L.sync_w2t()
    g = torch.Generator(device="cuda").manual_seed(6)
    src = torch.randn((B, 32), device="cuda", generator=g)
    src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
    st = L.stepper(mb)
    assert st.kx(mb)
    st.ptail.fill_(7.0)
    st.pw1.fill_(7.0)
    st.H1x.fill_(-1)
    st.dZ2x.fill_(-1)
    st.rowpass_kx(src, None)
    torch.cuda.synchronize()
    rows = (mb + 31) // 32 * 32

    def decode(x):
        p = x.view(2, 3, rows // 8, H, 8).view(torch.bfloat16).float()
        v = (p[:, 0] + p[:, 1]) + p[:, 2]                           # [2][rows/8][H][8]
        return v.permute(0, 1, 3, 2).reshape(2, rows, H)
    h1, dz2 = decode(st.H1x), decode(st.dZ2x)
    assert not h1[:, mb:].any() and not dz2[:, mb:].any() and h1[:, :mb].any() and dz2[:, :mb].any()
    _planes[mb] = (L, st, h1.double(), dz2.double(), rows)
    return _planes[mb]


@pytest.mark.parametrize("mb,S,net", [(mb, S, -1) for mb, S in CASES] + [(160, 2, 0), (160, 2, 1)])
def test_dw2_kx_slabs(mb, S, net):
    """Every slab s of satrl_ppo_dw2_kx at an explicit S is the f64 sum over
    its own rows [s KR, (s+1) KR) within the split-bf16 bound (relative to
    sum |a b|: <= 2.2e-7 per product sum + f32 accumulation, the bar of
    test_kx_rowpass_planes_and_dw2), slab slots the launch does not own keep
    their NaN, a second launch repeats the bits, and satrl_ppo_dw2_kx_w1
    (mode 3) writes the same bits."""
    import satrl._lib as _L
    from satrl._lib import ptr
    from satrl.ppo import rowpass_exchange_check
    L, st, h1, dz2, rows = _setup(mb)
    lib, sp = _L.lib(), _L.stream_ptr()
    nch = rows // 32
    KR = (nch + S - 1) // S * 32
    nets = (0, 1) if net < 0 else (net,)
    slots = st.p2.numel() // (H * H)
    assert 2 * S <= slots

    def run(w1):
        st.p2.fill_(float("nan"))
        if w1:
            rc = lib.satrl_ppo_dw2_kx_w1(H, mb, net, S, ptr(st.H1x), ptr(st.dZ2x), st.H1x.numel(), ptr(st.p2),
                                         st.p2.numel(), 3, ptr(st.pw1), ptr(st.ptail), ptr(L.G), ptr(st.nsq[0]), sp)
        else:
            rc = lib.satrl_ppo_dw2_kx(H, mb, net, S, ptr(st.H1x), ptr(st.dZ2x), st.H1x.numel(), ptr(st.p2),
                                      st.p2.numel(), sp)
        _L.check(rc, "satrl_ppo_dw2_kx_w1" if w1 else "satrl_ppo_dw2_kx")
        torch.cuda.synchronize()
        return st.p2.clone().view(slots, H, H)

    got = run(False)
    owned = {n * S + s for n in nets for s in range(S)}
    for slot in range(slots):
        if slot not in owned:
            assert bool(torch.isnan(got[slot]).all()), slot
    worst = 0.0
    for n in nets:
        for s in range(S):
            a, b = dz2[n, s * KR:(s + 1) * KR], h1[n, s * KR:(s + 1) * KR]
            assert a.shape[0] > 0
            ref = torch.einsum("rn,rm->nm", a, b)
            mag = torch.einsum("rn,rm->nm", a.abs(), b.abs())
            slab = got[n * S + s]
            assert bool(torch.isfinite(slab).all()), (n, s)
            err = ((slab.double() - ref).abs() / mag.clamp_min(1e-30)).max().item()
            worst = max(worst, err)
            assert err < 2e-6, (n, s, err)
    print(f"mb {mb} S {S} net {net}: worst slab error {worst:.3e} of sum |a b|")
    again, fused = run(False), run(True)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    assert torch.equal(got.view(torch.int32), fused.view(torch.int32))
    rowpass_exchange_check()
