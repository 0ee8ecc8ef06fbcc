"""The D skip of the 32-row H 256 k-packed rowpass (ppo_kernels.hip
rowpass_kernel, "D skip"; satrl_ppo_rowpass_dskip): a wave whose own tile of
tanh(fc1) is exactly +-1, in a block of finite states, whose dH1 the
exponents of the block's dZ2 and the net's fc2.weight bound to finite values,
skips phase D and phase E's products and stores +0.0 -- every output byte is
the full path's.

Every case runs satrl_ppo_rowpass_kx32 on poisoned outputs with the switch at
1 and at 0 (phase D always runs), in both sync forms, and compares the five
outputs -- H1 planes, dZ2 planes, [dW1|db1] slabs, tail slabs, ratio --
bytewise where they are not NaN, with equal NaN positions; the error word is
read before and after.  Where the inputs are ordinary (cases 1-3) the 0-mode
outputs also meet test_mlp_arms_gpu's f64 bounds (its helpers); the guard
cases 4-5 feed inf, NaN and 1e30-scale values, for which those bounds were
not made, and compare the two modes only.

Shapes: one 32-row block, the unit in which a wave decides (32 rows x its 16
columns), and ragged second blocks ending in either 16-row tile (40, 55),
whose waves must not skip (the rows past the minibatch are not saturated).
The product path runs at 1056 rows: the smallest minibatch of whole 32-row
blocks that the step plan gives to the 32-row kernel (above 1024), an odd
block count (33), so the block-to-workgroup map is the plain one."""
import functools

import pytest
import torch

import ppo_cases as pc
import test_mlp_arms_gpu as arms
from torch_reference import reference_full, reference_step_f64

pytestmark = pytest.mark.gpu

H = 256
NAMES = ("H1 planes", "dZ2 planes", "[dW1|db1] slabs", "tail slabs", "ratio")


@pytest.fixture()
def switches():
    """(rowpass_sync, rowpass_dskip), both restored afterwards."""
    from satrl.ppo import rowpass_dskip, rowpass_sync
    prev = rowpass_sync(), rowpass_dskip()
    yield rowpass_sync, rowpass_dskip
    rowpass_sync(prev[0])
    rowpass_dskip(prev[1])


def _run(L, st, src, idx, mb):
    arms._fill(st)
    ratio = torch.full((mb,), 7.0, device="cuda")
    arms._kx32(L, st, src, idx, mb, ratio)
    torch.cuda.synchronize()
    return [t.clone() for t in (st.H1x, st.dZ2x, st.pw1, st.ptail, ratio)]


def _assert_same(tag, on, off):
    for name, a, b in zip(NAMES, on, off):
        fa, fb = (t.view(torch.bfloat16) if t.dtype == torch.int16 else t for t in (a, b))
        na, nb = torch.isnan(fa), torch.isnan(fb)
        assert torch.equal(na, nb), f"{tag}: {name}: NaN positions differ"
        ia, ib = (t if t.dtype == torch.int16 else t.view(torch.int32) for t in (a, b))
        diff = (ia != ib) & ~na
        assert not bool(diff.any()), f"{tag}: {name}: {int(diff.sum())} values differ, first at " \
                                     f"{int(diff.reshape(-1).nonzero()[0])}"


def _on_off(switches, L, src, idx, mb):
    """{sync form: (outputs with the switch at 1, at 0)}, compared."""
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check
    sync, dskip = switches
    st = FusedMinibatch(L, 64, 1, use_graph=False)
    rowpass_exchange_check()
    got = {}
    for form in (0, 1):
        sync(form)
        outs = []
        for mode in (1, 0):
            dskip(mode)
            outs.append(_run(L, st, src, idx, mb))
        _assert_same(f"sync {form}", *outs)
        got[form] = outs
    rowpass_exchange_check()
    _assert_same("barrier / hand-off", got[0][1], got[1][1])
    return got


def _slab(outs, mb):
    """[block][net][H][20] (CPU) of the launched blocks."""
    return outs[2].view(-1, 2, H, 20)[:(mb + 31) // 32].cpu()


def _f64_bounds(tag, L, nets, rows, ref, r32, outs, mb, cancelling_row=None):
    """test_rowpass32_h256's bounds.  cancelling_row: a row whose fc1 pre-activations cancel (case 3: terms
    of 1e4 summing to 1e-3, so any f32 evaluation of them is off by ~1e-3 and the row's ratio by ~1e-4
    relative): its ratio is held to the bar rule against the f32 torch reference's own error, as dZ2 and
    the gradients are, where every other row keeps the 1e-5."""
    H1x, dZ2x, pw1, ptail, ratio = outs
    bad = []
    arms._check_rows_and_slabs(tag, H, L, nets, rows, ref, r32, arms._decode(H1x, mb, H), arms._decode(dZ2x, mb, H),
                               pw1, ptail, (mb + 31) // 32, bad)
    rel = (ratio.cpu().double() / ref.ratio - 1).abs()
    if cancelling_row is not None:
        arms._compare(f"{tag} ratio", ratio.cpu(), ref.ratio, r32.ratio, bad)
        print(f"{tag}: ratio of row {cancelling_row}: relative error {float(rel[cancelling_row]):.3e}, "
              f"f32 reference {float((r32.ratio.double() / ref.ratio - 1).abs()[cancelling_row]):.3e}")
        rel[cancelling_row] = 0.0
    q = float(rel.max())
    print(f"{tag}: ratio worst relative error {q:.3e}")
    assert q <= 1e-5
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _unit_rows():
    return pc.packed_rows(arms.B, seed=296)                       # unit-variance states, as under obs_norm


@pytest.mark.parametrize("mb", (32, 40, 55))
def test_saturated_blocks_skip_and_match(switches, mb):
    """Case 1: the saturated table.  Equal outputs; the [dW1|db1] slabs of the
    full blocks are +0.0 bytes; the ragged last block (its rows past mb are
    not saturated) takes the full path and matches too."""
    L, actor, critic = arms._learner(H)
    rows, idx, ref, r32 = arms._refs(H, "sat", mb, mb == 55)
    src = (arms._table(H, "sat") if idx is not None else rows).cuda()
    got = _on_off(switches, L, src, None if idx is None else idx.cuda(), mb)
    for form in (0, 1):
        on, off = got[form]
        assert bool((_slab(on, mb)[:mb // 32].view(torch.int32) == 0).all())
        _f64_bounds(f"sat mb {mb} sync {form}", L, (actor, critic), rows, ref, r32, off, mb)


@pytest.mark.parametrize("scaling", ("unit", "alt"))
def test_unsaturated_blocks_match(switches, scaling):
    """Case 2: unit-variance states, and rows alternating between saturated
    and small: no tile is all +-1, nothing may skip.  Equal outputs, and the
    slabs are not zero."""
    mb = 40
    L, actor, critic = arms._learner(H)
    if scaling == "alt":
        rows, _, ref, r32 = arms._refs(H, "alt", mb, False)
    else:
        rows = _unit_rows()[:mb]
        ref, r32 = reference_step_f64(actor, critic, rows), reference_full(actor, critic, rows, dtype=torch.float32)
    got = _on_off(switches, L, rows.cuda(), None, mb)
    for form in (0, 1):
        on, off = got[form]
        s = _slab(on, mb)
        for b in range(s.shape[0]):
            for net in (0, 1):
                assert bool((s[b, net, :, :19] != 0).any()), (b, net)
        _f64_bounds(f"{scaling} mb {mb} sync {form}", L, (actor, critic), rows, ref, r32, off, mb)


def _desaturating_state(actor, critic, j):
    """A state s (f32) with fc1 of the actor's tile j (units 16j .. 16j+15)
    at |z1| < 0.5 and every other unit of both nets at |z1| > 20, asserted in
    f64: s = -pinv(W_j) b_j + c v, v in the null space of W_j (two
    dimensions: the direction with the largest smallest |w . v| over the
    other units), c from 1e5 up."""
    W = torch.cat([n.fc1.weight.detach().double() for n in (actor, critic)])      # [2H][18]
    b = torch.cat([n.fc1.bias.detach().double() for n in (actor, critic)])
    tile = torch.zeros(2 * H, dtype=torch.bool)
    tile[16 * j:16 * j + 16] = True
    Wj, bj = W[tile], b[tile]
    s0 = -torch.linalg.pinv(Wj) @ bj
    null = torch.linalg.svd(Wj, full_matrices=True).Vh[16:]       # [2][18]
    assert float((Wj @ null.T).abs().max()) < 1e-12
    th = torch.arange(720, dtype=torch.float64) * (3.141592653589793 / 720)
    vs = torch.cos(th)[:, None] * null[0] + torch.sin(th)[:, None] * null[1]      # [720][18]
    v = vs[(vs @ W[~tile].T).abs().amin(1).argmax()]
    c = 1e5
    for _ in range(8):
        s = (s0 + c * v).float()
        z = (W @ s.double() + b).abs()
        if float(z[tile].max()) < 0.5 and float(z[~tile].min()) > 20.0:
            return s
        c *= 10.0
    raise AssertionError(f"tile {j}: no state found: tile max {float(z[tile].max())}, others min {float(z[~tile].min())}")


@pytest.mark.parametrize("j", (0, 15))
def test_one_desaturated_tile(switches, j):
    """Case 3: one row of a saturated block desaturates the actor's tile j
    only (wave j; 0 is the loss-head wave).  Equal outputs; the actor's slab
    rows of tile j's 16 columns are not all zero, every other slab row of
    both nets is +0.0 bytes."""
    mb = 32
    L, actor, critic = arms._learner(H)
    rows = arms._table(H, "sat")[:mb].clone()
    rows[7, 0:18] = _desaturating_state(actor, critic, j)
    # (the row's actor gradient must not vanish: at such a state the ratio is far outside the clip
    # range, and the surrogate keeps its gradient only on the side the sign of adv selects)
    ratio7 = float(reference_full(actor, critic, rows, dtype=torch.float32).ratio[7])
    rows[7, 24] = 1.0 if ratio7 < 1.0 else -1.0
    ref, r32 =reference_step_f64(actor, critic, rows), reference_full(actor, critic, rows, dtype=torch.float32)
    got = _on_off(switches, L, rows.cuda(), None, mb)
    for form in (0, 1):
        on, off = got[form]
        s = _slab(on, mb)[0]                                       # [net][H][20]
        tile = torch.zeros((2, H), dtype=torch.bool)
        tile[0, 16 * j:16 * j + 16] = True
        assert bool((s[tile] != 0).any()), "tile j multiplied"
        assert bool((s[~tile].view(torch.int32) == 0).all()), "every other wave's rows are +0.0"
        _f64_bounds(f"tile {j} sync {form}", L, (actor, critic), rows, ref, r32, off, mb, cancelling_row=7)


@pytest.mark.parametrize("column,value", ((24, float("inf")), (24, float("nan")), (24, 3e38), (25, float("inf"))))
def test_guard_dz2_magnitude(switches, column, value):
    """Case 4: a finite, saturated block with one row's adv (column 24) inf,
    NaN or 3e38, or its v_target (column 25) inf: dZ2 is not bounded, phase D
    runs and its non-finite dH1 reaches the slabs as in the full path."""
    mb = 32
    L, _, _ = arms._learner(H)
    rows = arms._table(H, "sat")[:mb].clone()
    rows[11, column] = value
    _on_off(switches, L, rows.cuda(), None, mb)


@pytest.mark.parametrize("weight,adv", ((float("inf"), None), (1e30, 1e12)))
def test_guard_w2_magnitude(switches, weight, adv):
    """Case 5: one fc2.weight element inf; and one at 1e30 with an adv of
    1e12 -- all finite, but the exponent bound refuses and phase D runs.  On
    the shared learner's parameters, restored afterwards."""
    mb = 32
    L, _, _ = arms._learner(H)
    rows = arms._table(H, "sat")[:mb].clone()
    if adv is not None:
        rows[11, 24] = adv
    saved = L.P.clone()
    try:
        L.flat_views(L.P)["actor.fc2.weight"].view(H, H)[3, 5] = weight
        L.flat_views(L.P)["critic.fc2.weight"].view(H, H)[200, 77] = weight
        L.sync_w2t()
        _on_off(switches, L, rows.cuda(), None, mb)
    finally:
        L.P.copy_(saved)
        L.sync_w2t()
        torch.cuda.synchronize()


def test_product_step_is_bitwise_the_full_path(switches):
    """Case 6: one eager FusedMinibatch step (rowpass, dW2, reduce, Adam) at
    mb 1056 -- 33 blocks of the 32-row kernel -- on saturated rows, under the
    switch at 1 and at 0, each on a fresh learner of the same weights: P, M
    and V are bytewise equal afterwards, and the rowpass error word is 0."""
    import satrl._lib as _L
    from satrl.ppo import FusedMinibatch, rowpass_exchange_check, step_plan
    _, dskip = switches
    mb = 1056
    assert step_plan(H, mb).rowpass == _L.RP_WG32_HANDOFF
    g = torch.Generator().manual_seed(5)
    rows = arms._table(H, "sat")[torch.arange(mb) % arms.B].clone()
    rows[:, 24] = torch.randn(mb, generator=g)
    rows[:, 25] = torch.randn(mb, generator=g) * 5
    src = rows.cuda()
    state = []
    for mode in (1, 0):
        dskip(mode)
        L, _, _ = pc.gpu_learner(H, mb=mb)
        st = FusedMinibatch(L, mb, 1, use_graph=False)
        before = L.P.clone()
        st.step(src, None)
        torch.cuda.synchronize()
        rowpass_exchange_check()
        assert bool((st.pw1.view(-1, 2 * H * 20)[:mb // 32].view(torch.int32) == 0).all())   # saturated: +0.0 slabs
        assert not torch.equal(L.P, before), "the step moved the parameters"
        state.append([t.clone() for t in (L.P, L.M, L.V)])
    for name, a, b in zip(("P", "M", "V"), *state):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
