"""Host side of the update diagnostics (no GPU): the argument checks of
satrl_ppo_diagnostics, UpdateDiagnostics.from_sums on hand-written sums, the
numpy reference (diag_reference.py) on four hand-placed rows, and the
reduction of the sums over two ranks (gloo)."""
import ctypes as C
import math
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import diag_reference as R
import ppo_cases as pc
from conftest import PKG_DIR
from torch_reference import reference_step_f64


def test_diagnostics_rejects_bad_arguments_before_any_device_call():
    """Every rejection returns -1 on the host; the fake non-null pointer is
    never dereferenced (a launch would fail with -2 on a host without a GPU)."""
    import satrl._lib as L
    lib = L.lib()
    fake = C.c_void_p(16)

    def dg(H=256, n=64, src=fake, idx=None, P=fake, sums=fake, scratch=fake, slen=None, rows=None):
        slen = lib.satrl_ppo_diagnostics_scratch(max(int(n), 1)) if slen is None else slen
        return lib.satrl_ppo_diagnostics(H, n, src, idx, P, 0.1, 1.6, sums, scratch, slen, rows, None)

    assert dg(H=100) == -1 and dg(H=0) == -1 and dg(H=512) == -1        # H not 64 / 128 / 256
    assert dg(n=0) == -1 and dg(n=-5) == -1
    assert dg(src=None) == -1 and dg(P=None) == -1 and dg(sums=None) == -1 and dg(scratch=None) == -1
    for H in (64, 128, 256):
        for n in (1, 32, 33, 4129, 32 * 4096 + 1):
            need = lib.satrl_ppo_diagnostics_scratch(n)
            assert dg(H=H, n=n, slen=need - 1) == -1 and dg(H=H, n=n, slen=0) == -1, (H, n)
            assert dg(H=H, n=n, idx=fake, rows=fake, slen=need - 1) == -1
    assert dg(n=2 ** 31) == -1                                           # rows are indexed in 32 bits
    assert b"satrl_ppo_diagnostics" in lib.satrl_ppo_last_error()
    # a line of 16 f64 per 32-row block; above 4096 blocks one more per 4096 of them
    sc = lib.satrl_ppo_diagnostics_scratch
    assert [sc(n) for n in (1, 32, 33, 65, 4129)] == [16, 16, 32, 48, 16 * 130]
    assert sc(32 * 4096) == 16 * 4096 and sc(32 * 4096 + 1) == 16 * (4097 + 2)
    assert sc(0) == -1 and sc(-1) == -1 and sc(2 ** 31) == -1
    for name in ("satrl_ppo_diagnostics", "satrl_ppo_diagnostics_scratch"):
        assert name in L.exported_symbols() and hasattr(lib, name)


def test_from_sums_on_hand_written_sums():
    from satrl.ppo import DIAG_SLOTS, ENT_CONST, UpdateDiagnostics
    assert DIAG_SLOTS == R.SLOTS and list(UpdateDiagnostics.FIELDS) == R.FIELDS
    #       rows surr  kl  log r clip max verr2 verr  vt    vt2
    sums = [4.0, 2.0, 0.5, -0.25, 1.0, 3.0, 8.0, 2.0, 10.0, 30.0]
    d = UpdateDiagnostics.from_sums(sums, [0.5, -0.25, 0.25], 0.01)
    ent = 0.5 + 3 * ENT_CONST
    assert ENT_CONST == 0.5 + 0.5 * math.log(2 * math.pi)
    assert d.rows == 4 and isinstance(d.rows, int)
    assert d.policy_loss == -0.5
    assert d.entropy == ent
    assert d.actor_loss == -0.5 - 0.01 * ent
    assert d.value_loss == 2.0
    assert d.approx_kl == 0.125
    assert d.mean_log_ratio == -0.0625
    assert d.clip_fraction == 0.25
    assert d.ratio_max == 3.0
    assert d.explained_variance_after == 1.0 - (8.0 / 4 - 0.5 ** 2) / (30.0 / 4 - 2.5 ** 2)    # 1 - 1.75 / 1.25
    assert d.as_dict() == {k: getattr(d, k) for k in R.FIELDS} and list(d.as_dict()) == R.FIELDS
    assert isinstance(d.sums, np.ndarray) and d.sums.dtype == np.float64 and d.sums.tolist() == sums
    ref = R.fields_from_sums(sums, [0.5, -0.25, 0.25], 0.01)
    assert ref == d.as_dict()
    # a constant v_target: Var(vt) = 0, the explained variance is undefined
    flat = UpdateDiagnostics.from_sums([4.0, 2.0, 0.5, -0.25, 1.0, 3.0, 8.0, 2.0, 8.0, 16.0], [0.0, 0.0, 0.0], 0.0)
    assert math.isnan(flat.explained_variance_after) and flat.value_loss == 2.0
    assert flat.entropy == 3 * ENT_CONST and flat.actor_loss == flat.policy_loss
    assert math.isnan(R.fields_from_sums(flat.sums, [0.0] * 3, 0.0)["explained_variance_after"])
    with pytest.raises(ValueError):
        UpdateDiagnostics.from_sums(sums[:9], [0.0] * 3, 0.0)
    with pytest.raises(ValueError):
        UpdateDiagnostics.from_sums([0.0] * 10, [0.0] * 3, 0.0)


def test_reference_on_four_hand_placed_rows():
    """Ratios 0.5, 1, 1.05, 2 (placed as ppo_cases.branch_rows places them:
    old log-probs = the f64 reference's own minus log(ratio) / 3 per
    dimension), adv +1, -1, +2, +1, v_target = v + (1, -1, 2, 0); epsilon 0.1.
    By hand: min(s1, s2) = 0.5, -1, 2.1, 1.1 (sum 2.7); kl terms (r - 1) -
    log r sum to 0.55 - log 1.05; the log ratios to log 1.05; rows 0 and 3 are
    clipped; (v - vt)^2 sums to 6 and vt - v to 2.  The old log-probs are
    rounded to f32 (the packed table's type), so the ratios are their targets
    to ~1e-6."""
    actor, critic = pc.cpu_nets(64)
    want = torch.tensor([0.5, 1.0, 1.05, 2.0], dtype=torch.float64)
    adv = torch.tensor([1.0, -1.0, 2.0, 1.0])
    dv = torch.tensor([1.0, -1.0, 2.0, 0.0])
    rows = pc._near_policy_rows(actor, critic, 4, seed=5)
    rows[:, 21:24] = 0.0
    ref0 = reference_step_f64(actor, critic, rows)
    rows[:, 21:24] = (ref0.logp - (want.log() / 3.0)[:, None]).float()
    rows[:, 24] = adv
    rows[:, 25] = (ref0.v + dv.double()).float()
    assert bool((rows[:, 26:] == pc.SENTINEL).all())
    ref = R.reference(actor, critic, rows, epsilon=pc.EPSILON, entropy_coef=0.01)
    assert torch.allclose(ref.ratio, want, rtol=1e-5, atol=0)
    s = dict(zip(R.SLOTS, ref.sums))
    assert s["rows"] == 4.0 and s["clipped"] == 2.0
    assert s["surr"] == pytest.approx(2.7, abs=2e-5)
    assert s["kl"] == pytest.approx(0.55 - math.log(1.05), abs=2e-5)
    assert s["log_ratio"] == pytest.approx(math.log(1.05), abs=2e-5)
    assert s["ratio_max"] == pytest.approx(2.0, rel=1e-5)
    assert s["verr2"] == pytest.approx(6.0, abs=1e-5) and s["verr"] == pytest.approx(2.0, abs=1e-5)
    vt = rows[:, 25].double().numpy()
    assert s["vt"] == pytest.approx(vt.sum(), rel=1e-14) and s["vt2"] == pytest.approx((vt ** 2).sum(), rel=1e-14)
    f = ref.fields
    assert f["rows"] == 4 and f["clip_fraction"] == 0.5
    assert f["ratio_max"] == pytest.approx(2.0, rel=1e-5)
    assert f["policy_loss"] == pytest.approx(-0.675, abs=1e-5)
    assert f["approx_kl"] == pytest.approx((0.55 - math.log(1.05)) / 4, abs=1e-5)
    assert f["mean_log_ratio"] == pytest.approx(math.log(1.05) / 4, abs=1e-5)
    assert f["value_loss"] == pytest.approx(1.5, abs=1e-5)
    ent = float(actor.log_std.detach().double().sum()) + 3 * R.ENT_CONST
    assert f["entropy"] == pytest.approx(ent, rel=1e-15)
    assert f["actor_loss"] == pytest.approx(f["policy_loss"] - 0.01 * ent, rel=1e-15)
    e = vt - ref.v.numpy()
    assert f["explained_variance_after"] == pytest.approx(1 - e.var() / vt.var(), rel=1e-9)
    # the f32 products of the kernel's expressions give the same sums up to f32 rounding
    s32 = R.sums_from_rows(ref.ratio.float().numpy(), ref.d.float().numpy(), ref.v.float().numpy(),
                           rows[:, 24].numpy(), rows[:, 25].numpy(), pc.EPSILON, f32_products=True)
    assert s32[0] == 4.0 and s32[4] == 2.0
    assert np.allclose(s32, ref.sums, rtol=1e-5, atol=1e-5)
    # the f32 measuring stick: the same forward in torch's f32
    r32 = R.reference(actor, critic, rows, epsilon=pc.EPSILON, entropy_coef=0.01, dtype=torch.float32)
    assert r32.ratio.dtype == torch.float32 and r32.sums.dtype == np.float64
    assert np.allclose(r32.sums, ref.sums, rtol=1e-4, atol=1e-4)


def _reduce_rank(rank, port, q):
    sys.path.insert(0, PKG_DIR)
    import torch.distributed as dist
    from satrl.ppo import reduce_diagnostics_sums
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        mine = torch.tensor(_RANK_SUMS[rank], dtype=torch.float64)
        keep = mine.clone()
        out = reduce_diagnostics_sums(mine, dist.group.WORLD)
        assert torch.equal(mine, keep)                                   # a new tensor
        q.put((rank, out.numpy()))
    finally:
        dist.destroy_process_group()


_RANK_SUMS = ([4.0, 2.0, 0.5, -0.25, 1.0, 3.0, 8.0, 2.0, 10.0, 30.0],
              [6.0, -1.0, 0.25, 0.75, 0.0, 1.5, 1.0, -3.0, 2.0, 5.0])


def test_sums_reduce_over_two_ranks_gloo():
    """The additive slots are summed, the max slot maxed; both ranks get the
    same bits.  One process: the identity (a copy)."""
    from satrl.ppo import DIAG_MAX_SLOT, reduce_diagnostics_sums
    assert R.SLOTS[DIAG_MAX_SLOT] == "ratio_max"
    one = torch.tensor(_RANK_SUMS[0], dtype=torch.float64)
    alone = reduce_diagnostics_sums(one, None)
    assert torch.equal(alone, one) and alone.data_ptr() != one.data_ptr()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_reduce_rank, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = [10.0, 1.0, 0.75, 0.5, 1.0, 3.0, 9.0, -1.0, 12.0, 35.0]
    assert res[0].tolist() == want and res[1].tolist() == want
