"""Update diagnostics on the GPU (satrl_ppo_diagnostics, PPOLearner.diagnostics,
VecTrainer's diagnostics / target_kl keywords).

Kernel cases: H in {64, 128, 256}, nets and rows of ppo_cases (gpu_learner,
packed_rows with the sentinel 1e30 in the pad columns), n in {1, 31, 32, 33,
65} (around the 32-row block) and 4129 (130 blocks, a ragged last one), with
idx = None and with a shuffled idx whose last entry repeats its first.  Every
case runs the kernel twice, into NaN-poisoned scratch, and is checked
  bitwise against the update's own forward (satrl_ppo_rowpass_ratio's ratio,
    satrl_policy_value's v);
  for its reduction: the sums against exactly rounded f64 host sums of the
    slot definitions applied to rows_out and src (1e-12 relative: only the
    order of the f64 additions differs), counts and the max exact;
  for accuracy against the f64 reference under ppo_cases.bar(e32), e32 the
    error of the same forward in torch's f32 (diag_reference.py)."""
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import diag_reference as R
import ppo_cases as pc
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256)
SIZES = (1, 31, 32, 33, 65, 4129)
B = 4200                              # rows of the packed table
_CACHE = {}


def _case_idx(n, seed):
    """A shuffled index with a repeated row (n >= 2: the last entry = the first)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(B, generator=g)[:n].clone()
    if n >= 2:
        idx[-1] = idx[0]
    return idx


def _width(H):
    """Everything the kernel cases of width H share, computed once: the
    learner, the table, the f64 / f32 references over all B rows (per-row
    results do not depend on the batch), and each case's two runs."""
    if H in _CACHE:
        return _CACHE[H]
    from satrl.ppo import diagnostics_scratch, ppo_diagnostics
    L, actor, critic = pc.gpu_learner(H)
    assert float(L.epsilon) == pc.EPSILON
    src = pc.packed_rows(B, seed=3)
    assert bool((src[:, 26:] == pc.SENTINEL).all())
    W = {"L": L, "src": src, "src_dev": src.cuda(), "cases": {},
         "ref": R.reference(actor, critic, src, epsilon=pc.EPSILON, entropy_coef=L.entropy_coef),
         "r32": R.reference(actor, critic, src, epsilon=pc.EPSILON, entropy_coef=L.entropy_coef,
                            dtype=torch.float32),
         "log_std": actor.log_std.detach().double().numpy().reshape(-1)}
    for n in SIZES:
        for shuffled in (False, True):
            idx = _case_idx(n, 100 + n) if shuffled else None
            idx_dev = None if idx is None else idx.cuda()
            runs = []
            for _ in range(2):
                sums = torch.full((10,), float("nan"), dtype=torch.float64, device="cuda")
                scratch = torch.full((diagnostics_scratch(n) + 5,), float("nan"), dtype=torch.float64, device="cuda")
                rows_out = torch.full((n + 3, 4), float("nan"), device="cuda")
                ppo_diagnostics(H, W["src_dev"][:n] if idx is None else W["src_dev"], idx_dev, L.P, L.epsilon,
                                L.max_action, sums, scratch, rows_out)
                torch.cuda.synchronize()
                runs.append((sums.cpu().numpy(), rows_out.cpu(), scratch[-5:].cpu()))
            sel = torch.arange(n) if idx is None else idx
            W["cases"][(n, shuffled)] = dict(idx=idx_dev, sel=sel, runs=runs)
    _CACHE[H] = W
    return W


def _cases(W):
    for (n, shuffled), c in W["cases"].items():
        yield f"n {n}{' idx' if shuffled else ''}", n, c


@pytest.mark.parametrize("H", WIDTHS)
def test_rows_are_the_updates_own_bits(H):
    """rows_out[:, 0] == satrl_ppo_rowpass_ratio's ratio and rows_out[:, 2] ==
    satrl_policy_value on the rows' observations, bit for bit; rows_out[:, 1]
    is the argument of the ratio's expf (torch's device exp of it within
    2^-21 relative of the ratio: two f32 exp implementations, each within an
    ulp of the true value); column 3 is 0; rows past n and the scratch past
    its stated size stay as they were (NaN)."""
    from satrl.ppo import FusedMinibatch, policy_value, rowpass_exchange_check
    W = _width(H)
    L, src = W["L"], W["src_dev"]
    for tag, n, c in _cases(W):
        out = c["runs"][0][1]
        assert bool(torch.isnan(out[n:]).all()), tag
        assert bool(torch.isnan(c["runs"][0][2]).all()), tag
        assert not bool(torch.isnan(out[:n]).any()), tag
        st = FusedMinibatch(L, n, 1, use_graph=False)
        ratio = torch.full((n,), float("nan"), device="cuda")
        st.rowpass_ratio(src[:n] if c["idx"] is None else src, c["idx"], ratio)
        obs = src[c["sel"].cuda(), 0:18].contiguous()
        v = policy_value(H, obs, L.P, torch.full((n,), float("nan"), device="cuda"))
        e = torch.exp(out[:n, 1].cuda())
        torch.cuda.synchronize()
        assert torch.equal(out[:n, 0], ratio.cpu()), tag
        assert torch.equal(out[:n, 2], v.cpu()), tag
        assert bool((out[:n, 3] == 0).all()), tag
        q = float(((e.cpu().double() - out[:n, 0].double()).abs() / out[:n, 0].double()).max())
        assert q <= 2.0 ** -21, (tag, q)
    if H == 256:
        rowpass_exchange_check()


@pytest.mark.parametrize("H", WIDTHS)
def test_sums_are_the_slot_definitions_in_a_fixed_order(H):
    """Two calls give bitwise-equal sums and rows; the sums equal the exactly
    rounded f64 host sums of the slot definitions over rows_out and src
    (the products ratio * adv and clamp(ratio) * adv in f32 as in the kernel)
    at 1e-12 relative; rows, the clipped count and the max are exact."""
    W = _width(H)
    worst = 0.0
    for tag, n, c in _cases(W):
        (s0, out0, _), (s1, out1, _) = c["runs"]
        assert s0.tobytes() == s1.tobytes(), (tag, s0, s1)
        assert out0[:n].numpy().tobytes() == out1[:n].numpy().tobytes(), tag
        rows = W["src"][c["sel"]]
        out = out0[:n].numpy()
        want = R.sums_from_rows(out[:, 0], out[:, 1], out[:, 2], rows[:, 24].numpy(), rows[:, 25].numpy(),
                                pc.EPSILON, f32_products=True)
        for k, name in enumerate(R.SLOTS):
            if name in ("rows", "clipped", "ratio_max"):
                assert s0[k] == want[k], (tag, name, s0[k], want[k])
            else:
                err = abs(s0[k] - want[k]) / abs(want[k]) if want[k] != 0 else abs(s0[k])
                worst = max(worst, err)
                assert err <= 1e-12, (tag, name, s0[k], want[k], err)
        assert s0[0] == n
    print(f"H {H}: worst relative difference of a sum from the exactly rounded host sum {worst:.3e}")


def _bar_check(tag, got, ref64, ref32, bad):
    err, e32 = pc.rel_err(got, ref64), pc.rel_err(ref32, ref64)
    bar = pc.bar(e32)
    print(f"{tag}: err {err:.3e} e32 {e32:.3e} err/bar {err / bar:.3f}")
    if not err <= bar:
        bad.append((tag, err, e32, bar))
    return err / bar


@pytest.mark.parametrize("H", WIDTHS)
def test_accuracy_against_the_f64_reference(H):
    """Per row, ratio and v against the f64 reference under ppo_cases.bar(e32):
    err = max |got - ref64| / max |ref64| within max(8 e32, 2^-20), e32 the
    same error of torch's f32 forward.  The derived fields (from_sums of the
    kernel's sums against the reference's fields) under the same rule, each
    field a one-element tensor; explained_variance_after is NaN on both sides
    at n = 1.
    Measured on MI355X (H 64 / 128 / 256): worst err / bar per row 0.17 / 0.20 /
    0.16, over the derived fields 0.19 / 0.34 / 0.41 (mean_log_ratio at n 32,
    err 3.2e-7; explained_variance_after at n 33 idx, err 3.9e-7), every one
    under the floor 2^-20; the sums differ from the exactly rounded host sums
    by at most 5.3e-16 relative."""
    from satrl.ppo import UpdateDiagnostics
    W = _width(H)
    ref, r32 = W["ref"], W["r32"]
    bad, worst_rows, worst_fields = [], 0.0, 0.0
    for tag, n, c in _cases(W):
        sel = c["sel"]
        out = c["runs"][0][1][:n]
        worst_rows = max(worst_rows, _bar_check(f"H {H} {tag} ratio", out[:, 0], ref.ratio[sel], r32.ratio[sel], bad))
        worst_rows = max(worst_rows, _bar_check(f"H {H} {tag} v", out[:, 2], ref.v[sel], r32.v[sel], bad))
        rows = W["src"][sel].double().numpy()
        fields = {}
        for key, r in (("f64", ref), ("f32", r32)):
            s = R.sums_from_rows(r.ratio[sel].double().numpy(), r.d[sel].double().numpy(),
                                 r.v[sel].double().numpy(), rows[:, 24], rows[:, 25], pc.EPSILON)
            fields[key] = R.fields_from_sums(s, W["log_std"], W["L"].entropy_coef)
        got = UpdateDiagnostics.from_sums(c["runs"][0][0], W["log_std"], W["L"].entropy_coef).as_dict()
        assert got["rows"] == fields["f64"]["rows"] == n
        for name in R.FIELDS[1:]:
            w64, w32, g = fields["f64"][name], fields["f32"][name], got[name]
            if np.isnan(w64):
                assert n == 1 and name == "explained_variance_after" and np.isnan(g), (tag, name, g)
                continue
            worst_fields = max(worst_fields, _bar_check(f"H {H} {tag} {name}", torch.tensor([g]), torch.tensor([w64]),
                                                        torch.tensor([w32]), bad))
    print(f"H {H}: worst err / bar per row {worst_rows:.3f}, over the derived fields {worst_fields:.3f}")
    assert not bad, bad


@pytest.mark.parametrize("H", WIDTHS)
def test_branches_and_tie_rows(H):
    """ppo_cases.branch_rows (ratios 0.5 / 0.95 / 1.05 / 2 x adv -1 / 0 / +1,
    at least 1e-3 from the clip edges by the f64 reference alone): the clipped
    count is exactly the reference's.  The eight tie rows carry actions and
    log-probs of satrl_policy_act under the same parameters: on their own they
    give ratio 1.0f, log ratio 0 and kl 0 exactly."""
    from satrl.ppo import policy_act
    L, actor, critic = pc.gpu_learner(H, mb=32)
    n, nt = 32, pc.N_TIE
    rows0, _, _ = pc.branch_rows(actor, critic)
    obs = rows0[n - nt:, 0:18].cuda().contiguous()
    act, lp = torch.empty((nt, 3), device="cuda"), torch.empty((nt, 3), device="cuda")
    policy_act(H, obs, L.P, None, L.max_action, 5, 0, 0, act, lp)
    torch.cuda.synchronize()
    rows, want, adv = pc.branch_rows(actor, critic, tie=(act, lp))
    ref = R.reference(actor, critic, rows, epsilon=pc.EPSILON, entropy_coef=L.entropy_coef)
    assert pc.branch_margin(ref.ratio[:n - nt]) > 1e-3
    assert float((ref.ratio[n - nt:] - 1).abs().max()) < 1e-5           # the tie rows: far inside the clip range
    src = rows.cuda()
    out = torch.full((n, 4), float("nan"), device="cuda")
    d = L.diagnostics(src, rows_out=out)
    assert d.rows == n
    assert d.sums[4] == ref.sums[4] == 12.0                             # ratios 0.5 and 2 x three advs, twice
    assert d.clip_fraction == 12 / 32
    out = out.cpu()
    assert bool((out[n - nt:, 0] == 1.0).all()) and bool((out[n - nt:, 1] == 0.0).all()), out[n - nt:].tolist()
    tie = L.diagnostics(src, idx=torch.arange(n - nt, n, device="cuda"))
    assert tie.rows == nt and tie.approx_kl == 0.0 and tie.mean_log_ratio == 0.0
    assert tie.ratio_max == 1.0 and tie.clip_fraction == 0.0
    assert tie.policy_loss == -float(adv[n - nt:].double().mean()) == 0.0   # adv +1 / -1 alternating


def _trainer(**kw):
    from satrl.trainer import VecTrainer, args_param
    a = dict(batch_size=512, mini_batch_size=128, hidden_width=64, K_epochs=3, num_envs=64, horizon=8,
             max_episode_steps=4, max_train_steps=1000, seed=7, chkpt_dir="/tmp")
    a.update(kw)
    return VecTrainer(args_param(**a), flag=0, d_capture=15000.0, use_graphs=False)


def test_trainer_before_any_update_ratio_is_one():
    """After collect() + compute_advantages() the update's forward recomputes
    the rollout's log-probs bit for bit: no KL, nothing clipped, and the
    policy loss is minus the mean of the packed advantages."""
    tr = _trainer()
    tr.collect()
    tr.compute_advantages()
    d = tr.learner.diagnostics(tr.buf.packed)
    assert d.rows == 512
    assert d.approx_kl == 0.0 and d.clip_fraction == 0.0 and d.ratio_max == 1.0 and d.mean_log_ratio == 0.0
    want = -float(tr.buf.packed[:, 24].double().cpu().numpy().mean())
    assert abs(d.policy_loss - want) <= 1e-12 * abs(want), (d.policy_loss, want)
    vt, v = tr.buf.packed[:, 25].double().cpu().numpy(), tr.buf.values[:8].reshape(-1).double().cpu().numpy()
    assert abs(d.value_loss - ((v - vt) ** 2).mean()) <= 1e-12 * d.value_loss    # v: satrl_policy_value's bits


def _end_state(tr):
    L = tr.learner
    f, i = tr.env.get_state()
    return [L.P, L.M, L.V, L.steps, L.lr, f, i, tr.env.stats, tr.buf.obs[0], tr.gen.get_state()]


def test_diagnostics_do_not_perturb_training():
    """Two iterations with diagnostics=True, and two with target_kl=1e9
    (measured after every epoch, never stopping), end bit for bit where the
    same run without them ends."""
    base = _trainer()
    for _ in range(2):
        base.iteration()
    assert base.diagnostics == [] and base.last_diagnostics is None
    want = [t.cpu() for t in _end_state(base)]
    for kw in (dict(diagnostics=True), dict(target_kl=1e9), dict(diagnostics=True, diagnostics_rows=100)):
        tr = _trainer(**kw)
        stats = [tr.iteration() for _ in range(2)]
        assert stats[1].shape == base.env.stats.shape
        for k, (a, b) in enumerate(zip(_end_state(tr), want)):
            assert torch.equal(a.cpu(), b), (kw, k)
        assert len(tr.diagnostics) == 2 and tr.last_diagnostics is tr.diagnostics[1]
        for k, rec in enumerate(tr.diagnostics):
            assert rec["epochs_run"] == 3 and rec["iteration_count"] == k
            assert rec["rows"] == (100 if "diagnostics_rows" in kw else 512)
            assert list(rec)[:4] == ["iteration_count", "episodes", "epochs_run", "explained_variance"]
            assert list(rec)[4:] == R.FIELDS
            assert rec["approx_kl"] > 0 and rec["ratio_max"] > 1 and np.isfinite(rec["explained_variance"])
        assert tr.diagnostics[0]["episodes"] == 0.0 and tr.diagnostics[1]["episodes"] > 0


def test_target_kl_stops_the_epoch_loop():
    """target_kl=1e-12: every update stops after its first epoch (4 minibatch
    steps of 128 of the 512 rows); the lr decay still runs."""
    tr = _trainer(target_kl=1e-12)
    for _ in range(2):
        tr.iteration()
    L = tr.learner
    assert [r["epochs_run"] for r in tr.diagnostics] == [1, 1]
    assert all(r["approx_kl"] > 1e-12 for r in tr.diagnostics)
    assert L.steps.cpu().tolist() == [8.0, 8.0]
    ep = tr.diagnostics[1]["episodes"]                                   # the episode count the second update decayed with
    assert 0 < ep < 1000
    want = torch.tensor([L.lr_a * (1 - ep / 1000), L.lr_c * (1 - ep / 1000)], dtype=torch.float32)
    assert torch.equal(L.lr.cpu(), want) and float(want[0]) < L.lr_a


def test_sampled_rows_are_the_epochs_first_permutation_entries():
    tr = _trainer(diagnostics=True, diagnostics_rows=100, K_epochs=2)
    perms, draw = [], tr.epoch_perm
    tr.epoch_perm = lambda: (perms.append(draw()), perms[-1])[1]
    tr.collect()
    tr.compute_advantages()
    tr.update()
    assert len(perms) == 2
    rec = tr.last_diagnostics
    assert rec["rows"] == 100 and rec["epochs_run"] == 2
    direct = tr.learner.diagnostics(tr.buf.packed, perms[-1][:100].contiguous()).as_dict()
    assert {k: rec[k] for k in R.FIELDS} == direct
    assert tr.learner.diagnostics(tr.buf.packed).rows == 512
    with pytest.raises(ValueError):
        _trainer(diagnostics_rows=513)


def _dp_rank(rank, port, q):
    sys.path.insert(0, PKG_DIR)
    import torch.distributed as dist
    from test_dp_gpu import _global_mb_args
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        from satrl.trainer import VecTrainer
        tr = VecTrainer(_global_mb_args(32, diagnostics=True), flag=0, d_capture=15000.0, pg=dist.group.WORLD,
                        env_offset=rank * 32)
        tr.iteration()
        torch.cuda.synchronize()
        q.put((rank, tr.last_diagnostics, tr.learner.P.cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_record_the_same_diagnostics():
    """The two-ranks-on-one-device setting of tests/test_dp_gpu.py (gloo over
    CUDA tensors, its _global_mb_args): the sums are reduced over the ranks, so
    both record identical dicts over the 2 x 32 x 24 rows."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_dp_rank, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (d, P) for r, d, P in (q.get(timeout=300) for _ in procs)}
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert (res[0][1] == res[1][1]).all()
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert res[0][0]["rows"] == 2 * 32 * 24 and res[0][0]["epochs_run"] == 2
