"""Running observation normalisation and reward scaling on the GPU: the two
kernels of include/satrl_rollout.h (satrl_obs_normalize, satrl_return_scan)
against numpy restatements, and VecTrainer with obs_norm / reward_scaling."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEANS = np.tile(np.array([2e6, 2e6, 1e6, 1710.0, 1140.0, 1300.0]), 3)
SPREADS = np.tile(np.array([1e4, 5e4, 1e3, 1.0, 0.5, 2.0]), 3)
CONST_F = 7                            # one feature is constant
PAD = 64                               # sentinel elements on either side of a guarded buffer
OBS_SHAPES = [1, 31, 32, 33, 64, 257, 1000, 4113]     # slot edges; a workgroup is one slot


def _raw(N, seed):
    """Raw-scale rows f32 [N,18]: one constant feature, every fifth row 50 spreads out."""
    rng = np.random.default_rng(seed)
    x = MEANS + SPREADS * rng.standard_normal((N, 18))
    x[::5] += 50.0 * SPREADS * rng.choice([-1.0, 1.0], (len(x[::5]), 18))
    x[:, CONST_F] = MEANS[CONST_F]
    return x.astype(np.float32)


def _stats(seed):
    rng = np.random.default_rng(1000 + seed)
    mean = (MEANS + 0.3 * SPREADS * rng.standard_normal(18)).astype(np.float32)
    inv = (1.0 / (SPREADS * rng.uniform(0.8, 1.25, 18) + 1e-8)).astype(np.float32)
    mean[CONST_F], inv[CONST_F] = np.float32(MEANS[CONST_F]), np.float32(1e8)
    pivot = (MEANS + SPREADS * rng.standard_normal(18)).astype(np.float32)
    return np.stack([mean, inv]), pivot


def _np_normalize(x, st, clip):
    y = (x - st[0]) * st[1]                                  # f32: one subtract, one multiply
    assert y.dtype == np.float32
    return np.clip(y, np.float32(-clip), np.float32(clip)) if clip > 0 else y


def _np_slot_sums(x, pivot):
    """f64 [slots,2,18] sums of d and d*d, and the sums of the terms' magnitudes."""
    d = x.astype(np.float64) - pivot.astype(np.float64)
    k = (x.shape[0] + 31) // 32
    s, mag = np.zeros((k, 2, 18)), np.zeros((k, 2, 18))
    for j in range(k):
        b = d[32 * j:32 * j + 32]
        s[j, 0], s[j, 1] = b.sum(0), (b * b).sum(0)
        mag[j, 0], mag[j, 1] = np.abs(b).sum(0), (b * b).sum(0)
    return s, mag


def _guarded(n, dtype, fill):
    """A buffer of n elements between two sentinel pads (the view starts 16-byte aligned)."""
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return whole, whole[PAD:PAD + n]


def _pads_intact(whole, n, fill):
    w = whole.cpu()
    return bool((w[:PAD] == fill).all() and (w[PAD + n:] == fill).all())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("clip", [10.0, 0.0])
@pytest.mark.parametrize("N", OBS_SHAPES)
def test_obs_normalize_values_and_accumulators(N, clip):
    from satrl import norm
    x = _raw(N, N)
    st, pivot = _stats(N)
    raw, stats, piv = _t(x), _t(st), _t(pivot)
    slots = (N + 31) // 32
    ow, out = _guarded(N * 18, torch.float32, -7.0)
    aw, acc = _guarded(slots * 36, torch.float64, 0.0)       # (zero pads: acc is added to)
    out, acc = out.view(N, 18), acc.view(slots, 2, 18)
    norm.obs_normalize(raw, stats, clip, out, piv, acc)
    torch.cuda.synchronize()
    ref = _np_normalize(x, st, clip)
    if clip > 0:
        assert (np.abs(ref) == np.float32(clip)).any() and (np.abs(ref) < np.float32(clip)).any()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    s, mag = _np_slot_sums(x, pivot)
    err = np.abs(acc.cpu().numpy() - s)
    print("acc err / sum|terms| max:", (err / np.maximum(mag, 1e-300)).max())
    assert (err <= 1e-12 * mag).all()
    assert _pads_intact(ow, N * 18, -7.0) and _pads_intact(aw, slots * 36, 0.0)
    assert np.array_equal(raw.cpu().numpy(), x) and np.array_equal(stats.cpu().numpy(), st)
    # acc = NULL: nothing but out is written
    ow2, out2 = _guarded(N * 18, torch.float32, -7.0)
    before = acc.clone()
    norm.obs_normalize(raw, stats, clip, out2.view(N, 18))
    torch.cuda.synchronize()
    assert np.array_equal(out2.view(N, 18).cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert _pads_intact(ow2, N * 18, -7.0) and torch.equal(acc, before)
    assert np.array_equal(raw.cpu().numpy(), x) and np.array_equal(piv.cpu().numpy(), pivot)


@pytest.mark.parametrize("N", [33, 257])
def test_obs_normalize_rows_off_the_16_byte_boundary(N):
    """Row buffers that start 8 bytes past a 16-byte boundary (buf.obs[t] of
    an odd env count) take the element-wise path: same bits, same bounds."""
    from satrl import norm
    x = _raw(N, 5 * N)
    st, pivot = _stats(N)
    rw = torch.full((N * 18 + 2 * PAD,), 3.0, dtype=torch.float32, device=DEV)
    raw = rw[PAD + 2:PAD + 2 + N * 18].view(N, 18)
    raw.copy_(_t(x))
    ow = torch.full((N * 18 + 2 * PAD,), -7.0, dtype=torch.float32, device=DEV)
    out = ow[PAD + 2:PAD + 2 + N * 18].view(N, 18)
    assert raw.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 8
    acc = torch.zeros(((N + 31) // 32, 2, 18), dtype=torch.float64, device=DEV)
    norm.obs_normalize(raw, _t(st), 10.0, out, _t(pivot), acc)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _np_normalize(x, st, 10.0).view(np.uint32))
    o = ow.cpu()
    assert (o[:PAD + 2] == -7.0).all() and (o[PAD + 2 + N * 18:] == -7.0).all()
    s, mag = _np_slot_sums(x, pivot)
    assert (np.abs(acc.cpu().numpy() - s) <= 1e-12 * mag).all()


def test_obs_normalize_determinism_and_stream_order():
    from satrl import norm
    N = 257
    x = _raw(N, 9)
    st, pivot = _stats(9)
    raw, stats, piv = _t(x), _t(st), _t(pivot)
    out = torch.empty((N, 18), dtype=torch.float32, device=DEV)
    accs = [torch.zeros((9, 2, 18), dtype=torch.float64, device=DEV) for _ in range(3)]
    for a in accs[:2]:                                       # two runs of eight stream-ordered calls
        for _ in range(8):
            norm.obs_normalize(raw, stats, 10.0, out, piv, a)
    torch.cuda.synchronize()
    assert torch.equal(accs[0], accs[1])
    s, mag = _np_slot_sums(x, pivot)
    assert (np.abs(accs[0].cpu().numpy() - 8.0 * s) <= 1e-12 * 8.0 * mag).all()
    # a graph that captured one call, replayed eight times
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        norm.obs_normalize(raw, stats, 10.0, out, piv, accs[2])
    accs[2].zero_()
    for _ in range(8):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(accs[2], accs[0])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _np_normalize(x, st, 10.0).view(np.uint32))
    # the statistics are read from device memory on every launch
    st2, _ = _stats(10)
    stats.copy_(_t(st2))
    g.replay()
    torch.cuda.synchronize()
    ref2 = _np_normalize(x, st2, 10.0)
    assert not np.array_equal(ref2, _np_normalize(x, st, 10.0))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref2.view(np.uint32))


def test_obs_normalize_shard_writes_the_unsharded_slots():
    from satrl import norm
    x = _raw(64, 21)
    st, pivot = _stats(21)
    raw, stats, piv = _t(x), _t(st), _t(pivot)
    out = torch.empty((64, 18), dtype=torch.float32, device=DEV)
    one = torch.zeros((2, 2, 18), dtype=torch.float64, device=DEV)
    two = torch.zeros((2, 2, 18), dtype=torch.float64, device=DEV)
    norm.obs_normalize(raw, stats, 10.0, out, piv, one)
    norm.obs_normalize(raw[:32], stats, 10.0, out[:32], piv, two[0:1])
    norm.obs_normalize(raw[32:], stats, 10.0, out[32:], piv, two[1:2])
    torch.cuda.synchronize()
    assert torch.equal(one, two) and bool((one != 0).any())


# -- return scan ----------------------------------------------------------------------
def _scan_case(T, N, seed):
    rng = np.random.default_rng(seed)
    r = rng.normal(0.0, 30.0, (T, N)).astype(np.float32)
    done = (rng.random((T, N)) < 0.2).astype(np.uint8)
    done[0, 0] = 1
    done[T - 1, N - 1] = 1
    carry = rng.normal(0.0, 100.0, N)
    return r, done, carry


def _np_scan(r, done, gamma, carry):
    """R = gamma * R + r per env in f64 (a multiply, then an add), R = 0 after done."""
    T, N = r.shape
    R = carry.astype(np.float64).copy()
    allR = np.zeros((T, N))
    for t in range(T):
        R = gamma * R + r[t].astype(np.float64)
        allR[t] = R
        R = np.where(done[t] != 0, 0.0, R)
    k = (N + 31) // 32
    s, mag = np.zeros((k, 2)), np.zeros((k, 2))
    for j in range(k):
        b = allR[:, 32 * j:32 * j + 32]
        s[j] = b.sum(), (b * b).sum()
        mag[j] = np.abs(b).sum(), (b * b).sum()
    return R, s, mag, allR


@pytest.mark.parametrize("N", [1, 33, 257])
@pytest.mark.parametrize("T", [1, 2, 9, 64])
def test_return_scan_matches_the_f64_loop(T, N):
    from satrl import norm
    gamma = 0.99
    r, done, carry0 = _scan_case(T, N, 100 * T + N)
    slots = (N + 31) // 32
    cw, carry = _guarded(N, torch.float64, 5.0)
    aw, acc = _guarded(slots * 2, torch.float64, 0.0)
    carry.copy_(_t(carry0))
    acc = acc.view(slots, 2)
    rew, dn = _t(r), _t(done)
    norm.return_scan(rew, dn, gamma, carry, acc)
    torch.cuda.synchronize()
    R, s, mag, _ = _np_scan(r, done, gamma, carry0)
    assert np.array_equal(carry.cpu().numpy().view(np.uint64), R.view(np.uint64))
    err = np.abs(acc.cpu().numpy() - s)
    print("acc err / sum|terms| max:", (err / np.maximum(mag, 1e-300)).max())
    assert (err <= 1e-12 * mag).all()
    assert _pads_intact(cw, N, 5.0) and _pads_intact(aw, slots * 2, 0.0)
    assert np.array_equal(rew.cpu().numpy(), r) and np.array_equal(dn.cpu().numpy(), done)
    if T % 2 == 0:                                           # two scans of T/2 chained through carry
        c2 = _t(carry0)
        a2 = torch.zeros((slots, 2), dtype=torch.float64, device=DEV)
        norm.return_scan(rew[:T // 2], dn[:T // 2], gamma, c2, a2)
        norm.return_scan(rew[T // 2:], dn[T // 2:], gamma, c2, a2)
        torch.cuda.synchronize()
        assert torch.equal(c2, carry)
        assert (np.abs(a2.cpu().numpy() - s) <= 1e-12 * mag).all()


# -- VecTrainer ------------------------------------------------------------------------
def _args(**kw):
    from satrl.trainer import args_param
    base = dict(chkpt_dir="/tmp", batch_size=64 * 24, mini_batch_size=128, hidden_width=64, K_epochs=1, num_envs=64,
                horizon=24, max_episode_steps=10, seed=5, rollout_graph_chunk=8, update_graph_group=2)
    base.update(kw)
    return args_param(**base)


def _norm_args(**kw):
    return _args(obs_norm=True, reward_scaling=True, **kw)


def _env_snapshot(tr):
    f, i = tr.env.get_state()
    torch.cuda.synchronize()
    return f.clone(), i.clone(), tr.env.stats.clone(), tr.rollout_steps


@pytest.fixture(scope="module")
def run():
    """One eager iteration of a trainer with both keywords on, with the two
    wrappers of satrl.norm and the trainer's gae recording what they are handed."""
    from satrl import norm, trainer
    from satrl.trainer import VecTrainer
    rec = {"norm": [], "scan": [], "gae": []}
    real_n, real_s, real_g = norm.obs_normalize, norm.return_scan, trainer.gae

    def obs_normalize(raw, stats, clip, out, pivot=None, acc=None):
        rec["norm"].append(dict(raw=raw.clone(), stats=stats.clone(), clip=clip, out=out,
                                pivot=None if pivot is None else pivot.clone(), acc=acc is not None))
        return real_n(raw, stats, clip, out, pivot, acc)

    def return_scan(rew, done, gamma, carry, acc):
        rec["scan"].append(dict(rew=rew.clone(), done=done.clone(), gamma=gamma, carry=carry.clone()))
        return real_s(rew, done, gamma, carry, acc)

    def gae(rew, *a, **k):
        rec["gae"].append(rew.clone())
        return real_g(rew, *a, **k)

    norm.obs_normalize, norm.return_scan, trainer.gae = obs_normalize, return_scan, gae
    try:
        tr = VecTrainer(_norm_args(), flag=0, d_capture=15000.0, use_graphs=False)
        built = dict(calls=len(rec["norm"]), env=_env_snapshot(tr), stats=tr.obs_stats.clone(),
                     obs0=tr.buf.obs[0].clone(), rms=copy.deepcopy(tr.obs_rms.state_dict()))
        tr.iteration()
        torch.cuda.synchronize()
        assert tr.env.check_errors() == 0
    finally:
        norm.obs_normalize, norm.return_scan, trainer.gae = real_n, real_s, real_g
    return tr, rec, built


def _moments_ld(rows):
    x = np.concatenate(rows).astype(np.longdouble)
    mean = x.mean(0)
    return mean, np.sqrt(((x - mean) ** 2).mean(0)), np.abs(x).max(0)


def test_trainer_obs_norm_iteration(run):
    from satrl.trainer import VecTrainer
    tr, rec, built = run
    T, calib = 24, 64
    calls = rec["norm"]
    # construction: the reset row, `calib` accumulating steps under the identity, the reset row again
    assert built["calls"] == calib + 2 and len(calls) == built["calls"] + T + 1
    assert [c["acc"] for c in calls] == [False] + [True] * calib + [False] + [True] * T + [False]
    ident = np.stack([np.zeros(18, np.float32), np.ones(18, np.float32)])
    for c in calls[:calib + 1]:
        assert np.array_equal(c["stats"].cpu().numpy(), ident)
    for c in calls[1:calib + 1]:
        assert torch.equal(c["pivot"], calls[0]["raw"][0])            # row 0 of the reset observation
    # the iteration: frozen statistics, buf.obs[t+1] = the recorded raw row normalised, bit for bit
    step = calls[built["calls"]:built["calls"] + T]
    frozen = built["stats"].cpu().numpy()
    buf_obs = tr.buf.obs.cpu().numpy()
    for t, c in enumerate(step):
        assert torch.equal(c["stats"], built["stats"]) and c["clip"] == 10.0
        assert c["out"].data_ptr() == tr.buf.obs[t + 1].data_ptr()
        ref = _np_normalize(c["raw"].cpu().numpy(), frozen, 10.0)
        assert np.array_equal(buf_obs[t + 1].view(np.uint32), ref.view(np.uint32)), t
    assert (np.abs(buf_obs) <= np.float32(10.0)).all()
    assert np.abs(buf_obs).max() > 0.05 and not np.array_equal(frozen, ident)
    # calibration statistics, then the merged ones, against long-double moments of the recorded rows
    rows_c = [c["raw"].cpu().numpy() for c in calls[1:calib + 1]]
    rows_i = [c["raw"].cpu().numpy() for c in step]
    for rows, n, mean, M2 in ((rows_c, built["rms"]["n"], built["rms"]["mean"], built["rms"]["M2"]),
                              (rows_c + rows_i, tr.obs_rms.n, tr.obs_rms.mean, tr.obs_rms.M2)):
        rm, rs, xmax = _moments_ld(rows)
        assert float(n) == 64 * len(rows)
        std = np.sqrt(M2 / float(n))
        em, es = np.abs(mean.astype(np.longdouble) - rm), np.abs(std.astype(np.longdouble) - rs)
        print("mean err / max|x|:", (em / xmax).max(), " std rel err:", (es / np.maximum(rs, 1e-300)).max())
        assert (em <= 1e-13 * xmax).all()
        assert (es <= 1e-10 * rs).all()
    new = tr.obs_rms.device_stats()
    assert np.array_equal(tr.obs_stats.cpu().numpy(), new) and np.array_equal(tr.obs_pivot.cpu().numpy(), new[0])
    assert not np.array_equal(new, frozen)
    assert float(tr.obs_acc.abs().sum()) == 0.0
    # buf.obs[0] is the last raw row under the new statistics
    last = calls[-1]
    assert torch.equal(last["raw"], step[-1]["raw"]) and torch.equal(last["raw"], tr.obs_raw)
    assert np.array_equal(buf_obs[0].view(np.uint32),
                          _np_normalize(last["raw"].cpu().numpy(), new, 10.0).view(np.uint32))
    assert np.array_equal(built["obs0"].cpu().numpy().view(np.uint32),
                          _np_normalize(calls[0]["raw"].cpu().numpy(), frozen, 10.0).view(np.uint32))
    # the calibration left the env where a trainer without it starts
    tr0 = VecTrainer(_norm_args(obs_norm_calib_steps=0), flag=0, d_capture=15000.0, use_graphs=False)
    f0, i0, st0, steps0 = _env_snapshot(tr0)
    f, i, st, steps = built["env"]
    assert torch.equal(f, f0) and torch.equal(i, i0) and torch.equal(st, st0) and steps == steps0 == 0
    assert np.array_equal(tr0.obs_stats.cpu().numpy(), ident) and tr0.obs_rms.n == 0


def test_trainer_reward_scaling(run):
    tr, rec, _ = run
    assert len(rec["scan"]) == 1 and len(rec["gae"]) == 1
    sc = rec["scan"][0]
    rew, done = tr.buf.rew.cpu().numpy(), tr.buf.done.cpu().numpy()
    assert np.array_equal(sc["rew"].cpu().numpy(), rew) and np.array_equal(sc["done"].cpu().numpy(), done)
    assert sc["gamma"] == 0.99 and float(sc["carry"].abs().sum()) == 0.0
    R, _, _, allR = _np_scan(rew, done, 0.99, np.zeros(64))
    std = np.std(allR)
    scale = np.float32(1.0 / (std + 1e-8))
    assert done.any() and std > 0
    assert np.array_equal(rec["gae"][0].cpu().numpy().view(np.uint32), (rew * scale).view(np.uint32))
    assert torch.equal(tr.rew_s, rec["gae"][0])
    assert np.array_equal(tr.ret_carry.cpu().numpy().view(np.uint64), R.view(np.uint64))
    assert tr.ret_rms.n == 24 * 64 and float(tr.ret_rms.std()) == pytest.approx(std, rel=1e-12)
    assert float(tr.ret_acc.abs().sum()) == 0.0


def test_trainer_graphs_match_eager():
    from satrl.trainer import VecTrainer
    res = []
    for graphs in (True, False):
        tr = VecTrainer(_norm_args(), flag=0, d_capture=15000.0, use_graphs=graphs)
        tr.collect()
        torch.cuda.synchronize()
        b = tr.buf
        got = [b.obs.clone(), b.act.clone(), b.logp.clone(), b.rew.clone(), b.done.clone()]
        tr.compute_advantages()
        tr.finish_iteration()
        torch.cuda.synchronize()
        got += [tr.obs_stats.clone(), tr.obs_pivot.clone(), tr.ret_carry.clone(), b.obs[0].clone(),
                torch.from_numpy(tr.obs_rms.mean), torch.from_numpy(tr.obs_rms.M2),
                torch.tensor([tr.obs_rms.n, tr.ret_rms.n, float(tr.ret_rms.mean), float(tr.ret_rms.M2)],
                             dtype=torch.float64)]
        res.append(got)
    for k, (a, b_) in enumerate(zip(*res)):
        assert torch.equal(a, b_), k
    assert res[0][-1][0] == 64 * (64 + 24)


def _tensor_names(tr):
    return {k for k, v in vars(tr).items() if torch.is_tensor(v)}


def test_trainer_keywords_off_is_the_default_engine():
    from satrl.trainer import VecTrainer
    res = []
    for kw in (dict(obs_norm=False, reward_scaling=False), {}):
        tr = VecTrainer(_args(**kw), flag=0, d_capture=15000.0)
        tr.collect()
        torch.cuda.synchronize()
        res.append((tr.buf.obs.clone(), tr.buf.rew.clone(), tr.buf.done.clone(), _tensor_names(tr)))
    for k in range(3):
        assert torch.equal(res[0][k], res[1][k]), k
    assert res[0][3] == res[1][3]
    assert not {"obs_raw", "obs_acc", "obs_stats", "obs_pivot", "ret_acc", "ret_carry", "rew_s"} & res[0][3]
    on = VecTrainer(_norm_args(obs_norm_calib_steps=0), flag=0, d_capture=15000.0)
    assert {"obs_raw", "obs_acc", "rew_s"} <= _tensor_names(on)


def test_trainer_norm_state_round_trip(run):
    from satrl.trainer import VecTrainer
    tr, rec, _ = run
    state = tr.norm_state()
    fresh = VecTrainer(_norm_args(obs_norm_calib_steps=0), flag=0, d_capture=15000.0, use_graphs=False)
    raw = torch.cat([rec["norm"][k]["raw"] for k in (3, 40, -1)])      # raw observations the env produced
    want = tr.normalize_obs(raw)
    assert float(want.abs().max()) <= 10.0 and float((want.abs() < 10.0).float().mean()) > 0.5
    assert not torch.equal(fresh.normalize_obs(raw), want)
    fresh.load_norm_state(copy.deepcopy(state))
    torch.cuda.synchronize()
    assert torch.equal(fresh.normalize_obs(raw), want)
    assert torch.equal(fresh.obs_stats, tr.obs_stats) and torch.equal(fresh.obs_pivot, tr.obs_pivot)
    assert torch.equal(fresh.ret_carry, tr.ret_carry)
    got = fresh.norm_state()
    for part in ("obs", "ret"):
        for k, v in state[part].items():
            assert isinstance(got[part][k], np.ndarray) and np.array_equal(got[part][k], v), (part, k)
    assert np.array_equal(got["carry"], state["carry"])


# -- data parallelism: two ranks on one device over gloo -------------------------------
def _dp_args(num_envs, **kw):
    return _norm_args(num_envs=num_envs, batch_size=num_envs * 24, mini_batch_size=256, seed=4, **kw)


def _dp_outputs(tr):
    tr.collect()
    tr.compute_advantages()
    tr.finish_iteration()
    torch.cuda.synchronize()
    o, r = tr.obs_rms, tr.ret_rms
    return dict(obs=tr.buf.obs.cpu().numpy(), rew_s=tr.rew_s.cpu().numpy(), carry=tr.ret_carry.cpu().numpy(),
                stats=tr.obs_stats.cpu().numpy(), pivot=tr.obs_pivot.cpu().numpy(),
                moments=np.concatenate([[o.n], o.mean, o.M2, [r.n, float(r.mean), float(r.M2)]]))


def _dp_rank(rank, port, q):
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        from satrl.trainer import VecTrainer
        with pytest.raises(ValueError, match="num_envs % 32"):      # refused before anything is built
            VecTrainer(_dp_args(48), flag=0, d_capture=15000.0, pg=dist.group.WORLD, env_offset=rank * 48)
        tr = VecTrainer(_dp_args(32), flag=0, d_capture=15000.0, pg=dist.group.WORLD, env_offset=rank * 32)
        q.put((rank, _dp_outputs(tr)))
    finally:
        dist.destroy_process_group()


def test_trainer_statistics_are_sharding_invariant():
    """2 ranks x 32 envs == 1 process x 64 envs, bit for bit: the normalised
    rollout, the observation and return moments after the iteration's merge,
    the device statistics, the scaled rewards and the return carry."""
    import socket
    import torch.multiprocessing as mp
    from satrl.trainer import VecTrainer
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_dp_rank, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    one = _dp_outputs(VecTrainer(_dp_args(64, minibatch_sampler="stratified"), flag=0, d_capture=15000.0))
    assert one["moments"][0] == 64 * (64 + 24)
    for r in range(2):
        got = res[r]
        for k in ("stats", "pivot", "moments"):
            assert np.array_equal(got[k], one[k]), (r, k)
        assert np.array_equal(got["obs"], one["obs"][:, 32 * r:32 * r + 32]), r
        assert np.array_equal(got["rew_s"], one["rew_s"][:, 32 * r:32 * r + 32]), r
        assert np.array_equal(got["carry"], one["carry"][32 * r:32 * r + 32]), r
