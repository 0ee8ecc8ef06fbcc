"""Checkpoints without a GPU: the host build's episode-return entry points,
the checkpoint directory format (satrl/checkpoint.py), the configuration
fingerprint and the pure functions that slice per-env arrays by global env
range."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch


# -- host build: the 16th f64 plane -----------------------------------------------------
def _host_env(n, **kw):
    from satrl.env import VecSatellites
    return VecSatellites(n, device="cpu", d_capture=15000.0, max_episode_steps=2, threads=1, **kw)


def test_host_episode_return_round_trip_and_stats():
    """get / set round-trip; a step after set ends the episode with the set
    return (plus that step's reward) in stats[1]; NULL sets zeros."""
    n = 3
    rng = np.random.default_rng(0)
    pa = torch.from_numpy(rng.uniform(-1.6, 1.6, (2, n, 3)).astype(np.float32))
    ea = torch.from_numpy(rng.uniform(-1.6, 1.6, (2, n, 3)).astype(np.float32))
    env = _host_env(n)
    env.reset(0)
    assert np.array_equal(env.episode_return().numpy(), np.zeros(n))
    _, r1, d1 = env.step_autoreset(pa[0], ea[0])
    assert not d1.any()
    ret1 = env.episode_return()
    assert ret1.dtype == torch.float64 and np.array_equal(ret1.numpy().astype(np.float32), r1.numpy())
    assert float(env.stats[1]) == 0.0
    f, i = env.get_state()
    # the f64 reward of the next (timeout) step of env k, from a one-env handle in env k's state
    r2 = np.zeros(n)
    for k in range(n):
        one = _host_env(1)
        one.reset(0)
        one.set_state(f[:, k:k + 1].contiguous(), i[:, k:k + 1].contiguous())
        one.set_episode_return(None)
        assert float(one.episode_return()[0]) == 0.0
        _, _, d = one.step_autoreset(pa[1, k:k + 1].contiguous(), ea[1, k:k + 1].contiguous())
        assert bool(d[0]) and float(one.stats[0]) == 1.0
        r2[k] = float(one.stats[1])
    want = torch.tensor([10.5, -20.25, 3e7], dtype=torch.float64)
    env.set_episode_return(want)
    got = env.episode_return()
    assert torch.equal(got, want) and got.data_ptr() != want.data_ptr()
    f2, i2 = env.get_state()
    assert torch.equal(f, f2) and torch.equal(i, i2)           # the 15 public planes are untouched
    _, _, d2 = env.step_autoreset(pa[1], ea[1])
    assert d2.all() and float(env.stats[0]) == n
    acc = 0.0
    for k in range(n):                                          # the host build sums in env order
        acc += float(want[k]) + r2[k]
    assert float(env.stats[1]) == acc
    assert np.array_equal(env.episode_return().numpy(), np.zeros(n))   # every env was reset
    with pytest.raises(Exception, match="episode return"):
        env.set_episode_return(torch.zeros(n, dtype=torch.float32))


def test_episode_return_null_handle_is_err_arg():
    import satrl._lib as L
    lib = L.lib()
    buf = (C.c_double * 3)()
    p = C.cast(buf, C.c_void_p)
    assert lib.satenv_cpu_get_episode_return(None, p, None) == -1
    assert lib.satenv_cpu_set_episode_return(None, p, None) == -1
    assert lib.satenv_cpu_set_episode_return(None, None, None) == -1
    assert b"null handle" in lib.satenv_cpu_last_error()
    env = _host_env(3)
    assert lib.satenv_cpu_get_episode_return(env._h, None, None) == -1
    # the device twins check on the host before any HIP call
    assert lib.satenv_get_episode_return(None, p, None) == -1
    assert lib.satenv_set_episode_return(None, None, None) == -1
    assert lib.satenv_abi_version() == 2 and L.SATENV_F64_PLANES == 15


def test_host_full_state_round_trip():
    n = 5
    rng = np.random.default_rng(1)
    act = torch.from_numpy(rng.uniform(-1.6, 1.6, (4, 2, n, 3)).astype(np.float32))
    a, b = _host_env(n), _host_env(n)
    a.reset(0)
    for t in range(3):                                          # an episode ends at t = 1: indices and stats move
        a.step_autoreset(act[t, 0], act[t, 1])
    st = a.full_state()
    assert set(st) == {"f64", "i32", "ep_return", "episode_index", "stats"}
    assert st["f64"].shape == (15, n) and st["ep_return"].any() and st["episode_index"].all() and st["stats"][0] == n
    stats_ptr = b.stats.data_ptr()
    b.load_full_state(st)
    assert b.stats.data_ptr() == stats_ptr
    oa, ra, da = a.step_autoreset(act[3, 0], act[3, 1])
    ob, rb, db = b.step_autoreset(act[3, 0], act[3, 1])
    assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and da.all()
    sa, sb = a.full_state(), b.full_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    with pytest.raises(ValueError, match="ep_return"):
        b.load_full_state(dict(st, ep_return=st["ep_return"][:-1]))


# -- the directory format -----------------------------------------------------------------
def _nested():
    rng = np.random.default_rng(2)
    return {"flag": 1, "episodes": 12.0,
            "learner": {"P": rng.standard_normal(7).astype(np.float32), "steps": np.array([3.0, 3.0]),
                        "lr": np.float32(2e-4)},
            "env": {"f64": rng.standard_normal((15, 4)), "i32": rng.integers(-5, 5, (3, 4)).astype(np.int32),
                    "stats": np.zeros(4), "n": np.array(4.0)},
            "gen": rng.integers(0, 256, 16).astype(np.uint8), "empty": np.zeros((0, 18), np.float32),
            "strata_gen": {"0": np.arange(16, dtype=np.uint8), "7": np.arange(16, dtype=np.uint8)[::-1].copy()},
            "diagnostics": [{"iteration_count": 0, "approx_kl": float("nan"), "loss": 0.1 + 0.2, "agent": "pursuer"}],
            "metas": [None, {"agent": "evader", "episodes": 1e300}], "none": None, "on": True}


def _same(a, b):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), (sorted(a), sorted(b))
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (np.ndarray, np.generic)):
        b = np.asarray(b)
        assert np.asarray(a).dtype == b.dtype and np.shape(a) == b.shape and np.array_equal(a, b)
    elif isinstance(a, (int, float)) and not isinstance(a, bool):
        b = np.asarray(b)
        assert b.ndim == 0 and b.dtype == (np.int64 if isinstance(a, int) else np.float64) and b.item() == a
    else:
        assert json.dumps(a) == json.dumps(b)


META = {"format_version": 1, "world_size": 1, "global_envs": 4, "shards": [[0, 4]], "fingerprint": {}}


def test_write_read_reproduces_every_dtype(tmp_path):
    from satrl import checkpoint as ck
    d = _nested()
    flat = ck.flatten(d)
    assert {np.asarray(v).dtype for v in flat.values()} >= {np.dtype(t) for t in
                                                             (np.float32, np.float64, np.int32, np.uint8, np.int64)}
    assert flat["learner/lr"].ndim == 0 and flat["env/n"].ndim == 0 and flat["flag"].ndim == 0
    path = ck.write_checkpoint(tmp_path / "ck", flat, META)
    assert sorted(os.listdir(path)) == ["meta.json", "rank0.npz"] and not os.path.exists(path + ".tmp")
    assert ck.read_meta(path) == META
    with np.load(os.path.join(path, "rank0.npz"), allow_pickle=False) as z:      # numeric arrays only
        assert set(z.files) == set(flat)
        for k in z.files:
            assert z[k].dtype.kind in "fiu" and z[k].dtype == flat[k].dtype and z[k].shape == flat[k].shape
    with ck.read_rank(path, 0) as z:
        got = ck.unflatten({k: z[k] for k in z.files})
    _same(d, got)
    assert got["diagnostics"][0]["loss"] == 0.1 + 0.2 and np.isnan(got["diagnostics"][0]["approx_kl"])
    with pytest.raises(TypeError, match="numeric"):
        ck.write_rank(str(tmp_path), 3, {"x": np.array(["a"])})
    with pytest.raises(ValueError, match="separator"):
        ck.flatten({"a/b": 1})


def test_directory_without_meta_is_incomplete(tmp_path):
    from satrl import checkpoint as ck
    path = ck.write_checkpoint(tmp_path / "ck", ck.flatten(_nested()), META)
    os.remove(os.path.join(path, "meta.json"))
    with pytest.raises(FileNotFoundError, match="meta.json"):
        ck.read_meta(path)
    with pytest.raises(FileNotFoundError):
        ck.load(types.SimpleNamespace(pg=None), path)           # refused before the trainer is touched
    with pytest.raises(FileNotFoundError):
        ck.read_meta(str(tmp_path / "nothing"))
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump(dict(META, format_version=99), f)
    with pytest.raises(ValueError, match="format"):
        ck.read_meta(path)


@pytest.mark.parametrize("where", ["write_rank", "json.dump", "_commit", "os.replace"])
def test_interrupted_write_keeps_the_previous_checkpoint(tmp_path, monkeypatch, where):
    from satrl import checkpoint as ck
    first = ck.flatten(_nested())
    path = ck.write_checkpoint(tmp_path / "ck", first, dict(META, tag="first"))

    class Stop(Exception):
        pass

    def boom(*a, **k):
        raise Stop()

    if where == "os.replace":                                   # the rename that moves the new directory into place
        real = os.replace
        monkeypatch.setattr(ck.os, "replace", lambda a, b: boom() if str(a).endswith(".tmp") else real(a, b))
    elif where == "json.dump":
        monkeypatch.setattr(ck.json, "dump", boom)
    else:
        monkeypatch.setattr(ck, where, boom)
    second = dict(first, flag=np.asarray(0))
    with pytest.raises(Stop):
        ck.write_checkpoint(tmp_path / "ck", second, dict(META, tag="second"))
    monkeypatch.undo()
    assert ck.read_meta(path)["tag"] == "first"
    with ck.read_rank(path, 0) as z:
        assert int(z["flag"]) == 1 and set(z.files) == set(first)
    # and the next complete write replaces it
    ck.write_checkpoint(tmp_path / "ck", second, dict(META, tag="second"))
    assert ck.read_meta(path)["tag"] == "second" and sorted(os.listdir(tmp_path)) == ["ck"]
    with ck.read_rank(path, 0) as z:
        assert int(z["flag"]) == 0


# -- fingerprint ---------------------------------------------------------------------------
def _stub_trainer(**kw):
    """What checkpoint.fingerprint reads of a trainer, without a device."""
    from satrl.trainer import args_param
    half = [100.0] * 3 + [1.0] * 3 + [200.0] * 3 + [2.0] * 3
    base = dict(hidden_width=64, mini_batch_size=64, num_envs=64, horizon=8, K_epochs=2, max_episode_steps=5, seed=3,
                opponent_pool=2, obs_norm=True, reward_scaling=True, reset_spread=half, chkpt_dir="/tmp")
    args = args_param(**dict(base, **kw))
    return types.SimpleNamespace(args=args, pg=None, N=args.num_envs, seed=args.seed, reset_seed=args.seed,
                                 opponent_seed=args.seed, obs_norm=args.obs_norm, reward_scaling=args.reward_scaling,
                                 sampler="uniform", dp_minibatch=args.dp_minibatch, reset_spread=args.reset_spread,
                                 env=types.SimpleNamespace(d_capture=15000.0))


def test_fingerprint_names_the_field_that_differs():
    from satrl import checkpoint as ck
    fp = ck.fingerprint(_stub_trainer())
    assert tuple(fp) == ck.FINGERPRINT_FIELDS and fp["global_envs"] == 64 and len(fp["reset_box"][0]) == 12
    saved = json.loads(json.dumps(fp))                          # as meta.json holds it
    ck.check_fingerprint(saved, fp)
    other = {"hidden_width": 256, "global_envs": 128, "seed": 4, "reset_seed": 9, "opponent_seed": 11, "obs_norm": False,
             "reward_scaling": False, "opponent_pool": 3, "minibatch_sampler": "stratified", "dp_minibatch": "per_gpu",
             "mini_batch_size": 128, "max_episode_steps": 6, "d_capture": 100000.0, "reset_box": None,
             "max_train_steps": 1e6}
    assert set(other) == set(ck.FINGERPRINT_FIELDS)
    for field, v in other.items():
        assert v != fp[field]
        with pytest.raises(ValueError, match=rf"\b{field}=") as e:
            ck.check_fingerprint(saved, dict(fp, **{field: v}))
        assert repr(saved[field]) in str(e.value) and repr(json.loads(json.dumps(v))) in str(e.value)
    with pytest.raises(ValueError, match="seed"):
        ck.check_fingerprint({k: v for k, v in saved.items() if k != "seed"}, fp)
    # what may differ between the writer and the reader
    for kw in (dict(horizon=16), dict(K_epochs=7), dict(lr_a=1e-3, lr_c=5e-4), dict(rollout_graph_chunk=4),
               dict(update_graph_group=2), dict(diagnostics=True)):
        ck.check_fingerprint(saved, ck.fingerprint(_stub_trainer(**kw)))
    # ... and the same differences through the trainer's own fields
    with pytest.raises(ValueError, match="max_episode_steps=5.*max_episode_steps=9"):
        ck.check_fingerprint(saved, ck.fingerprint(_stub_trainer(max_episode_steps=9)))


# -- global env ranges ---------------------------------------------------------------------
def test_range_slicing():
    from satrl import checkpoint as ck
    rng = np.random.default_rng(3)
    planes = rng.standard_normal((15, 96))                      # env axis 1
    obs = rng.standard_normal((96, 18)).astype(np.float32)      # env axis 0
    idx = np.arange(96, dtype=np.int32)
    for cut in ([(0, 96)], [(0, 32), (32, 64)], [(0, 64), (64, 32)], [(0, 32), (32, 32), (64, 32)]):
        ck.check_tiling(cut, 96, whole_blocks=True)
        for a, env_axis in ((planes, 1), (obs, 0), (idx, 0)):
            pieces = [(o, np.take(a, np.arange(o, o + n), axis=env_axis)) for o, n in cut]
            whole = ck.gather_range(pieces, 0, 96, env_axis)                     # whole
            assert whole.dtype == a.dtype and np.array_equal(whole, a) and whole.flags.c_contiguous
            for lo, n in ((0, 48), (48, 48), (32, 64), (16, 40)):                 # split in two; spanning two shards
                got = ck.gather_range(pieces, lo, n, env_axis)
                assert np.array_equal(got, np.take(a, np.arange(lo, lo + n), axis=env_axis)), (cut, lo, n)
    shards = [(0, 64), (64, 32)]
    assert ck.overlapping(shards, 32, 64) == [0, 1] and ck.overlapping(shards, 0, 64) == [0]
    assert ck.overlapping(shards, 64, 32) == [1]
    with pytest.raises(ValueError, match="none of the checkpoint's shards"):
        ck.gather_range([(0, idx[:32]), (64, idx[64:])], 0, 96)                  # a hole
    with pytest.raises(ValueError, match="none of the checkpoint's shards"):
        ck.gather_range([(0, idx[:32])], 0, 40)


def test_range_checks():
    from satrl import checkpoint as ck
    for bad in ([(0, 32), (64, 32)], [(0, 64), (32, 64)], [(0, 32), (32, 32)], [(32, 64)], [(0, 64), (64, 64)],
                [(0, 96), (96, 0)]):
        with pytest.raises(ValueError, match="do not tile"):
            ck.check_tiling(bad, 96)
    ck.check_tiling([(48, 48), (0, 48)], 96)                    # any order; a split block without per-block state
    with pytest.raises(ValueError, match="split a 32-env block"):
        ck.check_tiling([(0, 48), (48, 48)], 96, whole_blocks=True)
    ck.check_tiling([(0, 64), (64, 36)], 100, whole_blocks=True)          # the run's ragged last block is whole
    ck.check_range(32, 32, 64, True)
    ck.check_range(0, 40, 40, True)
    for lo, n in ((16, 32), (0, 48), (32, 16)):
        with pytest.raises(ValueError, match="split a 32-env block"):
            ck.check_range(lo, n, 64, True)
        ck.check_range(lo, n, 64, False)
    for lo, n in ((32, 64), (-1, 8), (0, 0)):
        with pytest.raises(ValueError, match="outside"):
            ck.check_range(lo, n, 64)
