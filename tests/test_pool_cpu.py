"""Opponent pool, host side: the refusals of satrl_policy_act_pool and
satrl_opponent_assign before any device call, the assignment rule against a
NumPy restatement on the Philox of reset_dist_reference.py (itself checked
against Random123's vectors first), its independence of the sharding, the
OpponentPool ring on host tensors, and the args_param keywords.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import reset_dist_reference as R

ASSIGN_STREAM = 3          # Philox key streams 0 / 1: action noise, 2: the reset draw


def _lib():
    import satrl._lib as L
    return L, L.lib()


def test_symbols_are_exported_and_bound():
    L, lib = _lib()
    for name in ("satrl_policy_act_pool", "satrl_opponent_assign"):
        assert name in L.exported_symbols()
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None
    assert len(lib.satrl_policy_act_pool.argtypes) == 20
    assert len(lib.satrl_opponent_assign.argtypes) == 7


def test_entry_points_reject_bad_arguments_before_any_device_call():
    """Every refusal returns -1 on the host; the fake non-null pointer is never
    dereferenced (a launch would fail with -2 on a host without a GPU)."""
    L, lib = _lib()
    fake = C.c_void_p(4096)                                # non-null, 16-byte aligned
    total = {H: L_total(H) for H in (64, 128, 256)}

    def pa(H=64, N=40, obs=fake, P0=fake, P1=fake, sb=None, act0=fake, logp0=fake, act1=fake, logp1=fake, agent=1,
           pool=fake, stride=None, K=3, member=fake):
        stride = (total[H] + 63) // 64 * 64 if stride is None and H in total else stride or 0
        return lib.satrl_policy_act_pool(H, N, obs, P0, P1, 1.6, 0, 0, 0, sb, act0, logp0, act1, logp1, agent, pool,
                                         stride, K, member, None)

    # every refusal of satrl_policy_act
    assert pa(H=100) == -1 and pa(H=0) == -1 and pa(H=512) == -1
    assert pa(N=0) == -1 and pa(N=-3) == -1
    assert pa(obs=None) == -1 and pa(P0=None) == -1 and pa(act0=None) == -1 and pa(logp0=None) == -1
    # both agents are required
    assert pa(P1=None) == -1 and pa(act1=None) == -1 and pa(logp1=None) == -1
    assert pa(P1=None, act1=None, logp1=None) == -1
    assert pa(agent=-1) == -1 and pa(agent=2) == -1
    assert pa(pool=None) == -1 and pa(member=None) == -1
    assert pa(K=0) == -1 and pa(K=-1) == -1
    for H in (64, 128, 256):
        assert pa(H=H, stride=total[H] - 1) == -1                       # below the layout total
        assert pa(H=H, stride=(total[H] // 4) * 4 - 4) == -1
        for d in (1, 2, 3):
            assert pa(H=H, stride=(total[H] + 3) // 4 * 4 + 4 + d) == -1   # large enough, not a multiple of 4
    for off in (4, 8, 12, 1):
        assert pa(pool=C.c_void_p(4096 + off)) == -1                    # not 16-byte aligned
    assert b"satrl_policy_act_pool" in lib.satrl_ppo_last_error()

    out = (C.c_int32 * 4)()
    po = C.cast(out, C.c_void_p)

    def oa(first=0, n=4, filled=2, p=0.5, o=po):
        return lib.satrl_opponent_assign(1, 2, first, n, filled, p, o)

    assert oa() == 0
    assert oa(o=None) == -1
    assert oa(n=0) == -1 and oa(n=-1) == -1
    assert oa(first=-1) == -1
    assert oa(filled=-1) == -1
    assert oa(p=-1e-9) == -1 and oa(p=1.0 + 1e-9) == -1 and oa(p=math.nan) == -1 and oa(p=math.inf) == -1
    assert b"satrl_opponent_assign" in lib.satrl_ppo_last_error()


def L_total(H):
    from satrl.ppo import ppo_layout
    return ppo_layout(H)["total"]


def test_numpy_philox_reproduces_random123_vectors():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32_10(np.array(ctr, dtype=np.uint32), *key)
        assert tuple(int(x) for x in got) == want


def _restated(seed, iteration, first_block, n_blocks, filled, latest_prob):
    g = np.arange(n_blocks, dtype=np.uint64) + np.uint64(first_block)
    it = np.uint64(iteration)
    m32 = np.uint64(R.M32)
    ctr = np.stack([g & m32, g >> np.uint64(32), np.full_like(g, it & m32), np.full_like(g, it >> np.uint64(32))],
                   axis=-1).astype(np.uint32)
    w = R.philox4x32_10(ctr, *R.philox_key(seed, ASSIGN_STREAM))
    u = (w[:, 0].astype(np.float64) + 0.5) * 2.0 ** -32
    pick = ((w[:, 1].astype(np.uint64) * np.uint64(filled)) >> np.uint64(32)).astype(np.int32)
    if filled == 0:
        return np.full(n_blocks, -1, dtype=np.int32)
    return np.where(u < latest_prob, np.int32(-1), pick).astype(np.int32)


def test_opponent_assign_equals_restatement():
    from satrl.pool import opponent_assign
    some_stored = False
    for seed in (0, 2 ** 63 + 5):
        for it in (0, 1, 2 ** 32 + 3):
            for first in (0, 7, 2 ** 32 + 1):
                for filled in (0, 1, 3, 8):
                    for p in (0.0, 0.5, 1.0):
                        tag = (seed, it, first, filled, p)
                        got = opponent_assign(seed, it, first, 64, filled, p)
                        want = _restated(seed, it, first, 64, filled, p)
                        assert got.dtype == np.int32 and got.shape == (64,), tag
                        assert np.array_equal(got, want), tag
                        assert ((got >= -1) & (got < max(filled, 1))).all(), tag
                        if filled == 0 or p == 1.0:
                            assert (got == -1).all(), tag
                        elif p == 0.0:
                            assert (got >= 0).all(), tag
                        else:
                            some_stored |= bool((got >= 0).any()) and bool((got == -1).any())
    assert some_stored                                       # latest_prob 0.5 mixes live and stored blocks
    # the draws of different iterations, seeds and blocks differ
    a = opponent_assign(0, 0, 0, 64, 8, 0.0)
    assert not np.array_equal(a, opponent_assign(0, 1, 0, 64, 8, 0.0))
    assert not np.array_equal(a, opponent_assign(1, 0, 0, 64, 8, 0.0))
    assert len(set(a.tolist())) > 1


def test_assignment_does_not_depend_on_the_sharding():
    from satrl.pool import OpponentPool
    pool = OpponentPool(4, 64, "cpu", seed=11)
    P = torch.zeros(pool.total)
    for _ in range(3):
        pool.add(P)
    for it in (0, 5, 2 ** 32 + 3):
        whole = pool.assign(it, 0, 8, 0.5)
        parts = np.concatenate([pool.assign(it, 0, 4, 0.5), pool.assign(it, 4, 4, 0.5)])
        assert np.array_equal(whole, parts), it


def test_opponent_pool_ring_on_host_tensors():
    from satrl.pool import OpponentPool
    K, H = 3, 64
    pool = OpponentPool(K, H, "cpu", seed=5)
    total = L_total(H)
    assert pool.total == total and pool.stride % 64 == 0 and pool.stride >= total
    assert tuple(pool.storage.shape) == (K, pool.stride) and pool.storage.dtype == torch.float32
    assert pool.filled == 0
    with pytest.raises(IndexError):
        pool.slot(0)
    base = pool.storage.data_ptr()
    sets = [torch.full((total,), float(j + 1)) + torch.arange(total) * 1e-3 for j in range(5)]
    for j, P in enumerate(sets):
        k = pool.add(P, {"agent": "evader", "iteration_count": j, "episodes": 10.0 * j})
        assert k == j % K                                    # ring order: the oldest slot is overwritten once full
        assert pool.filled == min(j + 1, K)
    assert pool.storage.data_ptr() == base                   # in place: the storage never moves
    # after five adds into three slots: slots hold sets 3, 4, 2
    for k, j in enumerate((3, 4, 2)):
        assert torch.equal(pool.slot(k), sets[j]), k
        assert pool.metas[k] == {"agent": "evader", "iteration_count": j, "episodes": 10.0 * j}
        assert pool.slot(k).data_ptr() == base + 4 * k * pool.stride      # a view
    assert not bool(pool.storage[:, total:].any())           # the padding is never written
    with pytest.raises(IndexError):
        pool.slot(K)
    with pytest.raises(IndexError):
        pool.slot(-1)
    with pytest.raises(ValueError):
        pool.add(torch.zeros(total - 1))
    with pytest.raises(ValueError):
        OpponentPool(0, H, "cpu")
    # state() -> load_state() round trip into a fresh pool
    st = pool.state()
    assert not st["storage"].is_cuda
    fresh = OpponentPool(K, H, "cpu", seed=5)
    fresh.load_state(st)
    assert torch.equal(fresh.storage, pool.storage) and fresh.metas == pool.metas
    assert fresh.cursor == pool.cursor == 5 % K and fresh.filled == K
    assert fresh.add(sets[0]) == pool.add(sets[0])           # the ring goes on from the same slot
    # the state is a copy: the pool's later adds do not reach it
    assert torch.equal(st["storage"][2], torch.cat([sets[2], torch.zeros(pool.stride - total)]))
    with pytest.raises(ValueError):
        OpponentPool(K + 1, H, "cpu").load_state(st)
    # a partly filled pool: assign() draws over the filled slots only
    part = OpponentPool(8, H, "cpu", seed=5)
    part.add(sets[0])
    part.add(sets[1])
    a = part.assign(3, 0, 64, 0.0)
    assert set(a.tolist()) == {0, 1}
    assert (OpponentPool(8, H, "cpu", seed=5).assign(3, 0, 64, 0.0) == -1).all()


def test_args_param_keywords():
    from satrl.trainer import args_param
    a = args_param()
    assert a.opponent_pool == 0 and a.opponent_latest_prob == 0.5
    assert a.opponent_snapshot_every is None and a.opponent_seed is None
    b = args_param(opponent_pool=8, opponent_latest_prob=0.25, opponent_snapshot_every=4, opponent_seed=9)
    assert (b.opponent_pool, b.opponent_latest_prob, b.opponent_snapshot_every, b.opponent_seed) == (8, 0.25, 4, 9)
    assert args_param(opponent_latest_prob=0).opponent_latest_prob == 0.0
    assert args_param(opponent_latest_prob=1).opponent_latest_prob == 1.0
    for bad in (dict(opponent_pool=-1), dict(opponent_latest_prob=-0.1), dict(opponent_latest_prob=1.5),
                dict(opponent_latest_prob=float("nan")), dict(opponent_snapshot_every=0)):
        with pytest.raises(ValueError):
            args_param(**bad)
