"""League play, host side: satrl_league_assign against a NumPy restatement
on the Philox of reset_dist_reference.py, its equality with
satrl_opponent_assign where no law and no weight is given, its independence
of the sharding, the weighted pick, pfsp_weights against a hand-computed
table, the refusals of the three league entry points before any device call,
and the args_param keywords.  No GPU."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import reset_dist_reference as R

ASSIGN_STREAM = 3          # the pool's assignment stream (tests/test_pool_cpu.py)
MAX_LAWS = 8


def _lib():
    import satrl._lib as L
    return L, L.lib()


@functools.lru_cache(maxsize=None)
def _words(seed, iteration, first_block, n_blocks):
    g = np.arange(n_blocks, dtype=np.uint64) + np.uint64(first_block)
    it = np.uint64(iteration)
    m32 = np.uint64(R.M32)
    ctr = np.stack([g & m32, g >> np.uint64(32), np.full_like(g, it & m32), np.full_like(g, it >> np.uint64(32))],
                   axis=-1).astype(np.uint32)
    return R.philox4x32_10(ctr, *R.philox_key(seed, ASSIGN_STREAM))


def _restated(seed, iteration, first_block, n_blocks, K, filled, n_laws, latest_prob, law_prob, weights):
    """The rule of include/satrl_ppo.h, block by block in Python floats (f64)."""
    w = _words(seed, iteration, first_block, n_blocks)
    out = np.empty(n_blocks, dtype=np.int32)
    S, last_pos = 0.0, -1
    if weights is not None:
        for k in range(filled):
            S += float(weights[k])
            if weights[k] > 0:
                last_pos = k
    for i in range(n_blocks):
        w0, w1, w2 = int(w[i, 0]), int(w[i, 1]), int(w[i, 2])
        u = (w0 + 0.5) * 2.0 ** -32
        if (filled == 0 and n_laws == 0) or u < latest_prob:
            m = -1
        elif n_laws > 0 and (filled == 0 or u < latest_prob + law_prob):
            m = K + ((w2 * n_laws) >> 32)
        elif weights is None:
            m = (w1 * filled) >> 32
        else:
            v = (w1 + 0.5) * 2.0 ** -32 * S
            c, m = 0.0, last_pos
            for k in range(filled):
                c += float(weights[k])
                if v < c:
                    m = k
                    break
        out[i] = m
    return out


PROBS = ((0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.25, 0.5), (0.5, 0.5), (0.3, 0.0))


def _weight_cases(filled):
    if filled == 0:
        return (None,)
    if filled == 1:
        return (None, [1.0], [0.125])
    return (None, [1.0] * filled, [0.01, 4.0, 0.5][:filled], [0.0, 1.0, 0.0][:filled], [0.5, 0.0, 0.25][:filled])


def test_symbols_are_exported_and_bound():
    L, lib = _lib()
    for name, n in (("satrl_policy_act_league", 23), ("satrl_league_assign", 11), ("satrl_league_tally", 7)):
        assert name in L.exported_symbols()
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n


def test_league_assign_equals_restatement():
    from satrl.pool import league_assign
    K, n = 4, 48
    kinds = set()
    for seed in (0, 2 ** 63 + 5):
        for it in (0, 2 ** 32 + 3):
            for first in (0, 2 ** 32 - 16, 2 ** 33 + 1):          # the second range crosses the 2^32 boundary of g
                for filled in (0, 1, 3):
                    for n_laws in (0, 1, 3):
                        for lp, wp in PROBS:
                            for wts in _weight_cases(filled):
                                tag = (seed, it, first, filled, n_laws, lp, wp, wts)
                                got = league_assign(seed, it, first, n, K, filled, n_laws, lp, wp, wts)
                                want = _restated(seed, it, first, n, K, filled, n_laws, lp, wp, wts)
                                assert got.dtype == np.int32 and got.shape == (n,), tag
                                assert np.array_equal(got, want), tag
                                assert ((got == -1) | ((got >= 0) & (got < filled)) |
                                        ((got >= K) & (got < K + n_laws))).all(), tag
                                if wts is not None:
                                    stored = got[(got >= 0) & (got < K)]
                                    assert all(wts[k] > 0 for k in stored.tolist()), tag
                                kinds |= {"live"} if (got == -1).any() else set()
                                kinds |= {"stored"} if ((got >= 0) & (got < K)).any() else set()
                                kinds |= {"law"} if (got >= K).any() else set()
                                if lp == 0.25 and wp == 0.5 and filled == 3 and n_laws == 3:
                                    assert (got == -1).any() and (got >= K).any() and ((got >= 0) & (got < K)).any()
    assert kinds == {"live", "stored", "law"}
    # no stored opponent yet: what is not live is a law, whatever law_prob says
    a = league_assign(1, 2, 0, 64, K, 0, 2, 0.5, 0.0)
    assert set(a.tolist()) == {-1, K, K + 1}


def test_league_assign_without_laws_and_weights_is_the_pool_rule():
    from satrl.pool import league_assign, opponent_assign
    for seed in (0, 2 ** 63 + 5):
        for it in (0, 1, 2 ** 32 + 3):
            for first in (0, 7, 2 ** 32 - 16, 2 ** 32 + 1):
                for filled in (0, 1, 3, 8):
                    for p in (0.0, 0.5, 1.0):
                        for law_prob in (0.0, 1.0 - p):                   # without laws it plays no part
                            got = league_assign(seed, it, first, 64, 8, filled, 0, p, law_prob, None)
                            assert np.array_equal(got, opponent_assign(seed, it, first, 64, filled, p)), \
                                (seed, it, first, filled, p, law_prob)


def test_league_assignment_does_not_depend_on_the_sharding():
    from satrl.pool import league_assign
    w = [0.2, 0.0, 1.5]
    for it in (0, 5, 2 ** 32 + 3):
        for first in (0, 2 ** 32 - 4):
            for wts in (None, w):
                whole = league_assign(11, it, first, 8, 4, 3, 2, 0.25, 0.25, wts)
                parts = np.concatenate([league_assign(11, it, first, 4, 4, 3, 2, 0.25, 0.25, wts),
                                        league_assign(11, it, first + 4, 4, 4, 3, 2, 0.25, 0.25, wts)])
                assert np.array_equal(whole, parts), (it, first, wts)


def test_weighted_pick():
    from satrl.pool import league_assign
    a = league_assign(3, 1, 0, 256, 3, 3, 0, 0.25, 0.0, [0.0, 1.0, 0.0])
    assert set(a.tolist()) == {-1, 1}                         # every stored pick is slot 1
    a = league_assign(3, 1, 0, 256, 3, 3, 2, 0.0, 0.5, [0.0, 1.0, 0.0])
    assert set(a.tolist()) == {1, 3, 4}
    # a heavier slot is drawn more often; equal weights are the uniform proportions
    a = league_assign(3, 1, 0, 4096, 3, 3, 0, 0.0, 0.0, [1.0, 8.0, 1.0])
    n = np.bincount(a, minlength=3)
    assert n[1] > 3 * n[0] and n[1] > 3 * n[2] and n[0] > 0 and n[2] > 0
    # the scale of the weights plays no part beyond rounding: powers of two are exact
    b = league_assign(3, 1, 0, 4096, 3, 3, 0, 0.0, 0.0, [0.25, 2.0, 0.25])
    assert np.array_equal(a, b)


def test_pfsp_weights_table():
    from satrl.pool import pfsp_weights
    # (episodes, wins): p = (wins + 1) / (episodes + 2); weight = (1 - p) ** power
    e = np.array([0, 2, 2, 6, 98])
    w = np.array([0, 0, 2, 3, 98])
    one = np.array([1 / 2, 3 / 4, 1 / 4, 1 / 2, 1 / 100])          # 1 - p by hand: 1-1/2, 1-1/4, 1-3/4, 1-4/8, 1-99/100
    assert np.array_equal(pfsp_weights(e, w, 1), 1.0 - (w + 1.0) / (e + 2.0))
    assert np.allclose(pfsp_weights(e, w, 1), one, rtol=0, atol=1e-15)
    assert np.array_equal(pfsp_weights(e, w, 1)[:4], one[:4])        # dyadic values are exact
    p1 = pfsp_weights(e, w, 1)
    assert np.array_equal(pfsp_weights(e, w, 2), p1 * p1)            # repeated multiplication, in this order
    assert np.array_equal(pfsp_weights(e, w, 3), p1 * p1 * p1)
    assert np.array_equal(pfsp_weights(e, w, 2)[:4], np.array([1 / 4, 9 / 16, 1 / 16, 1 / 4]))
    assert pfsp_weights(e, w).dtype == np.float64 and np.array_equal(pfsp_weights(e, w), pfsp_weights(e, w, 2))
    assert pfsp_weights([0], [0], 5)[0] == 0.5 ** 5                   # an unplayed slot
    assert pfsp_weights([], [], 2).shape == (0,)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises((ValueError, TypeError)):
            pfsp_weights(e, w, bad)
    with pytest.raises(ValueError):
        pfsp_weights([1, 2], [2, 1])                                  # more wins than episodes
    with pytest.raises(ValueError):
        pfsp_weights([1, 2], [1])


def _msg(lib):
    return lib.satrl_ppo_last_error()


def test_league_assign_refusals_name_the_entry_point_and_the_argument():
    L, lib = _lib()
    out = (C.c_int32 * 4)()
    po = C.cast(out, C.c_void_p)

    def wp(*v):
        return C.cast((C.c_double * len(v))(*v), C.c_void_p)

    def la(first=0, n=4, K=3, filled=2, n_laws=2, p=0.5, q=0.25, w=None, o=po):
        return lib.satrl_league_assign(1, 2, first, n, K, filled, n_laws, p, q, w, o)

    def no(word, **kw):
        assert lib.satrl_gae(0, 0, None, None, None, 0.0, 0.0, None, None, None) == -1     # another call's text first
        assert la(**kw) == -1, kw
        msg = _msg(lib)
        assert msg.startswith(b"satrl_league_assign: ") and word in msg, (kw, msg)

    assert la() == 0 and la(w=wp(1.0, 2.0)) == 0
    assert la(filled=0, w=wp()) == 0 and la(filled=0, n_laws=0) == 0
    no(b"member_out", o=None)
    no(b"n_blocks", n=0)
    no(b"n_blocks", n=-1)
    no(b"first_block", first=-1)
    no(b"K", K=-1, filled=0)
    no(b"filled", filled=-1)
    no(b"filled", filled=4)
    no(b"n_laws", n_laws=-1)
    no(b"n_laws", n_laws=MAX_LAWS + 1)
    assert la(n_laws=MAX_LAWS) == 0
    for bad in (-1e-9, 1.0 + 1e-9, math.nan, math.inf):
        no(b"latest_prob", p=bad, q=0.0)
        no(b"law_prob", p=0.0, q=bad)
    no(b"latest_prob + law_prob", p=0.75, q=0.5)
    assert la(p=0.75, q=0.25) == 0 and la(p=1.0, q=0.0) == 0 and la(p=0.0, q=1.0) == 0
    for bad in (-1.0, math.nan, math.inf, -math.inf):
        no(b"weights[1]", w=wp(1.0, bad))
    no(b"sum of weights", w=wp(0.0, 0.0))
    no(b"sum of weights", w=wp(1e308, 1e308))                    # finite weights, an infinite sum
    # the Python wrapper raises with the same text, and checks the weights' length
    from satrl.pool import league_assign
    with pytest.raises(L.NativeError, match=r"satrl_league_assign: n_laws 9"):
        league_assign(0, 0, 0, 4, 3, 2, 9, 0.5, 0.25)
    with pytest.raises(ValueError, match="weights"):
        league_assign(0, 0, 0, 4, 3, 2, 0, 0.5, 0.0, [1.0])


def test_policy_act_league_and_tally_reject_bad_arguments_before_any_device_call():
    """Every refusal the headers list returns -1 on the host; the fake non-null
    pointer is never dereferenced (a launch would fail with -2 without a GPU)."""
    L, lib = _lib()
    from satrl.ppo import ppo_layout
    fake = C.c_void_p(4096)                                # non-null, 16-byte aligned
    total = {H: ppo_layout(H)["total"] for H in (64, 128, 256)}

    def pl(H=64, N=40, obs=fake, P0=fake, P1=fake, act0=fake, logp0=fake, act1=fake, logp1=fake, agent=1, pool=fake,
           stride=None, K=3, member=fake, obs_law=fake, laws=fake, J=2):
        stride = (total[H] + 63) // 64 * 64 if stride is None and H in total else stride or 0
        return lib.satrl_policy_act_league(H, N, obs, P0, P1, 1.6, 0, 0, 0, None, act0, logp0, act1, logp1, agent,
                                           pool, stride, K, member, obs_law, laws, J, None)

    def no(word=b"", **kw):
        assert lib.satrl_gae(0, 0, None, None, None, 0.0, 0.0, None, None, None) == -1
        assert pl(**kw) == -1, kw
        msg = _msg(lib)
        assert msg.startswith(b"satrl_policy_act_league: ") and word in msg, (kw, msg)

    # every refusal of satrl_policy_act_pool
    for H in (100, 0, 512):
        no(b"H", H=H)
    no(b"N", N=0)
    no(b"N", N=-3)
    for k in ("obs", "P0", "act0", "logp0", "P1", "act1", "logp1"):
        no(k.encode(), **{k: None})
    no(b"pool_agent", agent=-1)
    no(b"pool_agent", agent=2)
    no(b"pool is NULL", pool=None)
    no(b"member is NULL", member=None)
    no(b"K", K=0)
    no(b"K", K=-1)
    for H in (64, 128, 256):
        no(b"pool_stride", H=H, stride=total[H] - 1)
        no(b"pool_stride", H=H, stride=(total[H] + 3) // 4 * 4 + 5)
    for off in (4, 8, 12, 1):
        no(b"16-byte", pool=C.c_void_p(4096 + off))
    # its own
    no(b"obs_law is NULL", obs_law=None)
    no(b"laws is NULL", laws=None)
    for J in (0, -1, MAX_LAWS + 1):
        no(b"J", J=J)
    for off in (4, 1, 2):
        no(b"8-byte", laws=C.c_void_p(4096 + off))

    def tl(T=5, N=39, rew=fake, done=fake, tally=fake):
        return lib.satrl_league_tally(T, N, rew, done, 150.0, tally, None)

    for word, kw in ((b"T", dict(T=0)), (b"T", dict(T=-1)), (b"N", dict(N=0)), (b"T", dict(T=2 ** 31)),
                     (b"rew is NULL", dict(rew=None)), (b"done is NULL", dict(done=None)),
                     (b"tally is NULL", dict(tally=None))):
        assert lib.satrl_gae(0, 0, None, None, None, 0.0, 0.0, None, None, None) == -1
        assert tl(**kw) == -1, kw
        assert _msg(lib).startswith(b"satrl_league_tally: ") and word in _msg(lib), (kw, _msg(lib))


def test_args_param_league_keywords():
    from satrl import scripted as S
    from satrl.trainer import args_param
    a = args_param()
    assert a.league_laws == {} and a.league_law_prob == 0.25 and a.opponent_weighting == "uniform"
    assert a.pfsp_power == 2
    law = S.evade(gain=0.25)
    b = args_param(opponent_pool=4, opponent_latest_prob=0.25, league_law_prob=0.5, opponent_weighting="pfsp",
                   pfsp_power=3, league_laws={"evader": [law, "coast"], "pursuer": ["intercept"]})
    assert b.league_laws["evader"][0] is law and len(b.league_laws["evader"]) == 2
    assert np.array_equal(b.league_laws["pursuer"][0].G, S.intercept_matrix())
    assert (b.league_law_prob, b.opponent_weighting, b.pfsp_power) == (0.5, "pfsp", 3)
    assert args_param(opponent_pool=2, league_laws={"evader": []}).league_laws == {}
    eight = ["coast"] * 8
    assert len(args_param(opponent_pool=2, league_laws={"evader": eight}).league_laws["evader"]) == 8
    # laws without a pool: refused, and the message points at scripted_opponent
    with pytest.raises(ValueError, match="scripted_opponent"):
        args_param(league_laws={"evader": ["coast"]})
    for bad in (dict(opponent_pool=2, league_laws={"evader": ["coast"] * 9}),               # nine laws
                dict(opponent_pool=2, league_laws={"referee": ["coast"]}),                  # a bad agent
                dict(opponent_pool=2, league_laws={"evader": ["orbit"]}),                   # no such builder
                dict(opponent_pool=2, league_laws={"evader": [3.0]}),
                dict(opponent_pool=2, league_laws=7),
                dict(opponent_pool=2, opponent_weighting="elo"),                            # a bad weighting
                dict(opponent_weighting="pfsp"),                                            # PFSP without a pool
                dict(opponent_pool=2, league_law_prob=-0.1), dict(opponent_pool=2, league_law_prob=float("nan")),
                dict(opponent_pool=2, league_law_prob=1.5),
                dict(opponent_pool=2, opponent_latest_prob=0.75, league_law_prob=0.5, league_laws={"evader": ["coast"]}),
                dict(opponent_pool=2, pfsp_power=0), dict(opponent_pool=2, pfsp_power=1.5),
                dict(opponent_pool=2, pfsp_power=True)):
        with pytest.raises(ValueError):
            args_param(**bad)
    # a scripted opponent together with a pool is still refused
    with pytest.raises(ValueError, match="not supported"):
        args_param(scripted_opponent="coast", opponent_pool=2)


def test_law_table_on_host_tensors():
    import torch
    from satrl import scripted as S
    tab = S.LawTable("cpu")
    assert tuple(tab.storage.shape) == (8, S.LAW_DOUBLES) and tab.storage.dtype == torch.float64 and len(tab) == 0
    base = tab.storage.data_ptr()
    a, b = S.intercept(), S.ScriptedLaw(np.arange(54.0).reshape(3, 18), [1.0, 2.0, 3.0], 0.5)
    tab.set([a, b])
    assert len(tab) == 2 and tab.storage.data_ptr() == base
    assert np.array_equal(tab.storage[0].numpy(), a.packed()) and np.array_equal(tab.storage[1].numpy(), b.packed())
    assert a.block("cpu").data_ptr() == base and b.block("cpu").data_ptr() == base + S.LAW_BYTES       # views of rows
    assert not bool(tab.storage[2:].any())
    b.update(b=[4.0, 5.0, 6.0])                              # in place: the table's row follows
    assert np.array_equal(tab.storage[1].numpy(), b.packed()) and tab.storage[1, 54].item() == 4.0
    other = S.LawTable("cpu")
    with pytest.raises(ValueError, match="another law table"):
        other.set([a])
    with pytest.raises(ValueError, match="twice"):
        tab.set([a, a])
    used = S.coast()
    used.block("cpu")                                        # a law that owns a block: launches elsewhere may read it
    with pytest.raises(ValueError, match="already owns"):
        tab.set([a, used])
    with pytest.raises(ValueError, match="at most 8"):
        tab.set([S.coast() for _ in range(9)])
    assert len(tab) == 2                                     # a refused set changes nothing
    tab.set([b])                                             # b moves to row 0, a is detached
    assert np.array_equal(tab.storage[0].numpy(), b.packed()) and not bool(tab.storage[1:].any())
    assert a._table is None and a._block is None and b.block("cpu").data_ptr() == base
    other.set([a])                                           # a detached law may join another table
    tab.set(None)
    assert len(tab) == 0 and not bool(tab.storage.any())
    with pytest.raises(ValueError):
        S.LawTable("cpu", capacity=9)
