"""Scripted opponents, host side: the law's arithmetic through
satrl_scripted_act_host against a NumPy restatement (bitwise), the builders
against the env's own state transition matrix, the refusals of the C ABI
before any device call, and the args_param keyword.  No GPU."""
import ctypes as C

import numpy as np
import pytest


def _lib():
    import satrl._lib as L
    return L, L.lib()


def restated(obs, G, b, m):
    """The rule of include/satrl_ppo.h on float64 arrays: every product
    rounded to f64, then the sum, ascending j from b[d]; np.where for the
    clamp (a NaN sum fails both comparisons and passes); f32 by astype
    (round to nearest even)."""
    s = obs.astype(np.float64)
    out = np.empty((obs.shape[0], 3), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(3):
            acc = np.full(obs.shape[0], b[d], dtype=np.float64)
            for j in range(18):
                acc = acc + G[d, j] * s[:, j]
            c = np.where(acc < -m, -m, np.where(acc > m, m, acc))
            out[:, d] = c.astype(np.float32)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def raw_rows(rng, n):
    """Rows at the raw scale of the env's observation box: positions up to
    1e7 m (features 0:3, 6:9, 12:15), velocities up to 5e4 m/s."""
    scale = np.tile(np.array([1e7] * 3 + [5e4] * 3), 3)
    return (rng.uniform(-1.0, 1.0, (n, 18)) * scale).astype(np.float32)


def test_symbols_are_exported_and_bound():
    L, lib = _lib()
    want = {"satrl_scripted_act": 5, "satrl_scripted_act_host": 4, "satrl_policy_act_scripted": 16,
            "satrl_policy_eval_scripted": 16}
    for name, nargs in want.items():
        assert name in L.exported_symbols()
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    from satrl.scripted import LAW_BYTES, LAW_DOUBLES
    assert (LAW_DOUBLES, LAW_BYTES) == (58, 464)


# ---------------------------------------------------------------------------
# 1. the host kernel against NumPy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 33, 257])
def test_host_kernel_equals_numpy_restatement_bitwise(N):
    from satrl.scripted import ScriptedLaw, scripted_act_host
    rng = np.random.default_rng(100 + N)
    for scale_G, rows in ((1e-6, raw_rows(rng, N)), (0.3, rng.standard_normal((N, 18)).astype(np.float32))):
        G = rng.standard_normal((3, 18)) * scale_G
        b = rng.standard_normal(3) * 0.2
        law = ScriptedLaw(G, b, 1.6)
        got = scripted_act_host(rows, law)
        want = restated(rows, G, b, 1.6)
        assert np.array_equal(bits(got), bits(want))
        assert np.all(np.abs(got) <= np.float32(1.6))
        if N > 1:                                       # not every row is clamped, not every row is free
            assert 0 < int((np.abs(got) == np.float32(1.6)).sum()) < got.size


def test_host_kernel_saturation_zero_law_and_nan():
    from satrl.scripted import ScriptedLaw, coast, scripted_act_host
    rng = np.random.default_rng(7)
    G = rng.uniform(0.5, 1.5, (3, 18)) * 1e-3           # positive weights: a row of +-1e7 saturates every dimension
    b = rng.standard_normal(3) * 0.1
    rows = rng.standard_normal((8, 18)).astype(np.float32)
    rows[1], rows[2] = 1e7, -1e7
    rows[3, 7] = np.nan
    got = scripted_act_host(rows, ScriptedLaw(G, b, 1.6))
    want = restated(rows, G, b, 1.6)
    assert np.array_equal(bits(got), bits(want))
    assert np.all(got[1] == np.float32(1.6)) and np.all(got[2] == np.float32(-1.6))
    # every row of this G weights feature 7: the NaN reaches all three dimensions of its row and no other row
    assert np.isnan(got[3]).all() and not np.isnan(np.delete(got, 3, axis=0)).any()
    # a weight of exactly 0 does not mask a NaN feature: 0 * NaN is NaN (IEEE 754), in the restatement as
    # in the kernel, so "the dimensions whose G row weights it" are all three here too
    G2 = G.copy()
    G2[1, 7] = 0.0
    got2 = scripted_act_host(rows, ScriptedLaw(G2, b, 1.6))
    assert np.array_equal(bits(got2), bits(restated(rows, G2, b, 1.6)))
    assert np.isnan(got2[3]).all()
    # the zero law commands exactly nothing on finite rows, at any scale
    finite = np.concatenate([np.delete(rows, 3, axis=0), raw_rows(rng, 9)])
    assert np.array_equal(bits(scripted_act_host(finite, coast())), np.zeros((finite.shape[0], 3), dtype=np.uint32))
    # a small max_action clamps both sides
    got3 = scripted_act_host(finite, ScriptedLaw(G, b, 0.25))
    assert np.array_equal(bits(got3), bits(restated(finite, G, b, 0.25))) and np.abs(got3).max() == np.float32(0.25)


# ---------------------------------------------------------------------------
# 2. the intercept law nulls the relative position under the env's own matrix
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("horizon", [1, 10, 100, 400])
def test_intercept_nulls_the_relative_position(horizon):
    """dv = G s unclamped, then `horizon` steps of satrl.env.stm(100) in f64:
    |r_final| < 1e-9 |r_0| (f64 eps 1.1e-16 x cond <= 158 x <= 400 products
    is about 7e-12)."""
    from satrl.env import reset_constants, stm
    from satrl.scripted import intercept
    G = intercept(horizon).G
    assert not G[:, 6:].any()
    phi = stm(100.0)
    k = reset_constants()                               # Pp Pv Ep Ev
    rng = np.random.default_rng(horizon)
    starts = [np.concatenate([k[0:3] - k[6:9], k[3:6] - k[9:12]])]
    starts += [np.concatenate([rng.uniform(-2e5, 2e5, 3), rng.uniform(-20.0, 20.0, 3)]) for _ in range(3)]
    for x0 in starts:
        s = np.zeros(18)
        s[:6] = x0
        x = x0.copy()
        x[3:] = x[3:] + G @ s                           # the pursuer's delta-v enters the relative velocity
        for _ in range(horizon):
            x = phi @ x
        assert np.linalg.norm(x[:3]) < 1e-9 * np.linalg.norm(x0[:3]), (horizon, np.linalg.norm(x[:3]))


# ---------------------------------------------------------------------------
# 3. builders and refusals of the Python layer
# ---------------------------------------------------------------------------
def test_builder_properties_and_refusals():
    from satrl.scripted import ScriptedLaw, coast, constant, evade, intercept
    for k in (1, 10, 100):
        Gi = intercept(k).G
        for g in (0.5, 2.0, 0.25):
            assert np.array_equal(evade(k, g).G, g * Gi)
        for g in (0.3, 1.7):
            Ge = evade(k, g).G
            assert np.all(np.abs(Ge - g * Gi) <= np.spacing(np.abs(g * Gi)))
        assert np.array_equal(Gi[:, 3:6], -np.eye(3)) and not intercept(k).b.any()
    c = coast()
    assert c.G.shape == (3, 18) and not c.G.any() and not c.b.any() and c.max_action == 1.6
    t = constant([0.1, -0.2, 0.3])
    assert not t.G.any() and np.array_equal(t.b, [0.1, -0.2, 0.3])
    for k in (862, 431, 1723):                          # the steps nearest to a multiple of half the period
        with pytest.raises(ValueError):
            intercept(k)
        with pytest.raises(ValueError):
            evade(k)
    for k in (400, 430, 860, 864):                      # cond(Phi_rv) 158 ... 6.3e3: accepted
        intercept(k)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            intercept(bad)
    G = np.zeros((3, 18))
    for badG in (np.zeros((3, 17)), np.zeros((18, 3)), np.zeros(54), np.full((3, 18), np.nan),
                 np.where(np.arange(54).reshape(3, 18) == 5, np.inf, 0.0)):
        with pytest.raises(ValueError):
            ScriptedLaw(badG)
    for badb in (np.zeros(2), np.zeros((3, 1)), [0.0, np.nan, 0.0], [np.inf, 0.0, 0.0]):
        with pytest.raises(ValueError):
            ScriptedLaw(G, badb)
    for badm in (0.0, -1.6, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ScriptedLaw(G, None, badm)
    law = intercept(10)
    with pytest.raises(ValueError):
        law.update(G=np.full((3, 18), np.nan))
    assert np.array_equal(law.G, intercept(10).G)       # a refused update changes nothing
    st = law.state()
    assert all(isinstance(v, (np.ndarray, np.generic)) for v in st.values())
    back = ScriptedLaw.from_state(st)
    assert np.array_equal(back.G, law.G) and np.array_equal(back.b, law.b) and back.max_action == law.max_action


# ---------------------------------------------------------------------------
# 4. refusals of the C ABI, before any device call
# ---------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_before_any_device_call():
    """Every refusal returns -1 on the host; the fake non-null pointer is never
    dereferenced (a launch would fail with -2 on a host without a GPU)."""
    L, lib = _lib()
    fake = C.c_void_p(4096)

    def pa(H=64, N=40, obs=fake, obs_law=fake, P=fake, agent=1, act=fake, logp=fake, law=fake, act_s=fake):
        return lib.satrl_policy_act_scripted(H, N, obs, obs_law, P, agent, 1.6, 0, 0, 0, None, act, logp, law, act_s,
                                             None)

    # every refusal of satrl_policy_act
    assert pa(H=100) == -1 and pa(H=0) == -1 and pa(H=512) == -1
    assert pa(N=0) == -1 and pa(N=-3) == -1
    assert pa(obs=None) == -1 and pa(P=None) == -1 and pa(act=None) == -1 and pa(logp=None) == -1
    assert b"satrl_policy_act_scripted" in lib.satrl_ppo_last_error()
    # its own
    assert pa(obs_law=None) == -1 and pa(law=None) == -1 and pa(act_s=None) == -1
    assert b"obs_law" in lib.satrl_ppo_last_error()
    assert pa(agent=-1) == -1 and pa(agent=2) == -1
    assert b"agent" in lib.satrl_ppo_last_error()

    def pe(H=64, N=40, obs=fake, obs_law=fake, P=fake, agent=0, det=1, act=fake, law=fake, act_s=fake):
        return lib.satrl_policy_eval_scripted(H, N, obs, obs_law, P, agent, 1.6, det, 0, 0, 0, None, act, law, act_s,
                                              None)

    assert pe(H=100) == -1 and pe(N=0) == -1 and pe(obs=None) == -1 and pe(P=None) == -1 and pe(act=None) == -1
    assert pe(obs_law=None) == -1 and pe(law=None) == -1 and pe(act_s=None) == -1
    assert pe(agent=-1) == -1 and pe(agent=2) == -1
    assert pe(det=-1) == -1 and pe(det=2) == -1
    assert b"satrl_policy_eval_scripted" in lib.satrl_ppo_last_error() and b"det" in lib.satrl_ppo_last_error()

    def sa(N=40, obs=fake, law=fake, act=fake):
        return lib.satrl_scripted_act(N, obs, law, act, None)

    assert sa(N=0) == -1 and sa(N=-1) == -1 and sa(obs=None) == -1 and sa(law=None) == -1 and sa(act=None) == -1
    assert b"satrl_scripted_act" in lib.satrl_ppo_last_error()

    obs = np.zeros((2, 18), dtype=np.float32)
    act = np.zeros((2, 3), dtype=np.float32)
    law = np.zeros(58, dtype=np.float64)
    law[57] = 1.6
    po, pl, pc = (a.ctypes.data_as(C.c_void_p) for a in (obs, law, act))
    assert lib.satrl_scripted_act_host(2, po, pl, pc) == 0
    assert lib.satrl_scripted_act_host(0, po, pl, pc) == -1 and lib.satrl_scripted_act_host(-1, po, pl, pc) == -1
    assert lib.satrl_scripted_act_host(2, None, pl, pc) == -1 and lib.satrl_scripted_act_host(2, po, None, pc) == -1
    assert lib.satrl_scripted_act_host(2, po, pl, None) == -1


# ---------------------------------------------------------------------------
# 5. args_param
# ---------------------------------------------------------------------------
def test_args_param_accepts_the_three_forms():
    from satrl.scripted import ScriptedLaw, coast, intercept
    from satrl.trainer import args_param
    assert args_param().scripted_opponent == {}
    assert args_param(scripted_opponent=None).scripted_opponent == {}
    law, law2 = intercept(10), coast()
    a = args_param(scripted_opponent={"evader": law, "pursuer": law2})
    assert a.scripted_opponent["evader"] is law and a.scripted_opponent["pursuer"] is law2
    a = args_param(scripted_opponent={"pursuer": law})
    assert list(a.scripted_opponent) == ["pursuer"] and a.scripted_opponent["pursuer"] is law
    a = args_param(scripted_opponent=law)               # shorthand for {"evader": law}
    assert list(a.scripted_opponent) == ["evader"] and a.scripted_opponent["evader"] is law
    a = args_param(scripted_opponent="intercept")       # a builder's name
    got = a.scripted_opponent["evader"]
    assert isinstance(got, ScriptedLaw) and np.array_equal(got.G, intercept().G)
    assert not args_param(scripted_opponent="coast").scripted_opponent["evader"].G.any()
    for bad in ("nonsense", "constant", {"umpire": law}, {"evader": 3}, 7):
        with pytest.raises(ValueError):
            args_param(scripted_opponent=bad)
    with pytest.raises(ValueError):
        args_param(scripted_opponent=law, opponent_pool=2)
