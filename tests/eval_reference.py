"""numpy restatement of the episode records (include/satrl_rollout.h
satrl_episode_record_reset / satrl_episode_record): a plain loop in f64 in the
kernel's order, shared by tests/test_eval_cpu.py and tests/test_eval_gpu.py."""
import numpy as np

REC_F64 = ["ret", "final_dis", "min_dis", "dv_p", "dv_e"]
REC_I32 = ["length", "outcome"]
DIS_RTOL = 1e-15      # a contracted vs an uncontracted sum of three squares <= 1.5 ulp, plus a correctly
#                       rounded sqrt: 1e-15 is about 4.5 ulp of an f64


def record_reset(N):
    return {"ret": np.zeros(N), "final_dis": np.full(N, np.nan), "min_dis": np.full(N, np.inf),
            "dv_p": np.zeros(N), "dv_e": np.zeros(N), "length": np.zeros(N, np.int32),
            "outcome": np.zeros(N, np.int32), "alive": int(N)}


def _abs_sum3(a):
    a = np.abs(a.astype(np.float64))
    return (a[0] + a[1]) + a[2]


def record_step(rec, reward, done, obs64, pa, ea, capture_reward):
    """One satrl_episode_record call on the dict of record_reset, in place."""
    for i in range(len(reward)):
        if rec["outcome"][i] != 0:
            continue
        o = obs64[i]
        dis = np.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
        rec["ret"][i] += reward[i]
        rec["dv_p"][i] += _abs_sum3(pa[i])
        rec["dv_e"][i] += _abs_sum3(ea[i])
        rec["length"][i] += 1
        if dis < rec["min_dis"][i]:
            rec["min_dis"][i] = dis
        if done[i]:
            rec["final_dis"][i] = dis
            rec["outcome"][i] = 1 if reward[i] == capture_reward else 2
            rec["alive"] -= 1
    return rec


def record_streams(reward, done, obs64, pa, ea, capture_reward):
    """The records after the whole [T, N, ...] streams, and alive after every step."""
    rec = record_reset(reward.shape[1])
    alive = []
    for t in range(reward.shape[0]):
        record_step(rec, reward[t], done[t], obs64[t], pa[t], ea[t], capture_reward)
        alive.append(rec["alive"])
    return rec, alive


def assert_records_equal(got, ref):
    """got / ref: dicts of numpy arrays by record name.  Sums, counts and
    outcomes exactly; distances within DIS_RTOL, with NaN / inf where the
    reference has them."""
    for k in ("ret", "dv_p", "dv_e", "length", "outcome"):
        assert np.array_equal(got[k], ref[k]), k
    for k in ("final_dis", "min_dis"):
        fin = np.isfinite(ref[k])
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
        assert np.array_equal(np.isposinf(got[k]), np.isposinf(ref[k])), k
        assert np.allclose(got[k][fin], ref[k][fin], rtol=DIS_RTOL, atol=0.0), k
