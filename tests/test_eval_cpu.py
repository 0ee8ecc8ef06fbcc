"""Host side of the evaluation path (no GPU): the argument checks of
satrl_policy_eval / satrl_episode_record_reset / satrl_episode_record, the
numpy reference recorder on a hand-written stream, and the pure-Python
pieces of satrl/evaluate.py."""
import ctypes as C

import numpy as np
import pytest

import eval_reference as R


def test_eval_entry_points_reject_bad_arguments_before_any_device_call():
    """Every rejection returns -1 on the host; the fake non-null pointer is
    never dereferenced (a launch would fail with -2 on a host without a GPU)."""
    import satrl._lib as L
    lib = L.lib()
    fake = C.c_void_p(16)

    def pe(H=256, N=8, obs=fake, P0=fake, P1=fake, det=1, sb=None, act0=fake, act1=fake):
        return lib.satrl_policy_eval(H, N, obs, P0, P1, 1.6, det, 0, 0, 0, sb, act0, act1, None)

    assert pe(H=100) == -1 and pe(H=0) == -1 and pe(H=512) == -1      # H not 64 / 128 / 256
    assert pe(N=0) == -1 and pe(N=-3) == -1
    assert pe(obs=None) == -1 and pe(P0=None) == -1 and pe(act0=None) == -1
    assert pe(det=-1) == -1 and pe(det=4) == -1                        # det_mask outside 0..3
    assert pe(P1=None, act1=None, det=2) == -1 and pe(P1=None, act1=None, det=3) == -1   # bit 1 without P1
    assert pe(act1=None) == -1                                          # second agent without its output
    for H in (64, 128, 256):
        assert pe(H=H, N=0) == -1

    assert lib.satrl_episode_record_reset(0, fake, fake, fake, None) == -1
    assert lib.satrl_episode_record_reset(-1, fake, fake, fake, None) == -1
    for k in range(3):
        a = [fake] * 3
        a[k] = None
        assert lib.satrl_episode_record_reset(8, *a, None) == -1, k
    assert b"satrl_episode_record_reset" in lib.satrl_last_error()

    def er(N=8, null=None):
        p = [fake] * 8                      # reward, done, obs64, pa, ea | rec_f64, rec_i32, alive
        if null is not None:
            p[null] = None
        return lib.satrl_episode_record(N, *p[:5], 100.0, *p[5:], None)

    assert er(N=0) == -1 and er(N=-1) == -1
    for k in range(8):
        assert er(null=k) == -1, k
    assert b"satrl_episode_record" in lib.satrl_last_error()


def test_reference_recorder_on_a_hand_written_stream():
    """Three envs, four steps, capture literal 100.  env 0: never done.
    env 1: captured at step 2, later steps (a second done among them) ignored.
    env 2: reward 100 on a step that is not done (not classified), then done
    with the timeout literal 0 at step 3."""
    reward = np.array([[1.0, 1e17, 100.0],
                       [2.0, 100.0, 1.0],
                       [-0.5, 7.0, 0.0],
                       [0.25, 100.0, 9.0]])
    done = np.array([[0, 0, 0],
                     [0, 1, 0],
                     [0, 0, 1],
                     [0, 1, 1]], np.uint8)
    obs64 = np.zeros((4, 3, 18))
    obs64[:, 0, :3] = [[3, 4, 0], [0, 0, 2], [6, 8, 0], [1, 2, 2]]           # dis 5, 2, 10, 3
    obs64[:, 1, :3] = [[0, 5, 12], [8, 0, 6], [0, 0, 1], [0, 0, 0.5]]         # dis 13, 10, (1), (0.5)
    obs64[:, 2, :3] = [[2, 3, 6], [1, 4, 8], [4, 4, 7], [0, 0, 0.25]]         # dis 7, 9, 9, (0.25)
    obs64[:, :, 3:] = 123.0                                                   # not read
    pa = np.zeros((4, 3, 3), np.float32)
    ea = np.zeros((4, 3, 3), np.float32)
    pa[:, 0] = [[1, -1, 0.5], [0, 0, 0], [-0.25, 0.25, 0], [1.5, 0, 0]]       # 2.5, 0, 0.5, 1.5
    pa[:, 1] = [[1, 1, 1], [-0.5, 0, 0], [9, 9, 9], [9, 9, 9]]                # 3, 0.5, then ignored
    pa[:, 2] = [[0, 0, 1], [0, -1, 0], [1, 0, 0], [9, 9, 9]]                  # 1, 1, 1, then ignored
    ea[:, 0] = [[0.5, 0, 0], [0, 0.5, 0], [0, 0, -0.5], [0.5, 0.5, 0.5]]      # 0.5, 0.5, 0.5, 1.5
    ea[:, 1] = [[0, 0, 0], [1.5, -1.5, 1.5], [9, 9, 9], [9, 9, 9]]            # 0, 4.5
    ea[:, 2] = [[-1, -1, 0], [0, 0, 0], [0, 0.125, 0], [9, 9, 9]]             # 2, 0, 0.125
    rec0 = R.record_reset(3)
    assert rec0["alive"] == 3 and np.isnan(rec0["final_dis"]).all() and np.isposinf(rec0["min_dis"]).all()
    rec, alive = R.record_streams(reward, done, obs64, pa, ea, 100.0)
    assert alive == [3, 2, 1, 1]
    assert rec["ret"].tolist() == [2.75, 1e17 + 100.0, 101.0]       # (one f64 addition, rounded as it rounds)
    assert rec["length"].tolist() == [4, 2, 3]
    assert rec["outcome"].tolist() == [0, 1, 2]
    assert rec["min_dis"].tolist() == [2.0, 10.0, 7.0]
    assert np.isnan(rec["final_dis"][0]) and rec["final_dis"][1:].tolist() == [10.0, 9.0]
    assert rec["dv_p"].tolist() == [4.5, 3.5, 3.0]
    assert rec["dv_e"].tolist() == [3.0, 4.5, 2.125]
    # the sum runs in step order: the other order loses the 1 next to 1e17
    r2 = np.array([[1.0], [1e17], [-1e17]])
    z = np.zeros((3, 1, 18)); a = np.zeros((3, 1, 3), np.float32)
    rec2, _ = R.record_streams(r2, np.zeros((3, 1), np.uint8), z, a, a, 100.0)
    assert rec2["ret"][0] == (1.0 + 1e17) - 1e17 == 0.0
    R.assert_records_equal(rec, rec)
    bad = {k: np.copy(v) for k, v in rec.items() if k != "alive"}
    bad["min_dis"][0] *= 1 + 4e-15
    with pytest.raises(AssertionError):
        R.assert_records_equal(bad, rec)


def test_det_mask_and_capture_literal():
    from satrl import env as E
    from satrl.evaluate import EVAL_SEED_XOR, capture_reward_of, det_mask_of
    assert det_mask_of("learner", 0) == 1 and det_mask_of("learner", 1) == 2
    assert det_mask_of("both", 0) == 3 and det_mask_of("none", 1) == 0
    assert det_mask_of({"pursuer"}, 1) == 1 and det_mask_of(["evader"], 0) == 2
    assert det_mask_of(("pursuer", "evader"), 0) == 3 and det_mask_of((), 0) == 0
    with pytest.raises(ValueError):
        det_mask_of("mean", 0)
    with pytest.raises(ValueError):
        det_mask_of({"chaser"}, 0)
    p = E.default_params()
    assert capture_reward_of(p, 0) == p.win_reward and capture_reward_of(p, 1) == -150.0
    with pytest.raises(ValueError):
        capture_reward_of(E.default_params(burn_reward=p.win_reward), 0)     # Flag 0: both literals equal
    with pytest.raises(ValueError):
        capture_reward_of(E.default_params(win_reward=-150.0), 1)            # Flag 1: both literals equal
    with pytest.raises(ValueError):
        capture_reward_of(p, 2)
    assert EVAL_SEED_XOR != 0                       # the default evaluation seed differs from args.seed


def test_exports_and_signatures():
    import satrl._lib as L
    from satrl import ppo
    from satrl.trainer import VecTrainer
    for name in ("satrl_policy_eval", "satrl_episode_record", "satrl_episode_record_reset"):
        assert name in L.exported_symbols() and hasattr(L.lib(), name)
    assert ppo.REC_F64 == R.REC_F64 and ppo.REC_I32 == R.REC_I32
    assert callable(ppo.policy_eval) and callable(ppo.episode_record) and callable(ppo.episode_record_reset)
    assert callable(VecTrainer.evaluate)
