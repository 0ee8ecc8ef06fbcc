"""bench.py's N-rank path on a 1-GPU box: `--gpus 2 --one-device` runs two
ranks (gloo, both on cuda:0; RCCL refuses two ranks on one GPU) through the
whole bench (`--full`) -- launch, rollout + GAE + update per rank, barrier +
max-over-ranks timing, the data-parallel measurements and the configs[3]-
semantics slice -- and rank 0 alone prints the JSON line (the driver's 8-GPU
run uses the same code path with RCCL).  And the plain run: the headline
line alone, `--steps` timed iterations, `--dump-outputs`."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("allreduce", ["rccl", "peer"])
def test_bench_two_ranks_one_device(allreduce):
    """... and with --allreduce peer the whole update runs through the peer
    all-reduce kernel (IPC within the device); either way the line carries
    the peer kernel's all-reduce time beside the c10d path.  Both at the
    product's hidden width (256).

    Both ranks share ONE device here, so rank 0's peer all-reduce waves spin
    on CUs while rank 1's next kernel must still be placed: the peer grid is
    at most one 256-thread workgroup per CU (satrl_peer_blocks), i.e. one
    spinning wave per SIMD, which leaves every CU room for a 16-wave rowpass
    workgroup (a 641-block grid, up to three spinning waves per SIMD, starved
    it in round 4).  The peer waits are bounded by SATRL_DP_TIMEOUT_S (30 s
    here, so a stall fails the test instead of the box's hang check)."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["SATRL_DP_TIMEOUT_S"] = "30"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--one-device",
                        "--num-envs", "512", "--horizon", "32", "--epochs", "1", "--minibatch", "4096",
                        "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--kernel-iters", "10",
                        "--global-slice", "8", "--allreduce", allreduce], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2"
    assert out["value"] > 0 and out["cpu_baseline"] is None
    dp = out["data_parallel"]
    assert dp["world"] == 2 and dp["backend"] == "gloo"
    sl = dp["configs3_semantics_slice"]
    assert sl["rows_per_rank"] == 2048 and sl["us_per_global_minibatch_step"] > 0
    assert dp["allreduce"] == allreduce and dp["peer_allreduce_error"] is False and dp["peer_allreduce_us"] > 0


def test_bench_one_gpu_line_keeps_the_contract():
    """The N = 1 line of a `--full` run: one JSON line with the contract's
    keys, the rowpass roofline (achieved = FLOP per launch / launch time,
    frac = achieved / peak) and a bounded CPU baseline of the same workload."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--num-envs", "1024",
                        "--horizon", "64", "--epochs", "1", "--minibatch", "4096", "--steps", "1", "--warmup", "1",
                        "--kernel-iters", "10", "--cpu-baseline-seconds", "1"],
                       env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert out["metric"] == base["metric"] and out["unit"] == "env-steps/s"
    assert out["n_gpus"] == 1 and out["steps"] == 1 and out["warmup"] == 1
    assert out["higher_is_better"] is True and out["scaling"] == "weak" and out["vs_baseline"] is None
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 1024 * 64 / (out["ms_per_step"] / 1e3)) <= 1e-6 * out["value"]
    assert "workload" in out["config"] and out["config"]["parallelism"] == "dp1"
    rf = out["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == 157.3
    assert rf["achieved"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert abs(rf["achieved"] - rf["flop_per_launch"] / rf["avg_launch_us"] / 1e6) <= 1e-6 * rf["achieved"]
    cb = out["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("port", "reference") and cb["sample"]


def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """`bench.py --steps K --warmup W` without --full: the line holds the
    headline (value = env-steps of the K timed iterations / their time,
    ms_per_step) and none of the measurements that take runs of their own.
    --dump-outputs writes the last timed iteration's outputs as float32 /
    float64 .npy files, and a second run with the same arguments rolls out
    the same table (seeded init, Philox noise keyed by env and step: with no
    warm-up the first rollout depends on nothing else), bit for bit."""
    import numpy as np
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    N, T = 512, 16
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1",
                            "--warmup", "0", "--num-envs", str(N), "--horizon", str(T), "--hidden", "64",
                            "--epochs", "1", "--minibatch", "1024", "--dump-outputs", str(d)],
                           env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64+f32"
        assert out["n_gpus"] == 1 and out["steps"] == 1 and out["warmup"] == 0
        assert out["value"] > 0 and out["ms_per_step"] > 0
        assert abs(out["value"] - N * T / (out["ms_per_step"] / 1e3)) <= 1e-6 * out["value"]
        for k in ("roofline", "roofline_env", "roofline_policy", "cpu_baseline", "propagators", "surrogate",
                  "reachable_domain", "rollout_sweep_num_envs", "data_parallel"):
            assert k not in out, k
        files = sorted(os.listdir(d))
        assert files == sorted(n + ".npy" for n in ("stats", "sample_index", "params", "obs", "act", "logp", "rew",
                                                    "done", "values", "adv", "vtarget"))
        arrs = {f[:-4]: np.load(d / f) for f in files}
        assert all(v.dtype in (np.float32, np.float64) for v in arrs.values())
        assert sum(v.nbytes for v in arrs.values()) <= 64 << 20
        rows = arrs["sample_index"].astype(np.int64)
        assert len(rows) == N * T and rows.min() >= N and rows.max() < N * T and (np.diff(rows) >= 0).all()
        assert arrs["obs"].shape == (len(rows), 18) and arrs["act"].shape == arrs["logp"].shape == (len(rows), 3)
        for k in ("rew", "done", "values", "adv", "vtarget"):
            assert arrs[k].shape == (len(rows),), k
        assert all(np.isfinite(v).all() for v in arrs.values())
        assert set(np.unique(arrs["done"])) <= {0.0, 1.0}
        dumps.append(arrs)
    for k in ("sample_index", "obs", "act", "logp", "rew", "done"):
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
