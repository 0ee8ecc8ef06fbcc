#!/usr/bin/env python3
"""Development tool (not shipped, not a test): what the opponent pool
(args_param opponent_pool) costs in the training rollout.

At 16384 envs and H 256 (BASELINE configs[2]'s env count and policy width) it
builds three trainers on one seed:

    off     no pool: the rollout launches satrl_policy_act
    empty   opponent_pool 8 with no slot filled: every block's member is -1, so
            the pooled kernel acts with the live parameters, the kernel's own
            cost (one dependent scalar load per workgroup, its argument list)
            with the weight footprint unchanged
    filled  opponent_pool 8, all 8 slots filled, opponent_latest_prob 0.5: half
            of the frozen agent's 512 blocks stream one of eight stored sets,
            nine address ranges of about 280 KB each instead of one

The stored sets are copies of the live evader's parameters: the same numbers at
eight other addresses.  The three trainers then collect the same rollout bit
for bit (checked), so the env step's workload is the same in all three and the
differences are the policy launch's alone; the caches see eight more weight
streams whatever the numbers in them are.

Four untimed rollouts each (graph capture, clocks), then the three alternate
over `reps` rollouts, timed with events around VecTrainer.collect().  Prints
every figure, the medians in us per env step, and the differences to `off`.

    python tools/pool_cost.py [reps=8] [horizon=512]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-rl-satellite_amd"))
from satrl.trainer import VecTrainer, args_param  # noqa: E402

reps = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 8
horizon = int(sys.argv[2]) if len(sys.argv) > 2 else 512
N, K = 16384, 8
VARIANTS = ("off", "empty", "filled")


def rollout_ms(tr):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    tr.collect()
    ev[1].record()
    tr.buf.obs[0].copy_(tr.buf.obs[tr.T])          # the next rollout goes on from here
    tr.iteration_count += 1                        # ... under the next iteration's assignment
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


trainers = {}
for v in VARIANTS:
    args = args_param(batch_size=N * horizon, num_envs=N, horizon=horizon, hidden_width=256, mini_batch_size=4096,
                      max_episode_steps=1000, seed=0, max_train_steps=int(3e6), chkpt_dir="/tmp",
                      opponent_pool=0 if v == "off" else K, opponent_latest_prob=0.5)
    tr = VecTrainer(args, flag=0, d_capture=15000.0)
    if v == "filled":
        for _ in range(K):
            tr.snapshot_opponent("evader")
    for _ in range(4):                             # graph capture and warm-up, untimed
        rollout_ms(tr)
    trainers[v] = tr

times = {v: [] for v in VARIANTS}
for r in range(reps):
    for v in VARIANTS:
        tr = trainers[v]
        ms = rollout_ms(tr)
        times[v].append(ms)
        stored = int((tr.last_assignment >= 0).sum()) if tr.pools is not None else 0
        print(f"{v:6s} rep {r}: rollout {ms:9.3f} ms, {stored:4d} of {(N + 31) // 32} blocks on a stored set",
              flush=True)
same = all(torch.equal(trainers["off"].buf.act, trainers[v].buf.act) and
           torch.equal(trainers["off"].buf.rew, trainers[v].buf.rew) for v in VARIANTS[1:])
print(f"the three trainers' last rollouts are bitwise equal: {same}", flush=True)
med = {v: statistics.median(times[v]) for v in VARIANTS}
for v in VARIANTS:
    print(f"{v:6s}: median of {reps} {med[v]:9.3f} ms, range {min(times[v]):.3f} .. {max(times[v]):.3f} ms = "
          f"{1e3 * med[v] / horizon:.3f} us per step", flush=True)
for v in VARIANTS[1:]:
    d = med[v] - med["off"]
    print(f"{v} - off = {d:+.3f} ms per rollout = {1e3 * d / horizon:+.3f} us per step "
          f"({100.0 * d / med['off']:+.2f} %)", flush=True)
