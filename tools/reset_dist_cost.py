#!/usr/bin/env python3
"""Development tool (not shipped, not a test): what randomised episode starts
(args_param reset_spread) cost in the training rollout.

At 16384 envs (BASELINE configs[2]'s env count and policy width) it builds two
trainers, reset_spread off and on (+-50 km / +-5 m/s around the reset's
constants), runs four untimed rollouts of each (graph capture, clocks: the
first timed rollouts of a process came out a third slower), then alternates
them over `reps` rollouts each, timed with events around VecTrainer.collect(),
and prints every figure, the medians and the difference per env step.  Two
episode lengths: max_episode_steps 1000 (the training configuration: an env
resets about once in 1000 steps) and 8 (reset-heavy: one step in 8 resets
every lane, the most the draw can cost).  With the box on, the envs are in
other states than with it off, so the difference holds the changed workload of
the step itself (other terminal and danger-zone mixes) as well as the draw.

    python tools/reset_dist_cost.py [reps=8] [horizon=512]
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
N = 16384
HALF = [50000.0] * 3 + [5.0] * 3 + [50000.0] * 3 + [5.0] * 3


def rollout_ms(tr):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    tr.collect()
    ev[1].record()
    tr.buf.obs[0].copy_(tr.buf.obs[tr.T])          # the next rollout goes on from here
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


for max_ep in (1000, 8):
    trainers = {}
    for on in (False, True):
        args = args_param(batch_size=N * horizon, num_envs=N, horizon=horizon, hidden_width=256, mini_batch_size=4096,
                          max_episode_steps=max_ep, seed=0, max_train_steps=int(3e6), chkpt_dir="/tmp",
                          reset_spread=HALF if on else None)
        tr = VecTrainer(args, flag=0, d_capture=15000.0)
        for _ in range(4):                             # graph capture and warm-up, untimed
            rollout_ms(tr)
        trainers[on] = tr
    times = {False: [], True: []}
    for r in range(reps):
        for on in (False, True):
            tr = trainers[on]
            fin0 = float(tr.env.stats[0].item())
            ms = rollout_ms(tr)
            resets = float(tr.env.stats[0].item()) - fin0
            times[on].append(ms)
            print(f"max_episode_steps {max_ep} reset_spread {int(on)} rep {r}: rollout {ms:9.3f} ms, "
                  f"{resets / horizon:9.1f} resets per step", flush=True)
    med = {on: statistics.median(times[on]) for on in (False, True)}
    for on in (False, True):
        print(f"max_episode_steps {max_ep} reset_spread {int(on)}: median of {reps} {med[on]:9.3f} ms, range "
              f"{min(times[on]):.3f} .. {max(times[on]):.3f} ms = {1e3 * med[on] / horizon:.3f} us per step",
              flush=True)
    d = med[True] - med[False]
    print(f"max_episode_steps {max_ep}: on - off = {d:+.3f} ms per rollout = {1e3 * d / horizon:+.3f} us per step "
          f"({100.0 * d / med[False]:+.2f} %)", flush=True)
    del trainers, tr
    torch.cuda.empty_cache()
