#!/usr/bin/env python3
"""Development tool (not shipped, not a test): what obs_norm + reward_scaling
cost, and what they buy at fc1.

For BASELINE configs[2] (16384 envs x 2048 steps, H 256, mb 4096, 10 epochs)
and then configs[1] (4096 envs x 2048 steps, H 64) it builds two trainers,
with the two keywords off and on, runs one untimed iteration of each (graph
capture), then alternates them over `reps` iterations each and prints the
rollout / GAE / update milliseconds of VecTrainer.iteration(timers) and their
medians.  Before the first iteration it prints, for the initial policy on the
rollout's first chunk, the share of the actor's fc1 outputs with
|tanh| > 0.999, with and without obs_norm.

    python tools/norm_cost.py [reps=3] [epochs=10]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-rl-satellite_amd"))
from satrl.trainer import VecTrainer, args_param  # noqa: E402

reps = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 3
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 10
SHAPES = [("configs[2]", dict(num_envs=16384, horizon=2048, hidden_width=256, mini_batch_size=4096)),
          ("configs[1]", dict(num_envs=4096, horizon=2048, hidden_width=64, mini_batch_size=4096))]


def saturation(tr):
    """Share of |tanh(fc1(obs))| > 0.999 over the first chunk's observations (the actor's fc1)."""
    obs = tr.buf.obs[:tr.chunk].reshape(-1, 18)
    with torch.no_grad():
        h = torch.tanh(tr.learner.actor.fc1(obs))
    return float((h.abs() > 0.999).float().mean())


for name, shape in SHAPES:
    trainers = {}
    for on in (False, True):
        args = args_param(batch_size=shape["num_envs"] * shape["horizon"], K_epochs=epochs, max_episode_steps=1000,
                          seed=0, max_train_steps=int(3e6), chkpt_dir="/tmp", obs_norm=on, reward_scaling=on,
                          **shape)
        tr = VecTrainer(args, flag=0, d_capture=15000.0)
        tr.collect()                                   # the initial policy's rollout
        torch.cuda.synchronize()
        print(f"{name} norm {int(on)}: fc1 |tanh| > 0.999 on the first chunk ({tr.chunk} steps x {tr.N} envs): "
              f"{100.0 * saturation(tr):.2f} %", flush=True)
        tr.compute_advantages()
        tr.update()
        tr.finish_iteration()
        torch.cuda.synchronize()
        trainers[on] = tr
    times = {False: {}, True: {}}
    for r in range(reps):
        for on in (False, True):
            t = {}
            trainers[on].iteration(t)
            for k, v in t.items():
                times[on].setdefault(k, []).append(v[0])
            print(f"{name} norm {int(on)} rep {r}: rollout {t['rollout_ms'][0]:8.2f} gae {t['gae_ms'][0]:7.2f} "
                  f"update {t['update_ms'][0]:9.2f} ms", flush=True)
    for on in (False, True):
        m = {k: statistics.median(v) for k, v in times[on].items()}
        print(f"{name} norm {int(on)} median of {reps}: rollout {m['rollout_ms']:8.2f} gae {m['gae_ms']:7.2f} "
              f"update {m['update_ms']:9.2f} ms", flush=True)
    off, on_ = times[False], times[True]
    d = statistics.median(on_["rollout_ms"]) - statistics.median(off["rollout_ms"])
    print(f"{name}: rollout +{d:.2f} ms = {1e3 * d / shape['horizon']:.2f} us per step; gae "
          f"+{statistics.median(on_['gae_ms']) - statistics.median(off['gae_ms']):.2f} ms", flush=True)
    del trainers, tr
    torch.cuda.empty_cache()
