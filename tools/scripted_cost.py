#!/usr/bin/env python3
"""Development tool (not shipped, not a test): what a scripted opponent
(args_param scripted_opponent) saves in the training rollout.

At 16384 envs and H 256 (BASELINE configs[2]'s env count and policy width) it
builds two trainers on one seed:

    off     no law: the rollout launches satrl_policy_act, both agents' MLPs
    coast   scripted.coast() on the evader: the rollout launches
            satrl_policy_act_scripted, the pursuer's MLP and a tail of 32
            workgroups that evaluate the law

Under `coast` the evader commands nothing, so the two rollouts are NOT the same
trajectories: the env step's work (fuel gating, the danger-zone count) differs
with the states it sees.  The rollout pair is therefore the figure a user gets,
and the policy launch's own share is timed separately: a captured graph of 64
launches of each entry point on the `off` trainer's last observation.

Four untimed rollouts each (graph capture, clocks), then the two alternate
over `reps` rollouts, timed with events around VecTrainer.collect(); then the
two launch graphs alternate over `reps` replays.  Prints every figure, the
medians in us per env step and per launch, the ranges, and the differences.

    python tools/scripted_cost.py [reps=8] [horizon=512]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-rl-satellite_amd"))
from satrl import scripted  # noqa: E402
from satrl.ppo import policy_act, policy_act_scripted  # noqa: E402
from satrl.trainer import VecTrainer, args_param  # noqa: E402

reps = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 8
horizon = int(sys.argv[2]) if len(sys.argv) > 2 else 512
N, LAUNCHES = 16384, 64
VARIANTS = ("off", "coast")


def rollout_ms(tr):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    tr.collect()
    ev[1].record()
    tr.buf.obs[0].copy_(tr.buf.obs[tr.T])          # the next rollout goes on from here
    tr.iteration_count += 1
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


trainers = {}
for v in VARIANTS:
    args = args_param(batch_size=N * horizon, num_envs=N, horizon=horizon, hidden_width=256, mini_batch_size=4096,
                      max_episode_steps=1000, seed=0, max_train_steps=int(3e6), chkpt_dir="/tmp",
                      scripted_opponent=None if v == "off" else {"evader": scripted.coast()})
    tr = VecTrainer(args, flag=0, d_capture=15000.0)
    for _ in range(4):                             # graph capture and warm-up, untimed
        rollout_ms(tr)
    trainers[v] = tr

times = {v: [] for v in VARIANTS}
for r in range(reps):
    for v in VARIANTS:
        ms = rollout_ms(trainers[v])
        times[v].append(ms)
        print(f"{v:6s} rep {r}: rollout {ms:9.3f} ms", flush=True)
med = {v: statistics.median(times[v]) for v in VARIANTS}
for v in VARIANTS:
    print(f"{v:6s}: median of {reps} {med[v]:9.3f} ms, range {min(times[v]):.3f} .. {max(times[v]):.3f} ms = "
          f"{1e3 * med[v] / horizon:.3f} us per step (range {1e3 * min(times[v]) / horizon:.3f} .. "
          f"{1e3 * max(times[v]) / horizon:.3f})", flush=True)
d = med["coast"] - med["off"]
print(f"coast - off = {d:+.3f} ms per rollout = {1e3 * d / horizon:+.3f} us per step ({100.0 * d / med['off']:+.2f} %)",
      flush=True)

# the policy launch alone, on the same observation
tr = trainers["off"]
obs = tr.buf.obs[tr.T].clone()
law = scripted.coast()
out = [torch.zeros((N, 3), dtype=torch.float32, device=tr.device) for _ in range(4)]


def launch(v):
    if v == "off":
        policy_act(256, obs, tr.pursuer.P, tr.evader.P, 1.6, 0, 0, 0, *out, step_base=tr.step_base)
    else:
        policy_act_scripted(256, obs, obs, tr.pursuer.P, 0, 1.6, 0, 0, 0, out[0], out[1], law, out[2],
                            step_base=tr.step_base)


graphs = {}
for v in VARIANTS:
    launch(v)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            launch(v)
    for _ in range(4):
        g.replay()
    graphs[v] = g
torch.cuda.synchronize()
ltimes = {v: [] for v in VARIANTS}
for r in range(reps):
    for v in VARIANTS:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(8):
            graphs[v].replay()
        ev[1].record()
        torch.cuda.synchronize()
        ltimes[v].append(1e3 * ev[0].elapsed_time(ev[1]) / (8 * LAUNCHES))
for v in VARIANTS:
    print(f"{v:6s} policy launch: median of {reps} {statistics.median(ltimes[v]):.3f} us, range "
          f"{min(ltimes[v]):.3f} .. {max(ltimes[v]):.3f} us (back-to-back launches in a graph)", flush=True)
print(f"coast - off = {statistics.median(ltimes['coast']) - statistics.median(ltimes['off']):+.3f} us per launch",
      flush=True)
