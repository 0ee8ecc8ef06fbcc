#!/usr/bin/env python3
"""Development tool (not shipped, not a test): what observation noise
(args_param obs_noise) costs in the training rollout, and whether a trainer
without it still runs at the parent commit's speed.

At 16384 envs, H 256 and max_episode_steps 1000 (BASELINE configs[2]'s env
count and policy width) a measuring process builds two trainers, obs_noise off
and on (both tracked craft, bias and refreshed error, --spec and --hold), runs
four untimed rollouts of each (graph capture, clocks), then alternates them
over `reps` rollouts each, timed with events around VecTrainer.collect(), and
prints every figure and the medians per env step (both policies, sampling, env
step).  With the noise on the policies act on other rows, so the envs are in
other states than with it off: the difference holds the changed workload of
the step itself as well as the six Philox blocks per env.

With --parent DIR (a checkout of the parent commit with its library built),
this process only drives: it starts `rounds` fresh measuring processes of each
tree, alternating parent, this tree, parent, ...; a parent's process builds
two trainers as well, both without noise (the parent has nothing else), so
that the two kinds of process hold the same memory and alternate alike.  The
summary gives the parent's median and range over all its rollouts beside this
tree's noise-off and noise-on ones.  --spec BIAS_POS,BIAS_VEL,POS,VEL: other
half-widths; 0,0,0,0 is an enabled noise that draws nothing, i.e. the
measuring kernels and their block loads alone.

    python tools/obs_noise_cost.py [reps=8] [horizon=512] [--parent DIR] [--rounds 3]
                                   [--spec 120,0.04,35,0.015] [--hold 1]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16384

ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=8)
ap.add_argument("horizon", nargs="?", type=int, default=512)
ap.add_argument("--parent", metavar="DIR", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--spec", default="120,0.04,35,0.015", help="BIAS_POS,BIAS_VEL,POS,VEL of both craft with the noise on")
ap.add_argument("--hold", type=int, default=1)
ap.add_argument("--measure", choices=("tree", "parent"), default=None, help="(internal) a measuring process")
opt = ap.parse_args()
reps, horizon = max(3, opt.reps), opt.horizon
CRAFT = dict(zip(("bias_pos", "bias_vel", "pos", "vel"), (float(x) for x in opt.spec.split(","))))
SPEC = {"pursuer": CRAFT, "evader": CRAFT, "hold": opt.hold}


def measure(tree, tag, with_noise):
    """One measuring process: trainers of `tree`, one line per timed rollout."""
    sys.path.insert(0, os.path.join(tree, "ppo-rl-satellite_amd"))
    import torch
    from satrl.trainer import VecTrainer, args_param

    def rollout_ms(tr):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        tr.collect()
        ev[1].record()
        tr.buf.obs[0].copy_(tr.buf.obs[tr.T])          # the next rollout goes on from here
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    trainers = {}
    for on in (False, True):
        kw = dict(obs_noise=SPEC) if on and with_noise else {}
        args = args_param(batch_size=N * horizon, num_envs=N, horizon=horizon, hidden_width=256, mini_batch_size=4096,
                          max_episode_steps=1000, seed=0, max_train_steps=int(3e6), chkpt_dir="/tmp", **kw)
        tr = VecTrainer(args, flag=0, d_capture=15000.0)
        for _ in range(4):                             # graph capture and warm-up, untimed
            rollout_ms(tr)
        trainers[on] = tr
    for r in range(reps):
        for on, tr in trainers.items():                # (a parent's two trainers are both "obs_noise 0")
            print(f"ROLLOUT {tag} obs_noise {int(on and with_noise)} rep {r}: {rollout_ms(tr):9.3f} ms", flush=True)


def summary(name, ms):
    med = statistics.median(ms)
    print(f"{name}: median of {len(ms)} {med:9.3f} ms, range {min(ms):.3f} .. {max(ms):.3f} ms = "
          f"{1e3 * med / horizon:.3f} us per step "
          f"(range {1e3 * min(ms) / horizon:.3f} .. {1e3 * max(ms) / horizon:.3f})", flush=True)
    return med


def parse(text, times):
    for line in text.splitlines():
        if line.startswith("ROLLOUT "):
            _, tag, _, on, *_ = line.split()
            times.setdefault((tag, int(on)), []).append(float(line.split(":")[1].split()[0]))


if opt.measure:
    measure(opt.parent if opt.measure == "parent" else ROOT, opt.measure, opt.measure == "tree")
    sys.exit(0)

common = [str(reps), str(horizon), "--spec", opt.spec, "--hold", str(opt.hold)]
times = {}
if opt.parent is None:
    out = subprocess.run([sys.executable, __file__, *common, "--measure", "tree"], check=True, stdout=subprocess.PIPE,
                         text=True).stdout
    print(out, end="", flush=True)
    parse(out, times)
else:
    parent = os.path.abspath(opt.parent)
    for rnd in range(max(1, opt.rounds)):
        for which in ("parent", "tree"):
            out = subprocess.run([sys.executable, __file__, *common, "--measure", which, "--parent", parent],
                                 check=True, stdout=subprocess.PIPE, text=True).stdout
            print(f"round {rnd}, {which}:\n{out}", end="", flush=True)
            parse(out, times)
med = {k: summary(f"{k[0]} obs_noise {k[1]}", v) for k, v in sorted(times.items())}
off, on = med[("tree", 0)], med[("tree", 1)]
print(f"on - off = {on - off:+.3f} ms per rollout = {1e3 * (on - off) / horizon:+.3f} us per step "
      f"({100.0 * (on - off) / off:+.2f} %)", flush=True)
if ("parent", 0) in med:
    par = med[("parent", 0)]
    for name, v in (("off", off), ("on", on)):
        print(f"{name} - parent = {v - par:+.3f} ms per rollout = {1e3 * (v - par) / horizon:+.3f} us per step "
              f"({100.0 * (v - par) / par:+.2f} %)", flush=True)
