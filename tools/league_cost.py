#!/usr/bin/env python3
"""Development tool (not shipped, not a test): what league play (args_param
league_laws) costs in the training rollout, and what the
tally kernel costs.

At 16384 envs and H 256 (BASELINE configs[2]'s env count and policy width),
on the training rollout's chunk graphs, it builds three trainers on one seed,
each with opponent_pool 8, all 8 slots filled, opponent_latest_prob 0.5:

    pool     no laws: the rollout launches satrl_policy_act_pool (the kernel as
             it was before league play)
    league0  two evader laws and league_law_prob 0: the rollout launches
             satrl_policy_act_league, and no block is ever assigned a law, so
             the members are `pool`'s -- the league kernel's own cost
    league25 league_law_prob 0.25: a quarter of the frozen agent's 512 blocks
             evaluate a law and skip the MLP

The stored sets are copies of the live evader's parameters, so `pool` and
`league0` collect the same rollout bit for bit (checked); `league25` plays
other opponents and collects another one.

Four untimed rollouts each (graph capture, clocks), then the three alternate
over `reps` rollouts, timed with events around VecTrainer.collect() (which
ends with the tally launch in all three).  `league25`'s rollouts are other
trajectories, so its env steps do other work; the policy launch's own share
is therefore timed separately, as tools/scripted_cost.py does: a captured
graph of 64 launches of each entry point on one observation, with the last
assignments of `pool` and `league25`, and with `pool`'s assignment where the
first quarter, the last quarter, every fourth or every block is put on a law
(where the law blocks lie matters more than how many there are).  Then satrl_league_tally alone on a
2048 x 16384 table: launch time and bytes / time.

    python tools/league_cost.py [reps=10] [horizon=512]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-rl-satellite_amd"))
from satrl import pool as P  # noqa: E402
from satrl.ppo import policy_act_league, policy_act_pool  # noqa: E402
from satrl.trainer import VecTrainer, args_param  # noqa: E402

reps = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 10
horizon = int(sys.argv[2]) if len(sys.argv) > 2 else 512
N, K = 16384, 8
VARIANTS = {"pool": None, "league0": 0.0, "league25": 0.25}


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
for v, law_prob in VARIANTS.items():
    kw = {} if law_prob is None else dict(league_laws={"evader": ["evade", "coast"]}, league_law_prob=law_prob)
    args = args_param(batch_size=N * horizon, num_envs=N, horizon=horizon, hidden_width=256, mini_batch_size=4096,
                      max_episode_steps=1000, seed=0, max_train_steps=int(3e6), chkpt_dir="/tmp", opponent_pool=K,
                      opponent_latest_prob=0.5, **kw)
    tr = VecTrainer(args, flag=0, d_capture=15000.0)
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
        a = tr.last_assignment
        print(f"{v:8s} rep {r}: rollout {ms:9.3f} ms, {int(((a >= 0) & (a < K)).sum()):4d} stored and "
              f"{int((a >= K).sum()):4d} law blocks of {(N + 31) // 32}", flush=True)
a, b = trainers["pool"], trainers["league0"]
same = all(torch.equal(getattr(a.buf, n), getattr(b.buf, n)) for n in ("act", "logp", "rew", "done")) and \
    torch.equal(a.other_a, b.other_a) and torch.equal(a._tally, b._tally)
print(f"pool and league0: the last rollouts and tallies are bitwise equal: {same}", flush=True)
med = {v: statistics.median(times[v]) for v in VARIANTS}
for v in VARIANTS:
    print(f"{v:8s}: median of {reps} {med[v]:9.3f} ms, range {min(times[v]):.3f} .. {max(times[v]):.3f} ms = "
          f"{1e3 * med[v] / horizon:.3f} us per step", flush=True)
for v in ("league0", "league25"):
    d = med[v] - med["pool"]
    print(f"{v} - pool = {d:+.3f} ms per rollout = {1e3 * d / horizon:+.3f} us per step "
          f"({100.0 * d / med['pool']:+.2f} %)", flush=True)
d = med["league25"] - med["league0"]
print(f"league25 - league0 = {d:+.3f} ms per rollout = {1e3 * d / horizon:+.3f} us per step", flush=True)

# The policy launch alone.  league25 plays other opponents, so its rollouts are other
# trajectories and its env steps do other work (fuel gating, the danger-zone count): the
# launch's own share is a captured graph of 64 launches of each entry point on ONE
# observation (the pool trainer's last), with the pool trainer's parameters, pool and law
# table of league25 and the last assignments of `pool` (no law block) and `league25`.
LAUNCHES = 64
tr, t25 = trainers["pool"], trainers["league25"]
obs = tr.buf.obs[tr.T].clone()
out = [torch.zeros((N, 3), dtype=torch.float32, device=tr.device) for _ in range(4)]
store, table = tr.pools["evader"].storage, t25._league["evader"]
member = {"pool": tr.member.clone(), "league0": tr.member.clone(), "league25": t25.member.clone()}
# ... and where the law blocks lie: `pool`'s assignment with a quarter of the blocks (the
# first, the last, every fourth: all of those on one XCD) or all of them put on a law
nb = (N + 31) // 32
for name, idx in (("first", range(nb // 4)), ("last", range(nb - nb // 4, nb)), ("every4th", range(0, nb, 4)),
                  ("all", range(nb))):
    m = tr.member.clone()
    m[list(idx)] = K
    member[name] = m


def launch(v):
    if v == "pool":
        policy_act_pool(256, obs, tr.pursuer.P, tr.evader.P, 1.6, 0, 0, 0, *out, 1, store, member[v],
                        step_base=tr.step_base)
    else:
        policy_act_league(256, obs, obs, tr.pursuer.P, tr.evader.P, 1.6, 0, 0, 0, *out, 1, store, member[v], table,
                          step_base=tr.step_base)


graphs = {}
for v in member:
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
ltimes = {v: [] for v in member}
for r in range(reps):
    for v in member:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(8):
            graphs[v].replay()
        ev[1].record()
        torch.cuda.synchronize()
        ltimes[v].append(1e3 * ev[0].elapsed_time(ev[1]) / (8 * LAUNCHES))
lmed = {v: statistics.median(ltimes[v]) for v in member}
for v in member:
    print(f"{v:8s} policy launch: median of {reps} {lmed[v]:.3f} us, range {min(ltimes[v]):.3f} .. "
          f"{max(ltimes[v]):.3f} us (back-to-back launches in a graph, {int((member[v] >= K).sum())} law blocks)",
          flush=True)
for v in list(member)[1:]:
    print(f"{v} - pool = {lmed[v] - lmed['pool']:+.3f} us per launch", flush=True)
del trainers, graphs, a, b, tr, t25, store, table
torch.cuda.empty_cache()

# the tally kernel alone, at BASELINE configs[2]'s rollout table
T = 2048
rew = torch.full((T, N), -1.0, dtype=torch.float32, device="cuda")
done = torch.zeros((T, N), dtype=torch.uint8, device="cuda")
done[999::1000] = 1
rew[999::1000] = 150.0
tally = torch.zeros(((N + 31) // 32, 2), dtype=torch.int64, device="cuda")
for _ in range(3):
    P.league_tally(rew, done, 150.0, tally)
torch.cuda.synchronize()
ts = []
for _ in range(10):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    P.league_tally(rew, done, 150.0, tally)
    ev[1].record()
    torch.cuda.synchronize()
    ts.append(ev[0].elapsed_time(ev[1]))
assert int(tally[:, 0].sum()) == 13 * 2 * N and torch.equal(tally[:, 0], tally[:, 1])
nbytes = 5 * T * N
m = statistics.median(ts)
print(f"satrl_league_tally {T} x {N}: median of 10 {1e3 * m:.1f} us, range {1e3 * min(ts):.1f} .. {1e3 * max(ts):.1f} us; "
      f"{nbytes / 1e6:.1f} MB read = {nbytes / m / 1e9:.3f} TB/s", flush=True)
