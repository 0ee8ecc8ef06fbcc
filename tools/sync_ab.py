#!/usr/bin/env python3
"""Development tool (not shipped, not a test): the two synchronisation forms
of the 32-row H 256 rowpass (satrl_ppo_rowpass_sync: 0 barriers, 1 LDS
hand-offs) against each other inside ONE process, on the same learner, rows
and buffers: the update graph is captured again after each switch, and the
forms alternate, barrier first and last.  The in-graph minibatch step
(event-timed replays of 16-minibatch groups) and the rowpass's live span
(satrl_span_probe) per turn; no allocation or placement differs between the
two, which a library-against-library A/B (tools/ab_spans.sh) cannot say.
Usage: python tools/sync_ab.py [mb] [turns] [replays per timed window]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-rl-satellite_amd"))
from satrl.ppo import FusedMinibatch, PPOLearner, rowpass_exchange_check, rowpass_sync  # noqa: E402
from satrl.spans import SpanProbe  # noqa: E402
from satrl.trainer import args_param  # noqa: E402

H = 256
mb = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
turns = int(sys.argv[2]) if len(sys.argv) > 2 else 4
nrep = int(sys.argv[3]) if len(sys.argv) > 3 else 1000      # (1000 x 16 steps: most of a second at mb 4096)
B = 16 * mb
L = PPOLearner(args_param(hidden_width=H, mini_batch_size=mb, batch_size=B, chkpt_dir="/tmp"), "pursuer",
               graph_group=16)
g = torch.Generator(device="cuda").manual_seed(0)
src = torch.randn((B, 32), device="cuda", generator=g)
src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
perm = torch.randperm(B, device="cuda", generator=g)
L.sync_w2t()
st = FusedMinibatch(L, mb, 16)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def turn(mode, n=nrep):
    rowpass_sync(mode)
    st.graph = None                                  # the next run captures the graph in this form
    for _ in range(3):
        st.run(src, perm)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        st.run(src, perm)
    e1.record()
    torch.cuda.synchronize()
    step = e0.elapsed_time(e1) * 1e3 / (n * 16)
    with SpanProbe(64 << 20) as pr:
        st.graph = None
        for _ in range(3):
            st.run(src, perm)
        torch.cuda.synchronize()
    st.graph = None
    s = pr.summary()
    return step, s["rowpass"]["median_us"]


prev = rowpass_sync()
names = {0: "barrier ", 1: "hand-off"}
res = {0: [], 1: []}
for k in range(2 * turns + 1):
    mode = k & 1
    step, span = turn(mode)
    res[mode].append(step)
    print(f"[{names[mode]}] H {H} mb {mb}: step {step:6.2f} us | rowpass span median {span:6.2f}", flush=True)
rowpass_sync(prev)
rowpass_exchange_check()
for mode, v in res.items():
    print(f"{names[mode]}: step min {min(v):.2f} max {max(v):.2f} mean {sum(v) / len(v):.2f} us")
