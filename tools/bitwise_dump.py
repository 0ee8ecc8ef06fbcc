#!/usr/bin/env python3
"""Development tool (not shipped, not a test): run a few graphed update epochs
and the rollout's policy pass at H (argv[2], default 256) with the library
SATRL_LIB_PATH selects, and save P, M, V, the rollout's actions / log-probs
and the values to argv[1] (.npz) -- two builds that must compute the same
bits (a scheduling-only change) are then compared file to file."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-rl-satellite_amd"))
from satrl.ppo import PPOLearner, policy_act, policy_value  # noqa: E402
from satrl.trainer import args_param  # noqa: E402

H = int(sys.argv[2]) if len(sys.argv) > 2 else 256
SCALE = float(os.environ.get("OBS_SCALE", "1"))   # 1e5: raw-metre magnitudes (as tools/span_time.py)
out = {}
for mb in (4096, 512, 777):
    torch.manual_seed(1)
    B = 8 * 4096
    a = args_param(hidden_width=H, mini_batch_size=mb, batch_size=B, chkpt_dir="/tmp", K_epochs=2)
    L = PPOLearner(a, "pursuer", graph_group=4)
    g = torch.Generator(device="cuda").manual_seed(2)
    src = torch.randn((B, 32), device="cuda", generator=g)
    src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
    src[:, 0:18] *= SCALE
    L.update_packed(src, 0.0, generator=g)
    torch.cuda.synchronize()
    for k in ("P", "M", "V", "G"):
        out[f"{mb}_{k}"] = getattr(L, k).cpu().numpy()
    obs = torch.randn((16384, 18), device="cuda", generator=g) * SCALE
    act = [torch.empty((16384, 3), device="cuda") for _ in range(4)]
    policy_act(H, obs, L.P, L.P, 1.6, 7, 0, 3, *act)
    v = torch.empty(16384, device="cuda")
    policy_value(H, obs, L.P, v)
    torch.cuda.synchronize()
    out[f"{mb}_act"] = torch.stack(act).cpu().numpy()
    out[f"{mb}_v"] = v.cpu().numpy()
np.savez(sys.argv[1], **out)
print("saved", sys.argv[1], os.environ.get("SATRL_LIB_PATH", "product"))
