"""The reference of the update diagnostics (satrl_ppo_diagnostics,
UpdateDiagnostics): the ten sums and the derived fields in numpy f64, from the
per-row ratio, log-prob and value of torch_reference.reference_full and the
packed rows.  dtype=torch.float32 gives the f32 measuring stick: the same
forward in torch's f32, the sums and fields still in f64."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from torch_reference import reference_full

SLOTS = ["rows", "surr", "kl", "log_ratio", "clipped", "ratio_max", "verr2", "verr", "vt", "vt2"]
ENT_CONST = 0.5 + 0.5 * math.log(2 * math.pi)           # entropy of a unit normal
FIELDS = ["rows", "policy_loss", "entropy", "actor_loss", "value_loss", "approx_kl", "mean_log_ratio",
          "clip_fraction", "ratio_max", "explained_variance_after"]


def _fsum(x):
    return math.fsum(np.asarray(x, dtype=np.float64).reshape(-1).tolist())


def sums_from_rows(ratio, d, v, adv, vt, epsilon, f32_products=False):
    """The ten sums by their slot definitions from per-row arrays.  The sums
    are exactly rounded (math.fsum).  f32_products: ratio, d, v, adv, vt are
    f32 and the products ratio * adv, clamp(ratio) * adv and the clip edges
    1 -+ epsilon are formed in f32 as the kernel's loss-head expressions form
    them (everything after that in f64); otherwise all in f64."""
    if f32_products:
        f = np.float32
        ratio, d, v, adv, vt = (np.asarray(x, dtype=f) for x in (ratio, d, v, adv, vt))
        lo, hi = f(1.0) - f(epsilon), f(1.0) + f(epsilon)
        s1 = (ratio * adv).astype(f)
        s2 = (np.minimum(np.maximum(ratio, lo), hi).astype(f) * adv).astype(f)
    else:
        ratio, d, v, adv, vt = (np.asarray(x, dtype=np.float64) for x in (ratio, d, v, adv, vt))
        lo, hi = 1.0 - epsilon, 1.0 + epsilon
        s1 = ratio * adv
        s2 = np.clip(ratio, lo, hi) * adv
    clipped = (ratio < lo) | (ratio > hi)
    r64, d64, v64, vt64 = (x.astype(np.float64) for x in (ratio, d, v, vt))
    out = np.zeros(len(SLOTS))
    out[0] = float(len(r64))
    out[1] = _fsum(np.minimum(s1.astype(np.float64), s2.astype(np.float64)))
    out[2] = _fsum((r64 - 1.0) - d64)
    out[3] = _fsum(d64)
    out[4] = float(clipped.sum())
    out[5] = float(r64.max())
    out[6] = _fsum((v64 - vt64) ** 2)
    out[7] = _fsum(vt64 - v64)
    out[8] = _fsum(vt64)
    out[9] = _fsum(vt64 ** 2)
    return out


def fields_from_sums(sums, log_std, entropy_coef):
    """The derived fields (a dict keyed by FIELDS) from the ten sums."""
    s = dict(zip(SLOTS, (float(x) for x in sums)))
    n = s["rows"]
    entropy = _fsum(np.asarray(log_std, dtype=np.float64)) + 3 * ENT_CONST
    var_vt = s["vt2"] / n - (s["vt"] / n) ** 2
    var_e = s["verr2"] / n - (s["verr"] / n) ** 2
    return {"rows": int(n), "policy_loss": -s["surr"] / n, "entropy": entropy,
            "actor_loss": -s["surr"] / n - entropy_coef * entropy, "value_loss": s["verr2"] / n,
            "approx_kl": s["kl"] / n, "mean_log_ratio": s["log_ratio"] / n, "clip_fraction": s["clipped"] / n,
            "ratio_max": s["ratio_max"],
            "explained_variance_after": 1.0 - var_e / var_vt if var_vt > 0 else float("nan")}


def reference(actor, critic, rows, epsilon=0.1, entropy_coef=0.01, dtype=torch.float64):
    """ratio, d (log ratio), v per row of the packed `rows` [n][32] in `dtype`
    (torch_reference.reference_full's forward), and from them in f64: sums
    [10], fields {name: value}."""
    ref = reference_full(actor, critic, rows, epsilon=epsilon, entropy_coef=entropy_coef, dtype=dtype)
    r = rows.detach().to("cpu", dtype)
    d = ref.logp.sum(1) - r[:, 21:24].sum(1)
    out = SimpleNamespace(ratio=ref.ratio, d=d, v=ref.v)
    out.sums = sums_from_rows(ref.ratio.double().numpy(), d.double().numpy(), ref.v.double().numpy(),
                              r[:, 24].double().numpy(), r[:, 25].double().numpy(), epsilon)
    out.fields = fields_from_sums(out.sums, actor.log_std.detach().double().cpu().numpy().reshape(-1), entropy_coef)
    return out
