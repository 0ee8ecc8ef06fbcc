"""Running observation normalisation and reward scaling of the vectorised
engine (the reference's "Trick 2" and "Trick 4": normalization.py:4-63,
which CPPO_main.py imports and never constructs).

* ``RunningMoments`` -- count, mean and M2 in host f64, fed whole batches by
  Chan's merge from shifted sums (sum of x - pivot, sum of its square): the
  form the kernels accumulate per 32-env slot.
* ``slot_total`` -- the slots of every rank placed into one zero array of the
  global slot count, summed over ranks (adding zeros is exact) and reduced
  over slots on that same-shaped array, so the total has the same bits for
  any sharding at multiples of 32 envs.
* ``obs_normalize`` / ``return_scan`` -- the two HIP kernels
  (include/satrl_rollout.h); VecTrainer reaches them through these two
  functions only.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import dist as _dist
from ._lib import OBS_DIM, check, ptr, stream_ptr

SLOT = 32            # envs per accumulator slot
EPS = 1e-8           # normalization.py:41 and :59


def num_slots(n: int) -> int:
    return (int(n) + SLOT - 1) // SLOT


class RunningMoments:
    """Count, mean and M2 (sum of squared deviations) of a stream, host f64."""

    def __init__(self, shape=()):
        self.shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        self.n = 0.0
        self.mean = np.zeros(self.shape, dtype=np.float64)
        self.M2 = np.zeros(self.shape, dtype=np.float64)

    def merge_shifted(self, n_b, sum_d, sum_d2, pivot):
        """Chan's merge with a batch of n_b samples given as sum_d = sum(x -
        pivot) and sum_d2 = sum((x - pivot)^2): the batch mean is pivot +
        sum_d / n_b and its M2 is sum_d2 - sum_d^2 / n_b."""
        n_b = float(n_b)
        if n_b <= 0:
            return self
        sum_d = np.asarray(sum_d, dtype=np.float64).reshape(self.shape)
        sum_d2 = np.asarray(sum_d2, dtype=np.float64).reshape(self.shape)
        pivot = np.broadcast_to(np.asarray(pivot, dtype=np.float64), self.shape)
        shift = sum_d / n_b                                  # batch mean - pivot
        M2_b = np.maximum(sum_d2 - sum_d * shift, 0.0)
        if self.n == 0:
            self.mean = pivot + shift
            self.M2 = M2_b
        else:
            tot = self.n + n_b
            delta = (pivot - self.mean) + shift              # batch mean - mean (pivot is near the mean)
            self.mean = self.mean + delta * (n_b / tot)
            self.M2 = self.M2 + M2_b + delta * delta * (self.n * n_b / tot)
        self.n += n_b
        return self

    def std(self):
        """sqrt(M2 / n): the population form of normalization.py:29."""
        if self.n == 0:
            return np.ones(self.shape, dtype=np.float64)
        return np.sqrt(self.M2 / self.n)

    def device_stats(self):
        """f32 [2][D]: the mean row and the inv_std = 1 / (std + 1e-8) row
        (the identity, mean 0 and inv_std 1, before the first batch)."""
        if self.n == 0:
            return np.stack([np.zeros(self.shape, np.float32), np.ones(self.shape, np.float32)])
        return np.stack([self.mean.astype(np.float32), (1.0 / (self.std() + EPS)).astype(np.float32)])

    def state_dict(self):
        return {"n": np.array(self.n, dtype=np.float64), "mean": np.array(self.mean, dtype=np.float64),
                "M2": np.array(self.M2, dtype=np.float64)}

    def load_state_dict(self, d):
        mean = np.array(d["mean"], dtype=np.float64)
        if mean.shape != self.shape:
            raise ValueError(f"moments of shape {mean.shape} loaded into shape {self.shape}")
        self.n = float(np.asarray(d["n"]))
        self.mean = mean
        self.M2 = np.array(d["M2"], dtype=np.float64).reshape(self.shape)
        return self


def slot_total(acc, pg, first_slot, global_slots):
    """Total over all ranks' slots of acc f64 [k, ...] (this rank's slots
    first_slot .. first_slot + k of global_slots), as a host f64 array.  The
    same bits on every rank and for every world size."""
    k = acc.shape[0]
    if first_slot < 0 or first_slot + k > global_slots:
        raise ValueError(f"slots {first_slot}..{first_slot + k} outside the {global_slots} global slots")
    full = torch.zeros((int(global_slots),) + tuple(acc.shape[1:]), dtype=torch.float64, device=acc.device)
    full[first_slot:first_slot + k] = acc
    full = _dist.sum_(full, pg)
    return np.add.reduce(full.cpu().numpy(), axis=0)         # slot after slot, in slot order


def obs_normalize(raw, stats, clip, out, pivot=None, acc=None):
    """out = clamp((raw - mean) * inv_std, +-clip) on satrl_obs_normalize;
    with acc (f64 [ceil(N/32), 2, 18]) the slots' sums of raw - pivot and of
    its square are added to it."""
    N = raw.shape[0]
    _lib.require_cuda(raw, torch.float32, (N, OBS_DIM), "raw")
    _lib.require_cuda(out, torch.float32, (N, OBS_DIM), "out")
    _lib.require_cuda(stats, torch.float32, (2, OBS_DIM), "stats")
    if acc is not None:
        _lib.require_cuda(acc, torch.float64, (num_slots(N), 2, OBS_DIM), "acc")
        _lib.require_cuda(pivot, torch.float32, (OBS_DIM,), "pivot")
    check(_lib.lib().satrl_obs_normalize(N, ptr(raw), ptr(stats), float(clip), ptr(out),
                                         ptr(pivot) if acc is not None else None, ptr(acc), stream_ptr()),
          "satrl_obs_normalize")
    return out


def return_scan(rew, done, gamma, carry, acc):
    """Forward scan R = gamma * R + r over rew f32 [T, N] (R = 0 after a done
    step) on satrl_return_scan: carry f64 [N] continues across calls, acc f64
    [ceil(N/32), 2] takes the slots' sums of R and R^2."""
    T, N = rew.shape
    _lib.require_cuda(rew, torch.float32, (T, N), "rew")
    _lib.require_cuda(done, torch.uint8, (T, N), "done")
    _lib.require_cuda(carry, torch.float64, (N,), "carry")
    _lib.require_cuda(acc, torch.float64, (num_slots(N), 2), "acc")
    check(_lib.lib().satrl_return_scan(T, N, ptr(rew), ptr(done), float(gamma), ptr(carry), ptr(acc), stream_ptr()),
          "satrl_return_scan")
    return carry, acc
