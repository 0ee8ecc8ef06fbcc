"""Opponent pool of the self-play trainer: a ring of K stored flat parameter
sets of one agent, and which of them each 32-env block plays in an iteration.

Storage is one f32 tensor [K, stride] on the trainer's device (stride: the
flat layout's total rounded up to 64 floats), handed as it is to
satrl_policy_act_pool, which reads it at every launch: ``add`` copies in
place and stream-ordered, so captured rollout graphs follow it with no
recapture.  ``assign`` is the host rule of satrl_opponent_assign: a block's
member depends on (seed, iteration, global block, filled, latest_prob) alone,
never on the sharding.  A member of -1 is the live opponent.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check

BLOCK = 32          # envs per block: the rows of one policy workgroup


def pool_stride(H):
    """Floats between two slots: the layout total rounded up to 64."""
    from .ppo import ppo_layout
    total = ppo_layout(H)["total"]
    return (total + 63) // 64 * 64


def opponent_assign(seed, iteration, first_block, n_blocks, filled, latest_prob):
    """satrl_opponent_assign -> host int32 array [n_blocks]."""
    out = np.empty(max(int(n_blocks), 0), dtype=np.int32)
    check(_lib.lib().satrl_opponent_assign(int(seed) & (2**64 - 1), int(iteration) & (2**64 - 1), int(first_block),
                                           int(n_blocks), int(filled), float(latest_prob),
                                           out.ctypes.data_as(C.c_void_p)), "satrl_opponent_assign")
    return out


def league_assign(seed, iteration, first_block, n_blocks, K, filled, n_laws, latest_prob, law_prob, weights=None):
    """satrl_league_assign -> host int32 array [n_blocks]: -1 the live
    opponent, k < K a stored slot, K + j law j.  weights: None (a uniform
    stored pick, satrl_opponent_assign's) or f64 [filled]."""
    out = np.empty(max(int(n_blocks), 0), dtype=np.int32)
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (int(filled),):
            raise ValueError(f"weights holds one f64 per filled slot ({filled}), got {w.shape}")
    check(_lib.lib().satrl_league_assign(int(seed) & (2**64 - 1), int(iteration) & (2**64 - 1), int(first_block),
                                         int(n_blocks), int(K), int(filled), int(n_laws), float(latest_prob),
                                         float(law_prob), None if w is None else w.ctypes.data_as(C.c_void_p),
                                         out.ctypes.data_as(C.c_void_p)), "satrl_league_assign")
    return out


def pfsp_weights(episodes, wins, power=2):
    """Prioritised fictitious self-play weights of stored opponents, f64: with
    the learner's smoothed win rate p_k = (wins_k + 1) / (episodes_k + 2)
    against slot k, weight_k = (1 - p_k) ** power by repeated multiplication
    (play more often what you lose to).  An unplayed slot gets (1/2) ** power."""
    if isinstance(power, bool) or int(power) != power or int(power) <= 0:
        raise ValueError(f"pfsp_power is a positive int, got {power!r}")
    e = np.asarray(episodes, dtype=np.float64)
    w = np.asarray(wins, dtype=np.float64)
    if e.shape != w.shape or e.ndim != 1 or (w < 0).any() or (w > e).any():
        raise ValueError("episodes and wins are equal-length counts with 0 <= wins <= episodes")
    base = 1.0 - (w + 1.0) / (e + 2.0)
    out = base.copy()
    for _ in range(int(power) - 1):
        out = out * base
    return out


def league_tally(rew, done, capture_reward, tally):
    """satrl_league_tally: tally i64 [ceil(N / 32), 2] += per 32-env block the
    done steps of rew / done [T, N] and those whose reward is capture_reward."""
    T, N = rew.shape
    _lib.require_cuda(rew, torch.float32, (T, N), "rew")
    if done.dtype == torch.bool:
        done = done.view(torch.uint8)
    _lib.require_cuda(done, torch.uint8, (T, N), "done")
    _lib.require_cuda(tally, torch.int64, ((N + BLOCK - 1) // BLOCK, 2), "tally")
    check(_lib.lib().satrl_league_tally(T, N, _lib.ptr(rew), _lib.ptr(done), float(capture_reward), _lib.ptr(tally),
                                        _lib.stream_ptr()), "satrl_league_tally")
    return tally


class OpponentPool:
    """K ring slots of flat parameter sets of width H on `device`."""

    def __init__(self, K, H, device, seed=0):
        self.K, self.H = int(K), int(H)
        if self.K <= 0:
            raise ValueError(f"an opponent pool holds at least one slot, got K={K}")
        self.device = torch.device(device)
        self.seed = int(seed)
        from .ppo import ppo_layout
        self.total = ppo_layout(self.H)["total"]
        self.stride = pool_stride(self.H)
        self.storage = torch.zeros((self.K, self.stride), dtype=torch.float32, device=self.device)
        self.metas = [None] * self.K
        self.cursor = 0                                  # the slot the next add() writes
        self.added = 0                                   # add() calls so far

    @property
    def filled(self):
        return min(self.added, self.K)

    def add(self, P, meta=None):
        """Copy the flat parameter buffer P into the next ring slot (the oldest
        once full), in place and stream-ordered; returns the slot."""
        P = P.detach().reshape(-1)
        if P.dtype != torch.float32 or P.numel() != self.total:
            raise ValueError(f"a flat f32 parameter buffer of {self.total} elements is expected, got "
                             f"{P.dtype} [{P.numel()}]")
        k = self.cursor
        self.storage[k, :self.total].copy_(P)
        self.metas[k] = dict(meta) if meta is not None else {}
        self.cursor = (k + 1) % self.K
        self.added += 1
        return k

    def slot(self, k):
        """A view of slot k's parameters [total]; IndexError if it is not filled."""
        k = int(k)
        if not 0 <= k < self.filled:
            raise IndexError(f"opponent slot {k} is not filled ({self.filled} of {self.K} are)")
        return self.storage[k, :self.total]

    def assign(self, iteration, first_block, n_blocks, latest_prob):
        """This iteration's member of global blocks first_block .. + n_blocks
        (host int32; -1: the live opponent)."""
        return opponent_assign(self.seed, iteration, first_block, n_blocks, self.filled, latest_prob)

    def state(self):
        return {"K": self.K, "H": self.H, "storage": self.storage.detach().cpu().clone(),
                "metas": [None if m is None else dict(m) for m in self.metas], "cursor": self.cursor,
                "added": self.added, "seed": self.seed}

    def load_state(self, d):
        if int(d["K"]) != self.K or int(d["H"]) != self.H:
            raise ValueError(f"a pool state of K={d['K']}, H={d['H']} for a pool of K={self.K}, H={self.H}")
        st = d["storage"]
        if tuple(st.shape) != tuple(self.storage.shape) or st.dtype != torch.float32:
            raise ValueError(f"pool storage of shape {tuple(st.shape)} for {tuple(self.storage.shape)}")
        self.storage.copy_(st)
        self.metas = [None if m is None else dict(m) for m in d["metas"]]
        self.cursor = int(d["cursor"])
        self.added = int(d["added"])
        self.seed = int(d.get("seed", self.seed))
