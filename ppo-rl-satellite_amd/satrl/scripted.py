"""Scripted opponents of the vectorised engine: linear guidance laws.

A ``ScriptedLaw`` is ``a = clamp(b + G s, +-max_action)`` over the 18 RAW
observation features ``s`` of an env (metres, m/s; the first six are the
relative position and velocity, pursuer minus evader).  It owns one 464-byte
device block (``satrl_scripted_law``, include/satrl_ppo.h) that the kernels
read at every launch: ``update`` rewrites it in place and stream-ordered, so
captured rollout graphs follow a gain schedule or a new horizon with no
recapture.

The builders take the env's own state transition matrix (``satrl.env.stm``,
the reference's CW matrix as the step kernel applies it), so the laws are
exact for the dynamics the env integrates:

* ``coast()``: no thrust; ``constant(a)``: the same thrust every step.
* ``intercept(horizon_steps)``: with Phi = stm(dt) ** horizon_steps, blocks
  Phi_rr = Phi[:3, :3], Phi_rv = Phi[:3, 3:] and A = Phi_rv^-1 Phi_rr, the
  commanded delta-v ``-(A r + v)`` makes the relative velocity the one that
  nulls the relative position after the horizon if nobody thrusts again;
  re-evaluated every step it is a receding horizon.  A pursuer's law.
* ``evade(horizon_steps, gain)``: ``gain`` times the same expression for the
  evader, whose delta-v enters the relative velocity with a minus sign: it
  pushes the relative velocity away from the collision course.

Phi_rv is singular at multiples of the reference orbit's period (861.64
steps of 100 s; its z block at half periods): a horizon whose
cond(Phi_rv) > 1e6 is refused, and so is the whole number of steps nearest
to a multiple of half the period (431, 862, ...), where cond only reaches
about 3e4 because the singular time falls between two steps.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

OBS_DIM, ACT_DIM = 18, 3
LAW_DOUBLES = ACT_DIM * OBS_DIM + ACT_DIM + 1          # satrl_scripted_law: G, b, max_action
LAW_BYTES = 8 * LAW_DOUBLES
MAX_COND = 1e6
AGENTS = ("pursuer", "evader")


def _checked(G, b, max_action):
    G = np.array(G, dtype=np.float64)
    if G.shape != (ACT_DIM, OBS_DIM):
        raise ValueError(f"G must be [{ACT_DIM}, {OBS_DIM}], got {G.shape}")
    b = np.zeros(ACT_DIM, dtype=np.float64) if b is None else np.array(b, dtype=np.float64)
    if b.shape != (ACT_DIM,):
        raise ValueError(f"b must be [{ACT_DIM}], got {b.shape}")
    if not (np.isfinite(G).all() and np.isfinite(b).all()):
        raise ValueError("G and b must be finite")
    max_action = float(max_action)
    if not (max_action > 0.0 and np.isfinite(max_action)):            # (NaN fails the comparison)
        raise ValueError(f"max_action must be positive and finite, got {max_action}")
    return G, b, max_action


class ScriptedLaw:
    """``a = clamp(b + G s, +-max_action)``; G [3, 18] and b [3] are f64."""

    def __init__(self, G, b=None, max_action=1.6):
        self.G, self.b, self.max_action = _checked(G, b, max_action)
        self._block = None                               # f64 [58] on the device, allocated at its first use
        self._table = None                               # the LawTable whose row the block is a view of, if any

    # -- the device block -------------------------------------------------------------------
    def packed(self):
        """The 58 doubles of satrl_scripted_law (host)."""
        return np.concatenate([self.G.reshape(-1), self.b, [self.max_action]])

    def block(self, device=None):
        """The law's device block (f64 [58]); the first call places it on
        `device` (default: the current one), every later one returns the same
        tensor."""
        if self._block is None:
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            self._block = torch.from_numpy(self.packed()).to(dev)
        elif device is not None and torch.device(device) != self._block.device:
            raise ValueError(f"this law's block lives on {self._block.device}, not on {device}")
        return self._block

    def update(self, G=None, b=None, max_action=None):
        """New values, validated as in the constructor; the device block is
        rewritten in place and stream-ordered."""
        G, b, m = _checked(self.G if G is None else G, self.b if b is None else b,
                           self.max_action if max_action is None else max_action)
        self.G, self.b, self.max_action = G, b, m
        if self._block is not None:
            self._block.copy_(torch.from_numpy(self.packed()))
        return self

    # -- plain state ------------------------------------------------------------------------
    def state(self):
        return {"G": self.G.copy(), "b": self.b.copy(), "max_action": np.float64(self.max_action)}

    @classmethod
    def from_state(cls, d):
        return cls(np.asarray(d["G"]), np.asarray(d["b"]), float(np.asarray(d["max_action"]).item()))

    def numpy(self, obs):
        """The law on host rows obs [n, 18] in the kernels' arithmetic (f32 [n, 3])."""
        return scripted_act_host(np.ascontiguousarray(obs, dtype=np.float32), self)

    def __repr__(self):
        return f"ScriptedLaw(|G|max={np.abs(self.G).max():.3g}, b={self.b.tolist()}, max_action={self.max_action})"


# -- builders -------------------------------------------------------------------------------
def _collision_matrix(horizon_steps, dt):
    """A = Phi_rv^-1 Phi_rr of Phi = stm(dt) ** horizon_steps."""
    from .env import stm
    k = int(horizon_steps)
    if k != horizon_steps or k <= 0:
        raise ValueError(f"horizon_steps is a positive number of env steps, got {horizon_steps!r}")
    phi1 = stm(float(dt))
    phi = np.linalg.matrix_power(phi1, k)
    prr, prv = phi[:3, :3], phi[:3, 3:]
    cond = np.linalg.cond(prv)
    if not cond <= MAX_COND:                                             # (NaN / inf are refused too)
        raise ValueError(f"a horizon of {k} steps of {dt} s: cond(Phi_rv) = {cond:.3g} > {MAX_COND:g}")
    # Phi_rv(t) is singular AT a multiple of half the period, which a whole number of steps never hits
    # (cond is 3.1e4 at 431 steps, 2.8e4 at 862): the horizon nearest to one is refused as well.  The
    # out-of-plane block of the matrix is [[cos wt, sin wt / w], [-w sin wt, cos wt]], which gives w dt
    wt = np.arctan2(np.sqrt(max(-phi1[5, 2] * phi1[2, 5], 0.0)), phi1[2, 2])      # the orbit's angle per step
    half = np.pi / wt if wt > 0 else np.inf                                      # half a period, in steps
    n = round(k / half)
    if n >= 1 and abs(k - n * half) <= 0.5:
        raise ValueError(f"a horizon of {k} steps of {dt} s is the nearest to {n} half period(s) of the orbit "
                         f"({n * half:.2f} steps), where Phi_rv is singular: cond(Phi_rv) = {cond:.3g}")
    return np.linalg.solve(prv, prr)


def coast(max_action=1.6):
    return ScriptedLaw(np.zeros((ACT_DIM, OBS_DIM)), None, max_action)


def constant(a, max_action=1.6):
    return ScriptedLaw(np.zeros((ACT_DIM, OBS_DIM)), a, max_action)


def intercept_matrix(horizon_steps=10, dt=100.0):
    """G [3, 18] of intercept(): G[:, 0:6] = -[A | I], the rest 0."""
    G = np.zeros((ACT_DIM, OBS_DIM))
    G[:, 0:3] = -_collision_matrix(horizon_steps, dt)
    G[:, 3:6] = -np.eye(3)
    return G


def intercept(horizon_steps=10, dt=100.0, max_action=1.6):
    return ScriptedLaw(intercept_matrix(horizon_steps, dt), None, max_action)


def evade_matrix(horizon_steps=10, gain=0.5, dt=100.0):
    return float(gain) * intercept_matrix(horizon_steps, dt)


def evade(horizon_steps=10, gain=0.5, dt=100.0, max_action=1.6):
    return ScriptedLaw(evade_matrix(horizon_steps, gain, dt), None, max_action)


BUILDERS = {"coast": coast, "constant": constant, "intercept": intercept, "evade": evade}


def as_law(spec):
    """A ScriptedLaw, or the name of a builder that needs no argument."""
    if isinstance(spec, ScriptedLaw):
        return spec
    if isinstance(spec, str):
        if spec not in BUILDERS or spec == "constant":
            raise ValueError(f"a scripted opponent is a ScriptedLaw or one of 'coast', 'intercept', 'evade', "
                             f"got {spec!r}")
        return BUILDERS[spec]()
    raise ValueError(f"a scripted opponent is a ScriptedLaw or a builder's name, got {type(spec).__name__}")


def parse_opponents(spec):
    """args_param(scripted_opponent=...): None, a mapping {"evader": law,
    "pursuer": law} with either key optional, or a builder's name / a
    ScriptedLaw as shorthand for {"evader": ...}.  Returns {agent: ScriptedLaw}."""
    if spec is None:
        return {}
    if isinstance(spec, (str, ScriptedLaw)):
        return {"evader": as_law(spec)}
    try:
        items = dict(spec).items()
    except (TypeError, ValueError):
        raise ValueError(f"scripted_opponent is None, a mapping over {AGENTS}, a builder's name or a ScriptedLaw, "
                         f"got {type(spec).__name__}") from None
    out = {}
    for k, v in items:
        if k not in AGENTS:
            raise ValueError(f"scripted_opponent names agents {AGENTS}, got {k!r}")
        if v is not None:
            out[k] = as_law(v)
    return out


# -- league play: several laws in one device table --------------------------------------------
LEAGUE_MAX_LAWS = 8                                      # SATRL_LEAGUE_MAX_LAWS (include/satrl_ppo.h)
LEAGUE_WEIGHTINGS = ("uniform", "pfsp")


class LawTable:
    """The law table of satrl_policy_act_league: one f64 tensor [capacity, 58]
    on `device` that never moves, a satrl_scripted_law per row.  ``set``
    copies each law's 58 doubles into its row and makes the law's device block
    a view of that row, so ``ScriptedLaw.update`` on a league law keeps
    writing in place and stream-ordered, and captured graphs follow it.  Rows
    past the set laws are zero (no thrust) and never assigned.  A law lives in
    one table at a time, and a law that already owns a device block (one that
    a kernel or a captured graph elsewhere may read) is refused: hand the
    table a copy.  A ``set`` may move a law to another row or detach it (its
    next use then allocates a block of its own), so whoever captured a graph
    on a league law's block outside the table's own launch drops that graph
    after a ``set`` (VecTrainer.set_league_laws does, for its evaluators)."""

    def __init__(self, device, capacity=LEAGUE_MAX_LAWS):
        self.capacity = int(capacity)
        if not 1 <= self.capacity <= LEAGUE_MAX_LAWS:
            raise ValueError(f"a law table holds 1 .. {LEAGUE_MAX_LAWS} laws, got capacity={capacity}")
        self.device = torch.device(device)
        self.storage = torch.zeros((self.capacity, LAW_DOUBLES), dtype=torch.float64, device=self.device)
        self.laws = []

    def __len__(self):
        return len(self.laws)

    def set(self, laws):
        laws = [as_law(x) for x in (laws or [])]
        if len(laws) > self.capacity:
            raise ValueError(f"at most {self.capacity} league laws per agent, got {len(laws)}")
        if len({id(x) for x in laws}) != len(laws):
            raise ValueError("the same ScriptedLaw object twice in one law table: pass a copy")
        for law in laws:
            if law._table is not None and law._table is not self:
                raise ValueError("this ScriptedLaw is bound to another law table: pass a copy "
                                 "(ScriptedLaw.from_state(law.state()))")
            if law._table is None and law._block is not None:
                raise ValueError("this ScriptedLaw already owns a device block that launches elsewhere may read: "
                                 "pass a copy (ScriptedLaw.from_state(law.state()))")
        for old in self.laws:                            # a detached law allocates a block of its own at its next use
            old._block, old._table = None, None
        self.storage.zero_()
        for j, law in enumerate(laws):
            self.storage[j].copy_(torch.from_numpy(law.packed()))
            law._block, law._table = self.storage[j], self
        self.laws = laws
        return self


def parse_league(spec):
    """args_param(league_laws=...): None, or a mapping {"evader": [law, ...],
    "pursuer": [...]} whose entries are a ScriptedLaw or a builder's name, at
    most LEAGUE_MAX_LAWS per agent.  Returns {agent: [ScriptedLaw]} without
    the agents that have none."""
    if spec is None:
        return {}
    try:
        items = dict(spec).items()
    except (TypeError, ValueError):
        raise ValueError(f"league_laws is None or a mapping over {AGENTS} of lists of laws, "
                         f"got {type(spec).__name__}") from None
    out = {}
    for k, v in items:
        if k not in AGENTS:
            raise ValueError(f"league_laws names agents {AGENTS}, got {k!r}")
        if v is None:
            continue
        if isinstance(v, (str, ScriptedLaw)):
            v = [v]
        laws = [as_law(x) for x in v]
        if len(laws) > LEAGUE_MAX_LAWS:
            raise ValueError(f"at most {LEAGUE_MAX_LAWS} league laws per agent, got {len(laws)} for {k!r}")
        if laws:
            out[k] = laws
    return out


# -- kernels ----------------------------------------------------------------------------------
def _host_law(law):
    a = np.ascontiguousarray(law.packed() if isinstance(law, ScriptedLaw) else law, dtype=np.float64)
    if a.shape != (LAW_DOUBLES,):
        raise ValueError(f"a law block is {LAW_DOUBLES} doubles, got {a.shape}")
    return a


def scripted_act_host(obs, law):
    """satrl_scripted_act_host: host rows obs f32 [n, 18] -> f32 [n, 3]."""
    obs = np.ascontiguousarray(obs)
    if obs.dtype != np.float32 or obs.ndim != 2 or obs.shape[1] != OBS_DIM:
        raise ValueError(f"obs must be f32 [n, {OBS_DIM}], got {obs.dtype} {obs.shape}")
    blk = _host_law(law)
    out = np.empty((obs.shape[0], ACT_DIM), dtype=np.float32)
    rc = _lib.lib().satrl_scripted_act_host(obs.shape[0], obs.ctypes.data_as(C.c_void_p),
                                            blk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise _lib.NativeError(f"satrl_scripted_act_host failed ({rc})")
    return out


def _block_of(law, device):
    blk = law.block(device) if isinstance(law, ScriptedLaw) else law
    _lib.require_cuda(blk, torch.float64, (LAW_DOUBLES,), "law")
    return blk


def scripted_act(obs, law, act=None):
    """satrl_scripted_act: the law over device rows obs f32 [n, 18]."""
    N = obs.shape[0]
    _lib.require_cuda(obs, torch.float32, (N, OBS_DIM), "obs")
    act = torch.empty((N, ACT_DIM), dtype=torch.float32, device=obs.device) if act is None else act
    _lib.require_cuda(act, torch.float32, (N, ACT_DIM), "act")
    check(_lib.lib().satrl_scripted_act(N, ptr(obs), ptr(_block_of(law, obs.device)), ptr(act), stream_ptr()),
          "satrl_scripted_act")
    return act
