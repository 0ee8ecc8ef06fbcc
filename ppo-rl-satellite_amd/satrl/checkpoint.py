"""Whole-state checkpoints of ``VecTrainer``.

A checkpoint is one directory: ``rank{r}.npz`` per writing rank (np.savez of
the rank's ``VecTrainer.state_dict()``, flattened to "a/b/c" keys; numeric
arrays only, read with allow_pickle=False) and ``meta.json`` (format version,
world size, global env count, every rank's (env_offset, N) and the
configuration fingerprint), which is written last: a directory without it is
an incomplete checkpoint.  The directory is built as a temporary sibling and
renamed into place, so the previous checkpoint stays until the new one is
complete.  Under a process group every rank writes into the same directory
(a file system all ranks see).

Per-env arrays (PER_ENV) carry their global env range, so a reader whose
(env_offset, N) differs from the writer's takes its slice from whichever
rank files overlap it; everything else is global and comes from rank 0's
file.  No pickle, no torch.save.
"""
from __future__ import annotations

import json
import os
import shutil

import numpy as np

from . import dist as _dist

FORMAT_VERSION = 1
BLOCK = 32                       # envs per normalisation slot / opponent block (norm.SLOT, pool.BLOCK)
JSON_TAG = "@json"               # a flattened key that holds a JSON document as uint8 bytes
META = "meta.json"

# flattened key of every per-env array -> its env axis
PER_ENV = {"env/f64": 1, "env/i32": 1, "env/ep_return": 0, "env/episode_index": 0, "ret_carry": 0, "obs0": 0,
           "obs_raw": 0}

# what must be equal between the writer and the reader (horizon, K_epochs, the
# learning rates, the graph knobs and diagnostics may differ; the actuation
# noise is not here either: its spec and seed are state, "act_noise", which the
# reader takes over from rank 0's file whatever its own sharding -- the draw is
# keyed by the global env id, the episode index and the step count, all restored)
FINGERPRINT_FIELDS = ("hidden_width", "global_envs", "seed", "reset_seed", "opponent_seed", "obs_norm",
                      "reward_scaling", "opponent_pool", "minibatch_sampler", "dp_minibatch", "mini_batch_size",
                      "max_episode_steps", "d_capture", "reset_box", "max_train_steps")


class IncompleteCheckpoint(FileNotFoundError):
    pass


# -- nested dict <-> flat numeric arrays ------------------------------------------------
def _json_default(o):
    if isinstance(o, np.generic):
        return o.item()
    if isinstance(o, np.ndarray):
        return o.tolist()
    raise TypeError(f"{type(o).__name__} is not a plain record")


def encode_json(obj) -> np.ndarray:
    """A plain record (lists, dicts, str, numbers, None) as the uint8 bytes of
    its JSON text; floats round-trip exactly (repr), NaN and inf included."""
    return np.frombuffer(json.dumps(obj, default=_json_default).encode("utf-8"), dtype=np.uint8).copy()


def decode_json(a):
    return json.loads(np.asarray(a, dtype=np.uint8).tobytes().decode("utf-8"))


def flatten(d, prefix=""):
    """Nested dict -> {"a/b": numeric ndarray}.  Arrays and numpy / python
    numbers stay arrays (numbers become zero-dimensional); anything else
    (lists of records, strings, None, bool) is stored as JSON bytes under
    key + "@json"."""
    out = {}
    for k, v in d.items():
        k = str(k)
        if "/" in k or k.endswith(JSON_TAG):
            raise ValueError(f"state key {k!r} holds the separator")
        key = prefix + k
        if isinstance(v, dict):
            out.update(flatten(v, key + "/"))
        elif isinstance(v, (np.ndarray, np.generic)) and np.asarray(v).dtype.kind in "fiu":
            out[key] = np.ascontiguousarray(v) if np.ndim(v) else np.asarray(v)
        elif isinstance(v, (int, float)) and not isinstance(v, bool):
            out[key] = np.asarray(v, dtype=np.int64 if isinstance(v, int) else np.float64)
        else:
            out[key + JSON_TAG] = encode_json(v)
    return out


def unflatten(flat):
    """Inverse of flatten (zero-dimensional arrays stay zero-dimensional)."""
    out = {}
    for key, v in flat.items():
        parts = key.split("/")
        node = out
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        leaf = parts[-1]
        if leaf.endswith(JSON_TAG):
            node[leaf[:-len(JSON_TAG)]] = decode_json(v)
        else:
            node[leaf] = np.asarray(v)
    return out


# -- configuration fingerprint -----------------------------------------------------------
def fingerprint(trainer, global_envs=None):
    """The fields whose change would make a restored state meaningless or
    shift a random stream, as JSON values."""
    from .env import reset_box
    a = trainer.args
    box = reset_box(trainer.reset_spread)
    pool = int(getattr(a, "opponent_pool", 0))
    fp = {"hidden_width": int(a.hidden_width),
          "global_envs": int(trainer.N * _dist.world_size(trainer.pg) if global_envs is None else global_envs),
          "seed": int(trainer.seed), "reset_seed": int(trainer.reset_seed),
          "opponent_seed": int(trainer.opponent_seed) if pool > 0 else None,
          "obs_norm": bool(trainer.obs_norm), "reward_scaling": bool(trainer.reward_scaling),
          "opponent_pool": pool, "minibatch_sampler": trainer.sampler, "dp_minibatch": trainer.dp_minibatch,
          "mini_batch_size": int(a.mini_batch_size), "max_episode_steps": int(a.max_episode_steps),
          "d_capture": float(trainer.env.d_capture),
          "reset_box": None if box is None else [box[0].tolist(), box[1].tolist()],
          "max_train_steps": float(a.max_train_steps)}
    assert tuple(fp) == FINGERPRINT_FIELDS
    return fp


def check_fingerprint(saved, current):
    """ValueError naming the first field that differs, with both values."""
    current = json.loads(json.dumps(current))
    for k in FINGERPRINT_FIELDS:
        if k not in saved:
            raise ValueError(f"checkpoint fingerprint has no field {k!r}")
        if saved[k] != current[k]:
            raise ValueError(f"checkpoint was written with {k}={saved[k]!r}, this trainer has {k}={current[k]!r}")


# -- global env ranges -------------------------------------------------------------------
def check_tiling(ranges, total, whole_blocks=False):
    """ranges [(env_offset, N)] of all readers (or writers) must tile
    [0, total) exactly; with whole_blocks no boundary inside the run may split
    a 32-env block (the constructor's rule under normalisation or a pool)."""
    at = 0
    for lo, n in sorted((int(lo), int(n)) for lo, n in ranges):
        if n <= 0 or lo != at:
            raise ValueError(f"env ranges {sorted(map(tuple, ranges))} do not tile the {total} global envs")
        at = lo + n
    if at != int(total):
        raise ValueError(f"env ranges {sorted(map(tuple, ranges))} do not tile the {total} global envs")
    if whole_blocks:
        for lo, n in ranges:
            check_range(lo, n, total, True)


def check_range(lo, n, total, whole_blocks=False):
    """One reader's range [lo, lo + n) must lie inside [0, total), on block
    boundaries where whole_blocks is set."""
    lo, n, total = int(lo), int(n), int(total)
    if lo < 0 or n <= 0 or lo + n > total:
        raise ValueError(f"envs {lo}..{lo + n} lie outside the checkpoint's {total} global envs")
    if whole_blocks and (lo % BLOCK or ((lo + n) % BLOCK and lo + n != total)):
        raise ValueError(f"envs {lo}..{lo + n} split a {BLOCK}-env block (observation normalisation, reward scaling "
                         f"and the opponent pool keep state per block)")


def overlapping(shards, lo, n):
    """Indices of the writer shards [(env_offset, N)] that overlap [lo, lo + n)."""
    return [r for r, (o, m) in enumerate(shards) if o < lo + n and lo < o + m]


def gather_range(pieces, lo, n, axis=0):
    """The slice [lo, lo + n) of a per-env array along `axis` out of
    pieces [(env_offset, array)], which must cover it without gaps."""
    out, at = [], int(lo)
    for o, a in sorted(pieces, key=lambda p: p[0]):
        m = a.shape[axis]
        if o + m <= at or o >= lo + n:
            continue
        if o > at:
            break
        end = min(o + m, lo + n)
        out.append(np.take(a, np.arange(at - o, end - o), axis=axis))
        at = end
    if at != lo + n:
        raise ValueError(f"envs {at}..{lo + n} are in none of the checkpoint's shards")
    return np.ascontiguousarray(np.concatenate(out, axis=axis))


# -- files ---------------------------------------------------------------------------------
def _rank_file(path, r):
    return os.path.join(path, f"rank{int(r)}.npz")


def write_rank(path, r, flat):
    for k, v in flat.items():
        if np.asarray(v).dtype.kind not in "fiu":
            raise TypeError(f"{k}: {np.asarray(v).dtype} is not a numeric array")
    np.savez(_rank_file(path, r), **flat)


def read_rank(path, r):
    """The lazily read arrays of rank r's file (a numpy NpzFile)."""
    return np.load(_rank_file(path, r), allow_pickle=False)


def read_meta(path):
    p = os.path.join(path, META)
    if not os.path.isfile(p):
        raise IncompleteCheckpoint(f"{path}: no {META} (not a checkpoint, or one whose writing never finished)")
    with open(p) as f:
        meta = json.load(f)
    if meta.get("format_version") != FORMAT_VERSION:
        raise ValueError(f"{path}: checkpoint format {meta.get('format_version')!r}, this build reads "
                         f"{FORMAT_VERSION}")
    return meta


def _commit(tmp, path):
    """The finished temporary directory takes the checkpoint's name; a previous
    checkpoint is moved aside first and removed afterwards."""
    old = path + ".old"
    shutil.rmtree(old, ignore_errors=True)
    had = os.path.lexists(path)
    if had:
        os.replace(path, old)
    try:
        os.replace(tmp, path)
    except BaseException:
        if had:
            os.replace(old, path)
        raise
    shutil.rmtree(old, ignore_errors=True)


def write_checkpoint(path, flat, meta, pg=None):
    """Every rank's `flat` arrays and rank 0's `meta` into the directory
    `path`, atomically: rank files into a temporary sibling, a barrier,
    meta.json last, then the rename."""
    path = os.path.abspath(os.fspath(path)).rstrip(os.sep)
    tmp = path + ".tmp"
    r = _dist.rank(pg)
    if r == 0:
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(tmp)
    _dist.barrier(pg)
    write_rank(tmp, r, flat)
    _dist.barrier(pg)
    if r == 0:
        with open(os.path.join(tmp, META), "w") as f:
            json.dump(meta, f, indent=1, sort_keys=True)
        _commit(tmp, path)
    _dist.barrier(pg)
    return path


# -- trainer level -------------------------------------------------------------------------
def _whole_blocks(trainer):
    return bool(trainer.obs_norm or trainer.reward_scaling or trainer.pools is not None)


def save(trainer, path):
    """VecTrainer.save_checkpoint."""
    flat = flatten(trainer.state_dict())
    pg = trainer.pg
    shards = _dist.all_gather_object((trainer.env_offset, trainer.N), pg)
    meta = {"format_version": FORMAT_VERSION, "world_size": _dist.world_size(pg),
            "global_envs": int(sum(n for _, n in shards)), "shards": [[int(o), int(n)] for o, n in shards],
            "fingerprint": fingerprint(trainer), "iteration_count": int(trainer.iteration_count),
            "flag": int(trainer.flag)}
    check_tiling(meta["shards"], meta["global_envs"])
    return write_checkpoint(path, flat, meta, pg)


def load(trainer, path, global_envs=None):
    """VecTrainer.load_checkpoint: the state of this trainer's env range out
    of the checkpoint at `path`, whatever sharding wrote it."""
    path = os.path.abspath(os.fspath(path)).rstrip(os.sep)
    meta = read_meta(path)
    pg = trainer.pg
    W, r = _dist.world_size(pg), _dist.rank(pg)
    if pg is not None and global_envs is not None and int(global_envs) != trainer.N * W:
        raise ValueError(f"global_envs={global_envs} under a process group of {W} x {trainer.N} envs")
    check_fingerprint(meta["fingerprint"], fingerprint(trainer, global_envs))
    G = int(meta["global_envs"])
    shards = [(int(o), int(n)) for o, n in meta["shards"]]
    lo, n = trainer.env_offset, trainer.N
    if pg is not None:
        check_tiling(_dist.all_gather_object((lo, n), pg), G, _whole_blocks(trainer))
    else:
        check_range(lo, n, G, _whole_blocks(trainer) and (lo, n) != (0, G))
    same = W == int(meta["world_size"]) and r < len(shards) and shards[r] == (lo, n)
    files = {}

    def rank_file(k):
        if k not in files:
            files[k] = read_rank(path, k)
        return files[k]

    try:
        base = rank_file(r if same else 0)
        flat = {}
        for key in base.files:
            if key in PER_ENV:
                if same:
                    flat[key] = base[key]
                else:
                    flat[key] = gather_range([(shards[k][0], rank_file(k)[key]) for k in overlapping(shards, lo, n)],
                                             lo, n, PER_ENV[key])
            elif key.startswith("strata_gen/") or (not same and key in ("gen", "env/stats")):
                continue
            else:
                flat[key] = base[key]
        for s in getattr(trainer, "my_strata", []) if trainer.sampler == "stratified" else []:
            key = f"strata_gen/{s}"
            for k in range(len(shards)):
                if key in rank_file(k).files:
                    flat[key] = rank_file(k)[key]
                    break
            else:
                raise ValueError(f"{path}: no generator state of stratum {s}")
        if not same:
            # the writer's global episode statistics go to the reader of env 0, so
            # that the sum over the readers is the writer's total
            tot = np.zeros(4, dtype=np.float64)
            if lo == 0:
                for k in range(len(shards)):
                    tot = tot + rank_file(k)["env/stats"]
            flat["env/stats"] = tot
        trainer.load_state_dict(unflatten(flat))
    finally:
        for f in files.values():
            f.close()
    return meta
