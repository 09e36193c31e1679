"""Episode store: trajectories on disk in the form the device batch assembly reads.

A store is a directory:

  meta.json             format version, counts, frame shape [C, H, W, 3] (C cameras), action_dim, proprio_dim, token
                        length L, pad token id, the frame shard table and one ``labeled`` flag per episode
  episode_offsets.npy   int64 [E + 1]: episode e occupies rows [offsets[e], offsets[e + 1]) of every per-step array
  action.npy            fp32 [N, A], raw robot units
  proprio.npy           fp32 [N, P], raw robot units
  input_ids.npy         int32 [E, L]: the full model prompt of each episode (image tokens, BOS, text, newline, padding);
                        tokenisation happens before the store is written
  frames_%05d.npy       uint8 [n_i, C, H, W, 3]; read through np.load(mmap_mode="r"); a shard never splits an episode
  statistics.json       mean / std / max / min / p99 / p01 of all action and proprio rows, num_transitions and
                        num_trajectories: the layout ``env.adapter.dataset_statistics_path`` points at

The statistics are the reference's (src/data/utils/data_utils.py:161-183): over the whole store, before any filtering.
Nothing here needs TensorFlow, torch or a GPU.
"""

from __future__ import annotations

import json
import os

import numpy as np

FORMAT_VERSION = 1
DEFAULT_SHARD_BYTES = 256 << 20
FILES = ("meta.json", "episode_offsets.npy", "action.npy", "proprio.npy", "input_ids.npy", "statistics.json")


def compute_statistics(action, proprio, num_trajectories):
    """data_utils.py:161-183 on fp32 [N, A] / [N, P]: the dict that statistics.json holds"""
    def one(x):
        return {"mean": x.mean(0).tolist(), "std": x.std(0).tolist(), "max": x.max(0).tolist(),
                "min": x.min(0).tolist(), "p99": np.quantile(x, 0.99, 0).tolist(),
                "p01": np.quantile(x, 0.01, 0).tolist()}

    return {"action": one(action), "num_transitions": int(action.shape[0]), "num_trajectories": int(num_trajectories),
            "proprio": one(proprio)}


def synthetic_episode(e, length, height, width, *, cameras=1, action_dim=7, proprio_dim=7, token_len=276,
                      image_tokens=256, image_token_index=257152, vocab_size=257216, pad_token_id=0, labeled=True,
                      seed=0):
    """Episode ``e`` of a counter-generated store (tests, benchmarks): a function of (seed, e) and the sizes alone.
    Tokens as SyntheticBridgeDataset lays a prompt out: image tokens, BOS (2), text, newline, padding; an unlabelled
    episode has no text between BOS and the padding."""
    g = np.random.Generator(np.random.Philox(key=[int(seed), 0x73796E7468657469], counter=[0, 0, int(e), 0]))
    frames = g.integers(0, 256, (length, cameras, height, width, 3), dtype=np.uint8)
    action = g.uniform(-1.5, 1.5, (length, action_dim)).astype(np.float32)
    action[:, -1] = g.integers(0, 2, length)  # the gripper: 0 / 1, passed through by the normalisation
    proprio = g.uniform(-2.0, 2.0, (length, proprio_dim)).astype(np.float32)
    ids = np.full(token_len, pad_token_id, np.int32)
    ids[:image_tokens] = image_token_index
    ids[image_tokens] = 2
    if labeled:
        vmax = min(int(vocab_size), int(image_token_index))
        room = token_len - image_tokens - 1  # after BOS: text + newline
        if room < 2:
            raise ValueError("synthetic_episode: token_len leaves no room for a text token and the newline")
        n = int(g.integers(1, room))  # text tokens
        ids[image_tokens + 1: image_tokens + 1 + n] = g.integers(3, vmax, n)
        ids[image_tokens + 1 + n] = min(108, vmax - 1)
    return {"frames": frames, "action": action, "proprio": proprio, "input_ids": ids, "labeled": bool(labeled)}


class EpisodeStoreWriter:
    """``add_episode(frames, action, proprio, input_ids, labeled=True)`` per trajectory, then ``close()``, which writes
    the offsets, the statistics and meta.json.  The first episode fixes the frame shape and the dimensions; frames are
    written shard by shard as they arrive (at most ``shard_bytes`` are held, a single longer episode excepted)."""

    def __init__(self, path, pad_token_id=0, shard_bytes=DEFAULT_SHARD_BYTES):
        self.path = str(path)
        os.makedirs(self.path, exist_ok=True)
        if os.path.exists(os.path.join(self.path, "meta.json")):
            raise ValueError(f"{self.path} already holds an episode store (meta.json exists)")
        self.pad_token_id = int(pad_token_id)
        self.shard_bytes = int(shard_bytes)
        if self.shard_bytes < 1:
            raise ValueError("shard_bytes must be positive")
        self._closed = False
        self._frame_shape = None
        self._dims = None
        self._lengths, self._labeled = [], []
        self._action, self._proprio, self._ids = [], [], []
        self._pending, self._pending_bytes = [], 0
        self._shards = []
        self._rows = 0

    @staticmethod
    def _array(name, x, dtype, ndim):
        if not isinstance(x, np.ndarray) or x.dtype != dtype:
            raise ValueError(f"add_episode: {name} must be a numpy array of dtype {np.dtype(dtype).name}, got "
                             f"{getattr(x, 'dtype', type(x).__name__)}")
        if x.ndim != ndim:
            raise ValueError(f"add_episode: {name} must have {ndim} dimensions, got shape {x.shape}")
        return x

    def add_episode(self, frames, action, proprio, input_ids, labeled=True):
        if self._closed:
            raise ValueError("add_episode after close()")
        frames = self._array("frames", frames, np.uint8, 4 if getattr(frames, "ndim", 5) == 4 else 5)
        if frames.ndim == 4:  # [T, H, W, 3]: one camera
            frames = frames[:, None]
        action = self._array("action", action, np.float32, 2)
        proprio = self._array("proprio", proprio, np.float32, 2)
        input_ids = self._array("input_ids", input_ids, np.int32, 1)
        T = action.shape[0]
        if T < 1:
            raise ValueError("add_episode: an empty episode (0 steps)")
        if frames.shape[0] != T or proprio.shape[0] != T:
            raise ValueError(f"add_episode: ragged lengths: {frames.shape[0]} frames, {T} actions, "
                             f"{proprio.shape[0]} proprio rows")
        if frames.shape[-1] != 3:
            raise ValueError(f"add_episode: frames must be [T, C, H, W, 3] or [T, H, W, 3], got {frames.shape}")
        dims = (action.shape[1], proprio.shape[1], input_ids.shape[0])
        if self._dims is None:
            if min(dims) < 1 or min(frames.shape[1:]) < 1:
                raise ValueError("add_episode: every dimension must be positive")
            self._dims, self._frame_shape = dims, tuple(frames.shape[1:])
        if dims != self._dims or tuple(frames.shape[1:]) != self._frame_shape:
            raise ValueError(f"add_episode: (action_dim, proprio_dim, token length) {dims} and frame shape "
                             f"{tuple(frames.shape[1:])} differ from the first episode's {self._dims}, "
                             f"{self._frame_shape}")
        if not (np.isfinite(action).all() and np.isfinite(proprio).all()):
            raise ValueError("add_episode: action / proprio hold non-finite values")
        if self._pending and self._pending_bytes + frames.nbytes > self.shard_bytes:
            self._flush()
        self._pending.append(np.ascontiguousarray(frames))
        self._pending_bytes += frames.nbytes
        self._action.append(action.copy())
        self._proprio.append(proprio.copy())
        self._ids.append(input_ids.copy())
        self._lengths.append(T)
        self._labeled.append(bool(labeled))

    def _flush(self):
        if not self._pending:
            return
        name = "frames_%05d.npy" % len(self._shards)
        block = self._pending[0] if len(self._pending) == 1 else np.concatenate(self._pending, 0)
        np.save(os.path.join(self.path, name), block)
        self._shards.append({"file": name, "first_row": self._rows, "rows": int(block.shape[0])})
        self._rows += int(block.shape[0])
        self._pending, self._pending_bytes = [], 0

    def close(self):
        if self._closed:
            raise ValueError("close() called twice")
        if not self._lengths:
            raise ValueError("close(): the store has no episode")
        self._closed = True
        self._flush()
        offsets = np.concatenate([[0], np.cumsum(np.asarray(self._lengths, np.int64))]).astype(np.int64)
        action, proprio = np.concatenate(self._action, 0), np.concatenate(self._proprio, 0)
        np.save(os.path.join(self.path, "episode_offsets.npy"), offsets)
        np.save(os.path.join(self.path, "action.npy"), action)
        np.save(os.path.join(self.path, "proprio.npy"), proprio)
        np.save(os.path.join(self.path, "input_ids.npy"), np.stack(self._ids, 0))
        with open(os.path.join(self.path, "statistics.json"), "w") as f:
            json.dump(compute_statistics(action, proprio, len(self._lengths)), f)
        meta = {"format_version": FORMAT_VERSION, "num_episodes": len(self._lengths),
                "num_transitions": int(offsets[-1]), "frame_shape": list(self._frame_shape),
                "action_dim": self._dims[0], "proprio_dim": self._dims[1], "token_len": self._dims[2],
                "pad_token_id": self.pad_token_id, "shards": self._shards,
                "labeled": [int(x) for x in self._labeled]}
        with open(os.path.join(self.path, "meta.json"), "w") as f:  # written last: a store without it is incomplete
            json.dump(meta, f)
        return self.path

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None and not self._closed:
            self.close()
        return False


class EpisodeStore:
    """Opens and validates a store.  The per-step arrays are read into memory (they are small); the frame shards stay
    memory-mapped."""

    def __init__(self, path):
        self.path = str(path)
        for f in FILES:
            if not os.path.exists(os.path.join(self.path, f)):
                raise ValueError(f"{self.path} is not an episode store: {f} is missing")
        with open(os.path.join(self.path, "meta.json")) as f:
            m = json.load(f)
        if m.get("format_version") != FORMAT_VERSION:
            raise ValueError(f"{self.path}: format version {m.get('format_version')!r}, this reader knows "
                             f"{FORMAT_VERSION}")
        self.meta = m
        self.num_episodes, self.num_transitions = int(m["num_episodes"]), int(m["num_transitions"])
        self.frame_shape = tuple(int(x) for x in m["frame_shape"])
        self.num_cameras, self.height, self.width = self.frame_shape[:3]
        self.action_dim, self.proprio_dim = int(m["action_dim"]), int(m["proprio_dim"])
        self.token_len, self.pad_token_id = int(m["token_len"]), int(m["pad_token_id"])
        self.labeled = np.asarray(m["labeled"], bool)
        load = lambda name: np.load(os.path.join(self.path, name))  # noqa: E731
        self.episode_offsets = load("episode_offsets.npy")
        self.action, self.proprio, self.input_ids = load("action.npy"), load("proprio.npy"), load("input_ids.npy")
        with open(os.path.join(self.path, "statistics.json")) as f:
            self.statistics = json.load(f)
        E, N = self.num_episodes, self.num_transitions
        off = self.episode_offsets
        if off.dtype != np.int64 or off.shape != (E + 1,) or E < 1:
            raise ValueError(f"{self.path}: episode_offsets.npy must be int64 [{E + 1}], got {off.dtype} {off.shape}")
        if off[0] != 0 or off[-1] != N or (np.diff(off) < 1).any():
            raise ValueError(f"{self.path}: episode offsets must rise strictly from 0 to num_transitions = {N}")
        if len(self.frame_shape) != 4 or self.frame_shape[3] != 3 or min(self.frame_shape) < 1:
            raise ValueError(f"{self.path}: frame shape must be [C, H, W, 3], got {list(self.frame_shape)}")
        for name, arr, dt, shape in (("action.npy", self.action, np.float32, (N, self.action_dim)),
                                     ("proprio.npy", self.proprio, np.float32, (N, self.proprio_dim)),
                                     ("input_ids.npy", self.input_ids, np.int32, (E, self.token_len))):
            if arr.dtype != dt or arr.shape != shape:
                raise ValueError(f"{self.path}: {name} must be {np.dtype(dt).name} {list(shape)}, got {arr.dtype} "
                                 f"{list(arr.shape)}")
        if self.labeled.shape != (E,):
            raise ValueError(f"{self.path}: meta.json must hold one labeled flag per episode")
        self.shards, row = [], 0
        for s in m["shards"]:
            a = np.load(os.path.join(self.path, s["file"]), mmap_mode="r")
            if a.dtype != np.uint8 or a.shape != (int(s["rows"]), *self.frame_shape) or int(s["first_row"]) != row:
                raise ValueError(f"{self.path}: {s['file']} must be uint8 [{s['rows']}, C, H, W, 3] starting at row "
                                 f"{row}, got {a.dtype} {list(a.shape)} at {s['first_row']}")
            if row not in off:
                raise ValueError(f"{self.path}: {s['file']} starts inside an episode (row {row})")
            self.shards.append(a)
            row += a.shape[0]
        if row != N:
            raise ValueError(f"{self.path}: the frame shards hold {row} rows, num_transitions is {N}")
        self._shard_first = np.asarray([int(s["first_row"]) for s in m["shards"]], np.int64)
        self.episode_of = np.repeat(np.arange(E, dtype=np.int32), np.diff(off))

    @property
    def frame_bytes(self):
        return int(np.prod(self.frame_shape))

    def check_dims(self, action_dim, proprio_dim, max_seq_len, num_images):
        """the store against the model config it is to be used with"""
        got = (self.action_dim, self.proprio_dim, self.token_len, self.num_cameras)
        want = (int(action_dim), int(proprio_dim), int(max_seq_len), int(num_images))
        if got != want:
            raise ValueError(f"{self.path}: the store's (action_dim, proprio_dim, token length, cameras) = {got} do "
                             f"not match the config's (action_dim, proprio_dim, max_seq_len, num_images) = {want}")

    def eligible_episodes(self, skip_unlabeled=False, max_action=None, max_proprio=None):
        """bool [E]: the reference's three filters (src/data/dataset.py:89-120) on the raw values"""
        ok = np.ones(self.num_episodes, bool)
        if skip_unlabeled:
            ok &= self.labeled
        starts = self.episode_offsets[:-1]
        for bound, arr in ((max_action, self.action), (max_proprio, self.proprio)):
            if bound is not None:
                ok &= np.maximum.reduceat(np.abs(arr).max(1), starts) <= float(bound)
        return ok

    def read_frames(self, rows, out=None):
        """uint8 [len(rows), C, H, W, 3] of the given store rows, copied out of the memory maps (host work only)"""
        rows = np.asarray(rows, np.int64)
        if rows.ndim != 1 or (rows.size and (rows.min() < 0 or rows.max() >= self.num_transitions)):
            raise ValueError(f"read_frames: rows must be one-dimensional in [0, {self.num_transitions})")
        if out is None:
            out = np.empty((rows.size, *self.frame_shape), np.uint8)
        which = np.searchsorted(self._shard_first, rows, side="right") - 1
        for i, (r, s) in enumerate(zip(rows.tolist(), which.tolist())):
            out[i] = self.shards[s][r - int(self._shard_first[s])]
        return out
