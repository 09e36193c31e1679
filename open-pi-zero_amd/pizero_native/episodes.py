"""Training batches from an episode store: the sampler and the device batch assembly.

``EpisodeSampler`` (numpy, host) decides which store rows make micro-batch k of a rank; its draws are a function of
counters alone (pizero_native.augment.generator under EPISODE_STREAM), like the augmentation's and the prefix's: neither
torch's generator nor numpy's global one is touched, and ``seek(k)`` resumes the sequence anywhere.
``EpisodeBatches`` turns those rows into reference-format batches that are already on the device, with two launches
(ops.episode_gather_rows, ops.episode_gather_frames).  The action and proprio arrays are normalised once, when the store
is loaded, by ops.action_normalize / ops.proprio_normalize; the kernels gather only.

Frames live either in HBM (``frames_placement: device``: the rank's own episodes, copied once, under a stated cap) or in
the store's memory maps (``host``: one worker thread gathers the next micro-batch's frames into one of two pinned
staging buffers while the current step runs; the main thread issues the single H2D copy on a side stream and makes the
consumer's stream wait for it).  Both deliver the same bits.
"""

from __future__ import annotations

import queue
import threading
from collections import deque

import numpy as np

from .augment import EPISODE_STREAM, EPISODE_VAL_STREAM, generator

# 288 GB of HBM, of which a micro-batch-256 training step maps about 240: 48 GB are left, and a
# store is admitted to two thirds of that unless the config states another cap
DEFAULT_DEVICE_STORE_MAX_GB = 32.0
PLACEMENTS = ("device", "host", "auto")
WORKER_NAME = "episode-frames-worker"

# reference keys of data.train / data.val with no meaning here: refused by name when set
REFUSED_KEYS = ("goal_relabeling_strategy", "goal_relabeling_kwargs", "subsample_length", "task_augment_strategy",
                "task_augment_kwargs", "sample_weights", "balance_weights")
# accepted and ignored: how many host threads the reference's pipeline would use
IGNORED_KEYS = ("traj_transform_threads", "traj_read_threads", "num_parallel_calls", "num_parallel_reads",
                "frame_transform_threads", "shuffle_buffer_size")


def chunk_rows(t, s, e, window, horizon):
    """the reference's chunking (src/data/traj_transforms.py:12-71) for the sample at row t of an episode occupying
    rows [s, e): (observation rows [window], action rows [horizon], action_pad_mask [horizon])"""
    obs = np.maximum(t - window + 1 + np.arange(window), s)
    ahead = t + np.arange(horizon)
    return obs, np.minimum(ahead, e - 1), ahead <= e - 1


class EpisodeSampler:
    """Which rows make micro-batch k.  The i-th eligible episode belongs to rank i % world; an epoch of a rank is a
    permutation of the frames of its own episodes, truncated to n = the smallest such frame count over the ranks (every
    rank computes n from the offsets alone, so all take the same number of steps without a collective); micro-batch k
    is positions [k B, (k + 1) B) of the rank's concatenated epochs and may straddle two of them."""

    def __init__(self, episode_offsets, eligible, batch_size, seed=0, rank=0, world=1, stream=EPISODE_STREAM):
        off = np.asarray(episode_offsets, np.int64)
        eligible = np.asarray(eligible, bool)
        if eligible.shape != (off.size - 1,):
            raise ValueError("EpisodeSampler: one eligibility flag per episode expected")
        self.batch_size, self.seed, self.rank, self.world = int(batch_size), int(seed), int(rank), int(world)
        self.stream = int(stream)
        if self.batch_size < 1 or self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f"EpisodeSampler: batch_size {batch_size}, rank {rank}, world {world} are not valid")
        ids = np.flatnonzero(eligible)
        if ids.size == 0:
            raise ValueError("EpisodeSampler: the filters leave no eligible episode")
        if ids.size < self.world:
            raise ValueError(f"EpisodeSampler: {ids.size} eligible episodes cannot be dealt to {self.world} ranks")
        lengths = off[1:] - off[:-1]
        self.episodes = ids[self.rank::self.world]
        self.frames_per_epoch = int(min(lengths[ids[r::self.world]].sum() for r in range(self.world)))
        # the rank's own frames in store order: sorted, so a store row's place in the rank's shard is a searchsorted
        self.rows = np.concatenate([np.arange(off[e], off[e + 1], dtype=np.int64) for e in self.episodes])
        self._epochs = {}

    def epoch(self, j):
        """int64 [n]: the store rows of epoch j, in the order they are sampled"""
        if j not in self._epochs:
            if len(self._epochs) >= 2:
                self._epochs.pop(min(self._epochs))
            perm = generator(self.seed, j, self.rank, stream=self.stream).permutation(self.rows.size)
            self._epochs[j] = self.rows[perm[: self.frames_per_epoch]]
        return self._epochs[j]

    def batch(self, k):
        """int64 [B]: the store rows of micro-batch k"""
        if k < 0:
            raise ValueError("EpisodeSampler.batch: k must be non-negative")
        n, B = self.frames_per_epoch, self.batch_size
        out = np.empty(B, np.int64)
        pos, filled = k * B, 0
        while filled < B:
            j, o = divmod(pos, n)
            take = min(B - filled, n - o)
            out[filled: filled + take] = self.epoch(j)[o: o + take]
            filled += take
            pos += take
        return out


def _frames_worker(store, requests, results):
    """host copies only (memory map -> pinned staging buffer); no HIP call is made on this thread"""
    while True:
        job = requests.get()
        if job is None:
            return
        k, rows, buf = job
        try:
            store.read_frames(rows, out=buf)
            results.put((k, None))
        except BaseException as exc:  # noqa: BLE001 -- handed to the consumer, which raises it
            results.put((k, exc))


class EpisodeBatches:
    """Iterable of reference-format batches on the device: input_ids, attention_mask (int64 [B, L]), pixel_values
    (uint8 [B * C, 3, H, W]), proprio (fp32 [B, window, P]), action (fp32 [B, horizon, A]), action_pad_mask (uint8
    [B, horizon]).  ``seek(k)`` sets the next micro-batch; ``recent`` keeps the (k, rows) of the last batches handed
    out; ``close()`` joins the ``host`` placement's worker (it starts again with the next batch)."""

    def __init__(self, store, batch_size, window, horizon, device, *, seed=0, rank=0, world=1, stream=EPISODE_STREAM,
                 skip_unlabeled=False, max_action=None, max_proprio=None, action_normalization_type="bound",
                 proprio_normalization_type="bound", action_normalization_n_pass=1, frames_placement="auto",
                 device_store_max_gb=DEFAULT_DEVICE_STORE_MAX_GB):
        import torch

        from . import ops

        if frames_placement not in PLACEMENTS:
            raise ValueError(f"frames_placement must be one of {list(PLACEMENTS)}, got {frames_placement!r}")
        self.store, self.device = store, torch.device(device)
        self.window, self.horizon = int(window), int(horizon)
        eligible = store.eligible_episodes(skip_unlabeled, max_action, max_proprio)
        self.sampler = EpisodeSampler(store.episode_offsets, eligible, batch_size, seed, rank, world, stream)
        self.batch_size = self.sampler.batch_size
        self.recent = deque(maxlen=16)
        self._k = 0

        dev = self.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        st = store.statistics
        keys = {"bound": ("p01", "p99"), "gaussian": ("mean", "std")}
        for name, kind in (("action", action_normalization_type), ("proprio", proprio_normalization_type)):
            if kind not in keys:
                raise ValueError(f"{name}_normalization_type must be bound or gaussian, got {kind!r}")
        stat = lambda name, kind: [up(np.asarray(st[name][k], np.float32)) for k in keys[kind]]  # noqa: E731
        # normalised once, here: a gathered value is the normalised raw value, bit for bit
        self.action = ops.action_normalize(up(store.action), *stat("action", action_normalization_type),
                                           action_normalization_type, n_pass=int(action_normalization_n_pass))
        self.proprio = ops.proprio_normalize(up(store.proprio), *stat("proprio", proprio_normalization_type),
                                             proprio_normalization_type)
        self.episode_of, self.episode_offsets = up(store.episode_of), up(store.episode_offsets)
        self.tokens = up(store.input_ids)

        shard_bytes = int(self.sampler.rows.size) * store.frame_bytes
        cap_bytes = int(round(float(device_store_max_gb) * 1e9))
        if frames_placement == "auto":
            frames_placement = "device" if shard_bytes <= cap_bytes else "host"
        elif frames_placement == "device" and shard_bytes > cap_bytes:
            raise ValueError(f"frames_placement: device: this rank's frames take {shard_bytes} bytes, "
                             f"device_store_max_gb allows {cap_bytes} bytes; raise the cap or use host / auto")
        self.frames_placement = frames_placement
        self._worker = None
        if frames_placement == "device":
            self.frames = torch.empty((self.sampler.rows.size, *store.frame_shape), device=dev, dtype=torch.uint8)
            row = 0
            off = store.episode_offsets
            for e in self.sampler.episodes:  # its own episodes only, one copy each
                n = int(off[e + 1] - off[e])
                self.frames[row: row + n].copy_(torch.from_numpy(store.read_frames(np.arange(off[e], off[e + 1]))))
                row += n
        else:
            shape = (self.batch_size, *store.frame_shape)
            self._pinned = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self._staging = [torch.empty(shape, device=dev, dtype=torch.uint8) for _ in range(2)]
            self._copy_stream = torch.cuda.Stream(device=dev)
            self._copied = [None, None]  # the H2D copy out of each pinned buffer
            self._consumed = [None, None]  # the transpose out of each device staging buffer
            self._slot = 0
            self._pending = None  # (k, rows, slot) the worker is gathering or has gathered

    # ------------------------------------------------------------ iteration --
    def seek(self, k):
        k = int(k)
        if k < 0:
            raise ValueError("EpisodeBatches.seek: k must be non-negative")
        self._k = k

    def __iter__(self):
        return self

    def __next__(self):
        import torch

        from . import ops

        k = self._k
        rows = self.sampler.batch(k)
        with torch.cuda.device(self.device):
            batch = ops.episode_gather_rows(self.action, self.proprio, self.episode_of, self.episode_offsets,
                                            self.tokens, rows, self.window, self.horizon, self.store.pad_token_id)
            if self.frames_placement == "device":
                local = np.searchsorted(self.sampler.rows, rows)
                batch["pixel_values"] = ops.episode_gather_frames(self.frames, local)
            else:
                batch["pixel_values"] = self._host_frames(k, rows)
        self._k = k + 1
        self.recent.append((k, rows))
        return batch

    # ------------------------------------------------------- host placement --
    def _submit(self, k, rows):
        if self._worker is None:
            self._requests, self._results = queue.Queue(maxsize=1), queue.Queue(maxsize=1)
            self._worker = threading.Thread(target=_frames_worker, args=(self.store, self._requests, self._results),
                                            name=WORKER_NAME, daemon=True)
            self._worker.start()
        slot = self._slot
        self._slot ^= 1
        if self._copied[slot] is not None:  # the copy that last read this pinned buffer, issued a step ago
            self._copied[slot].synchronize()
        self._pending = (k, rows, slot)
        self._requests.put((k, rows, self._pinned[slot].numpy()))

    def _collect(self):
        k, exc = self._results.get()
        pending, self._pending = self._pending, None
        if exc is not None:
            self.close()
            raise exc
        assert pending is not None and pending[0] == k
        return pending

    def _host_frames(self, k, rows):
        import torch

        from . import ops

        try:
            if self._pending is not None and not (self._pending[0] == k and np.array_equal(self._pending[1], rows)):
                self._collect()  # a seek moved away from what was prefetched: drop it
            if self._pending is None:
                self._submit(k, rows)
            _, _, slot = self._collect()
            self._submit(k + 1, self.sampler.batch(k + 1))  # fixed depth one: gathered while step k runs
            consumer = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(self._copy_stream):
                if self._consumed[slot] is not None:  # the transpose that last read this staging buffer
                    self._copy_stream.wait_event(self._consumed[slot])
                self._staging[slot].copy_(self._pinned[slot], non_blocking=True)
                self._copied[slot] = torch.cuda.Event()
                self._copied[slot].record(self._copy_stream)
            consumer.wait_event(self._copied[slot])
            out = ops.episode_gather_frames(self._staging[slot], None)
            self._consumed[slot] = torch.cuda.Event()
            self._consumed[slot].record(consumer)
            return out
        except BaseException:
            self.close()
            raise

    def close(self):
        """join the worker (host placement); the next batch starts a new one"""
        w, self._worker = self._worker, None
        if w is None:
            return
        if self._pending is not None and w.is_alive():
            try:  # let the gather in flight finish, so that nothing writes a pinned buffer after this returns
                self._results.get(timeout=60)
            except queue.Empty:
                pass
        self._pending = None
        self._requests.put(None)
        w.join()
        for ev in self._copied:
            if ev is not None:
                ev.synchronize()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


def from_config(cfg, split, batch_size, rank, world, device):
    """``data.train`` / ``data.val`` (``split`` = "train" | "val") -> EpisodeBatches, or None when the node names no
    ``episode_store``.  Refuses by name the reference's keys that have no meaning here, a window / horizon that differ
    from cond_steps / horizon_steps, and a store whose dimensions do not match the model's."""
    from src.data.episode_store import EpisodeStore
    from src.utils.config import cfg_get

    node = cfg_get(cfg, f"data.{split}")
    path = cfg_get(node, "episode_store") if node is not None else None
    if not path:
        return None
    get = lambda key, default=None: cfg_get(node, key, default)  # noqa: E731
    for key in REFUSED_KEYS:
        if get(key) is not None:
            raise ValueError(f"data.{split}.{key} is not supported by the episode store (DESIGN 7g)")
    mix = get("dataset_mix")
    if mix is not None and not isinstance(mix, str) and len(mix) > 1:
        raise ValueError(f"data.{split}.dataset_mix with more than one dataset is not supported by the episode store")
    window, horizon = int(cfg_get(cfg, "cond_steps")), int(cfg_get(cfg, "horizon_steps"))
    for key, want, name in (("window_size", window, "cond_steps"), ("action_horizon", horizon, "horizon_steps")):
        if int(get(key, want)) != want:
            raise ValueError(f"data.{split}.{key} = {get(key)} must equal {name} = {want}")
    store = EpisodeStore(path)
    store.check_dims(cfg_get(cfg, "action_dim"), cfg_get(cfg, "proprio_dim"), cfg_get(cfg, "max_seq_len"),
                     cfg_get(cfg, "num_images", 1))
    if store.pad_token_id != int(cfg_get(cfg, "pad_token_id", 0)):
        raise ValueError(f"{path}: the store's pad token id {store.pad_token_id} is not the config's pad_token_id")
    opt = lambda key: None if get(key) is None else float(get(key))  # noqa: E731
    return EpisodeBatches(
        store, batch_size, window, horizon, device, seed=int(get("seed", cfg_get(cfg, "seed", 0))), rank=rank,
        world=world, stream=EPISODE_STREAM if split == "train" else EPISODE_VAL_STREAM,
        skip_unlabeled=bool(get("skip_unlabeled", False)), max_action=opt("max_action"),
        max_proprio=opt("max_proprio"), action_normalization_type=get("action_normalization_type", "bound"),
        proprio_normalization_type=get("proprio_normalization_type", "bound"),
        action_normalization_n_pass=int(get("action_normalization_n_pass", 1)),
        frames_placement=get("frames_placement", "auto"),
        device_store_max_gb=float(get("device_store_max_gb", DEFAULT_DEVICE_STORE_MAX_GB)))
