"""numpy restatement of the episode store's batch assembly, for the tests.

Written from the specification with explicit loops, not from the implementation's vectorised code: the chunking index
rules, the statistics, the normalisation (tests/obs_ref.py's formulas), the NHWC -> NCHW layout change and the sampler.
The sampler's only shared piece is the counter-based generator itself (pizero_native.augment.generator): the draw is
part of the specification ("a permutation drawn from generator(seed, epoch, rank, stream)").
"""

from __future__ import annotations

import numpy as np

from tests import obs_ref


# ---- chunking (reference src/data/traj_transforms.py:12-71) -----------------------------------------------------
def sample_rows(t, s, e, W, H):
    """sample at store row t of the episode occupying rows [s, e): (obs rows [W], action rows [H], pad mask [H])"""
    obs, act, mask = [], [], []
    for w in range(W):
        obs.append(max(t - W + 1 + w, s))
    for h in range(H):
        act.append(min(t + h, e - 1))
        mask.append(t + h <= e - 1)
    return obs, act, mask


def episode_bounds(offsets, t):
    for e in range(len(offsets) - 1):
        if offsets[e] <= t < offsets[e + 1]:
            return e, int(offsets[e]), int(offsets[e + 1])
    raise ValueError(t)


def gather_rows(action, proprio, offsets, tokens, idx, W, H, pad_id):
    """the five outputs of ops.episode_gather_rows for (already normalised) action [N, A] / proprio [N, P]"""
    B, A, P, L = len(idx), action.shape[1], proprio.shape[1], tokens.shape[1]
    out = {"action": np.zeros((B, H, A), np.float32), "proprio": np.zeros((B, W, P), np.float32),
           "action_pad_mask": np.zeros((B, H), np.uint8), "input_ids": np.zeros((B, L), np.int64),
           "attention_mask": np.zeros((B, L), np.int64)}
    for b, t in enumerate(idx):
        e, s, en = episode_bounds(offsets, int(t))
        obs, act, mask = sample_rows(int(t), s, en, W, H)
        for w, r in enumerate(obs):
            out["proprio"][b, w] = proprio[r]
        for h, r in enumerate(act):
            out["action"][b, h] = action[r]
            out["action_pad_mask"][b, h] = 1 if mask[h] else 0
        for j in range(L):
            out["input_ids"][b, j] = tokens[e, j]
            out["attention_mask"][b, j] = 1 if tokens[e, j] != pad_id else 0
    return out


def gather_frames(frames, idx):
    """uint8 [N, C, H, W, 3] at rows idx -> [len(idx) * C, 3, H, W]"""
    N, C, H, W, _ = frames.shape
    out = np.zeros((len(idx) * C, 3, H, W), np.uint8)
    for b, r in enumerate(idx):
        for c in range(C):
            for ch in range(3):
                out[b * C + c, ch] = frames[int(r), c, :, :, ch]
    return out


# ---- statistics (reference src/data/utils/data_utils.py:161-183) -------------------------------------------------
def statistics(action, proprio, num_trajectories):
    def one(x):
        return {"mean": x.mean(0).tolist(), "std": x.std(0).tolist(), "max": x.max(0).tolist(),
                "min": x.min(0).tolist(), "p99": np.quantile(x, 0.99, 0).tolist(),
                "p01": np.quantile(x, 0.01, 0).tolist()}

    return {"action": one(action), "num_transitions": int(len(action)), "num_trajectories": int(num_trajectories),
            "proprio": one(proprio)}


# ---- normalisation (data_utils.py:250-298), fp64 --------------------------------------------------------------------
def normalize(x, stats, kind, n_pass=0):
    """fp64; the trailing n_pass dimensions pass through"""
    x = np.asarray(x, np.float64)
    k = x.shape[-1] - n_pass
    if kind == "bound":
        head = obs_ref.normalize_bound(x[..., :k], np.asarray(stats["p01"], np.float32)[:k],
                                       np.asarray(stats["p99"], np.float32)[:k])
    else:
        head = obs_ref.normalize_gaussian(x[..., :k], np.asarray(stats["mean"], np.float32)[:k],
                                          np.asarray(stats["std"], np.float32)[:k])
    return np.concatenate([head, x[..., k:]], axis=-1)


def normalize_f32(x, stats, kind, n_pass=0):
    """the same two formulas with every operation rounded to fp32, in the order the kernels evaluate them
    (pz_proprio_normalize / pz_action_normalize are compiled without FMA contraction, and IEEE fp32 add / multiply /
    divide give the same bits anywhere: tests/test_prefix_kernels_gpu.py holds the kernels to this statement)"""
    f = np.float32
    x = np.asarray(x, f)
    k = x.shape[-1] - n_pass
    out = x.copy()
    v = x[..., :k]
    if kind == "bound":
        p, q = np.asarray(stats["p01"], f)[:k], np.asarray(stats["p99"], f)[:k]
        o = f(2.0) * (v - p) / ((q - p) + f(1e-8)) - f(1.0)
        out[..., :k] = np.minimum(np.maximum(o, f(-1.0)), f(1.0))
    else:
        p, q = np.asarray(stats["mean"], f)[:k], np.asarray(stats["std"], f)[:k]
        out[..., :k] = (v - p) / (q + f(1e-8))
    assert out.dtype == f
    return out


# ---- filters (reference src/data/dataset.py:89-120) ---------------------------------------------------------------
def eligible(offsets, labeled, action, proprio, skip_unlabeled=False, max_action=None, max_proprio=None):
    ok = []
    for e in range(len(offsets) - 1):
        s, en = int(offsets[e]), int(offsets[e + 1])
        keep = True
        if skip_unlabeled and not labeled[e]:
            keep = False
        if max_action is not None and np.abs(action[s:en]).max() > max_action:
            keep = False
        if max_proprio is not None and np.abs(proprio[s:en]).max() > max_proprio:
            keep = False
        ok.append(keep)
    return ok


# ---- sampler -----------------------------------------------------------------------------------------------------------
def rank_episodes(ok, rank, world):
    """the i-th eligible episode goes to rank i % world"""
    mine, i = [], 0
    for e, keep in enumerate(ok):
        if keep:
            if i % world == rank:
                mine.append(e)
            i += 1
    return mine


def rank_frames(offsets, ok, rank, world):
    rows = []
    for e in rank_episodes(ok, rank, world):
        for t in range(int(offsets[e]), int(offsets[e + 1])):
            rows.append(t)
    return rows


def epoch_length(offsets, ok, world):
    return min(len(rank_frames(offsets, ok, r, world)) for r in range(world))


def epoch_rows(offsets, ok, seed, epoch, rank, world, stream):
    from pizero_native.augment import generator

    rows = rank_frames(offsets, ok, rank, world)
    n = epoch_length(offsets, ok, world)
    perm = generator(seed, epoch, rank, stream=stream).permutation(len(rows))
    return [rows[int(perm[i])] for i in range(n)]


def batch_rows(offsets, ok, seed, k, rank, world, B, stream):
    """micro-batch k: positions [k B, (k + 1) B) of the rank's concatenated epochs"""
    n = epoch_length(offsets, ok, world)
    out, cache = [], {}
    for pos in range(k * B, (k + 1) * B):
        j = pos // n
        if j not in cache:
            cache[j] = epoch_rows(offsets, ok, seed, j, rank, world, stream)
        out.append(cache[j][pos - j * n])
    return np.asarray(out, np.int64)


def batch(store, idx, W, H, action_kind="bound", proprio_kind="bound", n_pass=1):
    """the whole reference-format batch of rows idx from an EpisodeStore, on the host (normalize_f32: the bits)"""
    st = store.statistics
    act = normalize_f32(store.action, st["action"], action_kind, n_pass)
    pro = normalize_f32(store.proprio, st["proprio"], proprio_kind)
    out = gather_rows(act, pro, store.episode_offsets, store.input_ids, idx, W, H, store.pad_token_id)
    out["pixel_values"] = gather_frames(store.read_frames(np.arange(store.num_transitions)), idx)
    return out
