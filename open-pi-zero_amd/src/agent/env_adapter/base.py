"""Host-side statement of the env adapter's normalisation (reference src/agent/env_adapter/base.py:8-49), in numpy.

The device path (``pz_proprio_normalize`` / ``pz_action_denormalize``, csrc/pz_obs.hip) computes the same four
formulas in fp32 inside the captured inference graph; this class is what they are checked against and what a caller
without a GPU in the loop (a dataset tool, a unit test) uses.  Arrays broadcast as numpy does; nothing is rounded.
"""

from __future__ import annotations

import json

import numpy as np

NORMALIZATION_TYPES = ("bound", "gaussian")


def load_dataset_statistics(path):
    """The reference's dataset-statistics JSON (config/bridge_statistics.json layout): ``proprio`` and ``action``
    nodes, each with per-dimension ``p01``, ``p99``, ``mean``, ``std``."""
    with open(path) as f:
        stats = json.load(f)
    for node in ("proprio", "action"):
        missing = [k for k in ("p01", "p99", "mean", "std") if k not in stats.get(node, {})]
        if missing:
            raise ValueError(f"{path}: dataset statistics lack {node}.{missing[0]}")
    return stats


class BaseEnvAdapter:
    def normalize_bound(self, data, data_min, data_max, clip_min=-1, clip_max=1, eps=1e-8):
        """[data_min, data_max] -> [-1, 1], then clipped to [clip_min, clip_max]"""
        span = np.asarray(data_max) - np.asarray(data_min) + eps
        return np.clip(2 * (np.asarray(data) - data_min) / span - 1, clip_min, clip_max)

    def denormalize_bound(self, data, data_min, data_max, clip_min=-1, clip_max=1, eps=1e-8):
        """[clip_min, clip_max] -> [data_min, data_max] (eps is accepted and unused, as in the reference)"""
        unit = (np.asarray(data) - clip_min) / (clip_max - clip_min)
        return unit * (np.asarray(data_max) - np.asarray(data_min)) + data_min

    def normalize_gaussian(self, data, mean, std, eps=1e-8):
        return (np.asarray(data) - mean) / (np.asarray(std) + eps)

    def denormalize_gaussian(self, data, mean, std, eps=1e-8):
        return np.asarray(data) * (np.asarray(std) + eps) + mean

    # the two directions as the rollout uses them (simpler.py:76-90, 105-126), by normalisation type
    def normalize_proprio(self, raw_proprio, stats, kind="bound"):
        s = stats["proprio"]
        if kind == "bound":
            return self.normalize_bound(raw_proprio, np.array(s["p01"]), np.array(s["p99"]))
        if kind == "gaussian":
            return self.normalize_gaussian(raw_proprio, np.array(s["mean"]), np.array(s["std"]))
        raise ValueError(f"proprio_normalization_type must be one of {NORMALIZATION_TYPES}, got {kind!r}")

    def denormalize_action(self, actions, stats, kind="bound", n_pass=1):
        """every dimension but the trailing ``n_pass`` (the gripper is not normalised in the training data)"""
        s = stats["action"]
        actions = np.asarray(actions)
        k = actions.shape[-1] - n_pass
        if kind == "bound":
            head = self.denormalize_bound(actions[..., :k], np.array(s["p01"])[:k], np.array(s["p99"])[:k])
        elif kind == "gaussian":
            head = self.denormalize_gaussian(actions[..., :k], np.array(s["mean"])[:k], np.array(s["std"])[:k])
        else:
            raise ValueError(f"action_normalization_type must be one of {NORMALIZATION_TYPES}, got {kind!r}")
        return np.concatenate([head, actions[..., k:]], axis=-1)

    def normalize_action(self, actions, stats, kind="bound", n_pass=1):
        """the inverse of ``denormalize_action`` (robot units -> the model's action units; the device form is
        ``pz_action_normalize``): ``normalize_bound`` with its clip, or ``normalize_gaussian``, on every dimension
        but the trailing ``n_pass``"""
        s = stats["action"]
        actions = np.asarray(actions)
        k = actions.shape[-1] - n_pass
        if kind == "bound":
            head = self.normalize_bound(actions[..., :k], np.array(s["p01"])[:k], np.array(s["p99"])[:k])
        elif kind == "gaussian":
            head = self.normalize_gaussian(actions[..., :k], np.array(s["mean"])[:k], np.array(s["std"])[:k])
        else:
            raise ValueError(f"action_normalization_type must be one of {NORMALIZATION_TYPES}, got {kind!r}")
        return np.concatenate([head, actions[..., k:]], axis=-1)
