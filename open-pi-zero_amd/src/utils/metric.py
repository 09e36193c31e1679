"""Validation metrics of the training loop (the reference's src/utils/metric.py)."""

from __future__ import annotations

import torch


def get_action_accuracy(gt, pred, thresholds=(0.1, 0.2)):
    """Fraction of (sample, step) rows of ``[B, H, A]`` action chunks whose EVERY action dimension is within the
    threshold of the ground truth (strictly: |gt - pred| < threshold), one fp32 value per threshold, on gt's device."""
    err = (gt - pred).abs().reshape(-1, gt.shape[-1])
    out = torch.zeros(len(thresholds), device=gt.device)
    for i, thr in enumerate(thresholds):
        out[i] = (err < thr).all(dim=1).float().mean()
    return out
