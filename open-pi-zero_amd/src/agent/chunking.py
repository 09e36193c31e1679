"""Chunk scheduling for action-prefix conditioning ("real-time chunking"), on the host.

A robot that executes chunk k while chunk k + 1 is being inferred has, by the time the inference returns, executed
``delay`` more actions of chunk k.  Those actions are the committed prefix of chunk k + 1: ``EvalAgent.act(...,
prev_actions=prefix, delay=d)`` denoises the rest of the new chunk around them.  The caller supplies ``delay`` (the
inference latency in control steps); nothing here measures it.
"""

from __future__ import annotations

import numpy as np


def next_prefix(prev_chunk, offset, delay):
    """``(prefix [H, A], d)`` for the chunk inferred from an observation taken after ``offset`` actions of
    ``prev_chunk`` [H, A] had been executed, when the inference takes ``delay`` control steps:

        d = max(0, min(delay, H - offset)),   prefix[:d] = prev_chunk[offset : offset + d],   prefix[d:] = 0.

    The new chunk's row 0 is the action executed right after the observation, so rows [0, d) of the new chunk are
    rows [offset, offset + d) of the previous one; where the previous chunk runs out (``offset + delay > H``) only
    what is left of it is committed.  ``d`` can reach H only with ``offset = 0`` and ``delay >= H``, which no
    caller that overlaps inference with execution produces; ``act`` refuses ``d > H - 1``.  Accepts numpy arrays or
    torch tensors and returns the same kind."""
    H = prev_chunk.shape[0]
    offset, delay = int(offset), int(delay)
    if prev_chunk.ndim != 2:
        raise ValueError(f"next_prefix: prev_chunk must be [H, A], got shape {tuple(prev_chunk.shape)}")
    if offset < 0 or delay < 0:
        raise ValueError(f"next_prefix: offset and delay must be non-negative, got {offset}, {delay}")
    d = max(0, min(delay, H - offset))
    if isinstance(prev_chunk, np.ndarray):
        prefix = np.zeros_like(prev_chunk)
    else:
        import torch

        prefix = torch.zeros_like(prev_chunk)
    if d:
        prefix[:d] = prev_chunk[offset:offset + d]
    return prefix, d


# ---- inference-time guidance toward the previous chunk (Black et al. 2025) ----
# The tables below are made on the host and loaded into static device inputs: the kernels (csrc/pz_rtc.hip) contain
# no exp and no division, and one captured graph serves every delay, overlap and beta.


def soft_mask(H, delay, overlap):
    """fp32 [H] guidance weights over the rows of the new chunk: 1 on the rows that will have been executed from the
    previous chunk when the inference returns (i < delay), an exponential decay over the rest of what the previous
    chunk still covers,

        W_i = c_i (e^{c_i} - 1) / (e - 1),   c_i = (overlap - i) / (overlap - delay + 1),   delay <= i < overlap,

    and 0 on the rows the previous chunk says nothing about (i >= overlap).  Computed in fp64, rounded once."""
    H, delay, overlap = int(H), int(delay), int(overlap)
    if not (0 <= delay <= overlap <= H):
        raise ValueError(f"soft_mask: need 0 <= delay <= overlap <= H, got delay {delay}, overlap {overlap}, H {H}")
    i = np.arange(H, dtype=np.float64)
    c = (overlap - i) / (overlap - delay + 1)
    w = c * np.expm1(c) / np.expm1(1.0)
    w = np.where(i < delay, 1.0, np.where(i < overlap, w, 0.0))
    return w.astype(np.float32)


def guidance_coef(steps, beta):
    """fp32 [steps]: the guidance weight of Euler step k, min(beta, (t^2 + (1 - t)^2) / (t (1 - t))) at t = k / steps
    (t = 0 noise, t = 1 clean); entry 0, where the ratio is unbounded, is beta.  Computed in fp64, rounded once."""
    steps, beta = int(steps), float(beta)
    if steps < 1 or not beta >= 0.0:
        raise ValueError(f"guidance_coef: need steps >= 1 and beta >= 0, got {steps}, {beta}")
    out = np.full(steps, beta, dtype=np.float64)
    t = np.arange(1, steps, dtype=np.float64) / steps
    out[1:] = np.minimum(beta, (t * t + (1 - t) * (1 - t)) / (t * (1 - t)))
    return out.astype(np.float32)


def next_guidance(prev_chunk, offset, delay):
    """``(target [H, A], delay, overlap)`` for the chunk inferred from an observation taken after ``offset`` actions
    of ``prev_chunk`` [H, A] had been executed -- the sibling of ``next_prefix`` for guidance:

        overlap = H - offset,   target[i] = prev_chunk[offset + i] for i < overlap,   target[i >= overlap] = the last row,
        delay   = max(0, min(delay, overlap)).

    The repeated rows carry weight 0 in ``soft_mask(H, delay, overlap)``; they only keep the target finite.  Accepts
    numpy arrays or torch tensors and returns the same kind."""
    if prev_chunk.ndim != 2:
        raise ValueError(f"next_guidance: prev_chunk must be [H, A], got shape {tuple(prev_chunk.shape)}")
    H = prev_chunk.shape[0]
    offset, delay = int(offset), int(delay)
    if offset < 0 or delay < 0:
        raise ValueError(f"next_guidance: offset and delay must be non-negative, got {offset}, {delay}")
    if offset > H - 1:
        raise ValueError(f"next_guidance: offset {offset} leaves nothing of a chunk of {H} rows")
    overlap = H - offset
    idx = np.minimum(np.arange(H) + offset, H - 1)
    if isinstance(prev_chunk, np.ndarray):
        target = prev_chunk[idx].copy()
    else:
        import torch

        target = prev_chunk[torch.as_tensor(idx, device=prev_chunk.device)].clone()
    return target, max(0, min(delay, overlap)), overlap
