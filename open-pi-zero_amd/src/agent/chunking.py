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
