"""Several flow draws per observation (flow_samples_per_observation) stated on the CPU oracle.

The feature is defined by an equivalence: B observations with S draws (t, x0) each give the loss and the gradients of
the oracle's own ``pizero_loss`` (oracle/pizero_oracle.py, read-only) on the batch of B * S samples in which observation
b is repeated S times, sample e = b * S + s carrying draw s.  This file builds that replicated batch from the fixture
inputs and runs the oracle on it; nothing else is restated.  With S = 1 the batch is the fixture's and the run is
oracle_helpers.oracle_run's, bit for bit (tests/test_flow_draws_host.py).
"""

from __future__ import annotations

import numpy as np
import torch

from oracle.synth import synth_inputs
from tests.oracle_helpers import O, frozen


def draws(inp, S, seed=7):
    """(t [B, S], x0 [B, S, H, A]) float32 numpy: draw 0 is the fixture's own (t, x0); the others are distinct, from
    a generator of their own (t uniform in [0.02, 0.98], x0 standard normal)"""
    t0, x00 = inp["t"], inp["x0"]
    B = t0.shape[0]
    g = np.random.default_rng(seed)
    t = np.empty((B, S), np.float32)
    x0 = np.empty((B, S, *x00.shape[1:]), np.float32)
    t[:, 0], x0[:, 0] = t0, x00
    for s in range(1, S):
        t[:, s] = g.uniform(0.02, 0.98, B).astype(np.float32)
        x0[:, s] = g.standard_normal(x00.shape).astype(np.float32)
    return t, x0


def draws_run(d, bsz, S, bf16=False, ragged=True, prefix_len=None, seed=7):
    """loss and every gradient of the oracle on the S-fold replicated fixture batch with the draws of ``draws``.
    ``bf16`` runs it under CPU autocast (tests/prefix_ref.py's rule): its deviation from the fp32 run is what the parity
    tolerances may widen to.  ``prefix_len`` [B] or [B, S]: the action-prefix restatement (tests/prefix_ref.py) on the
    replicated batch instead of pizero_loss."""
    W = O.synth_weights(d, seed=0)
    seen = {}
    for k, v in W.items():
        if id(v) not in seen:
            seen[id(v)] = v.requires_grad_(not frozen(d, k))
    inp = synth_inputs(d, bsz, seed=0, ragged=ragged)
    t, x0 = draws(inp, S, seed)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    rep = lambda a: T(a) if S == 1 else T(np.repeat(a, S, axis=0))  # noqa: E731
    ids = rep(inp["input_ids"])
    mask, vpos, ppos, apos = O.build_mask_and_positions(d, rep(inp["attention_mask"]))
    args = (W, d, ids, rep(inp["pixel_values"]), mask, vpos, ppos, apos, rep(inp["proprios"]), rep(inp["actions"]),
            T(t.reshape(bsz * S)), T(x0.reshape(bsz * S, *x0.shape[2:])))
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16):
        if prefix_len is None:
            loss = O.pizero_loss(*args)
        else:
            from tests.prefix_ref import prefix_loss

            pl = torch.as_tensor(prefix_len, dtype=torch.int64)
            pl = pl.repeat_interleave(S) if pl.dim() == 1 else pl.reshape(bsz * S)
            loss = prefix_loss(*args, pl)
    loss.backward()
    grads = {k: (None if v.grad is None else v.grad.detach().float().clone()) for k, v in W.items()}
    return {"loss": loss.item(), "grads": grads, "t": t, "x0": x0}, inp
