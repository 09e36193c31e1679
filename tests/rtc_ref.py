"""Inference-time guidance toward the previous chunk (Black et al. 2025, "real-time chunking") restated on
the CPU oracle's pieces.

No reference implementation of this feature exists in the project this one is modelled on; this file is the executable
statement of its semantics, composed from oracle/pizero_oracle.py (read-only).  In this repository's convention
(t = 0 noise, t = 1 clean) every Euler step is

    v     = denoiser(A_t, o, t)
    x1hat = A_t + (1 - t) v
    e     = W (.) (Y - x1hat)                  Y: what is left of the previous chunk, W: soft mask over rows
    g     = e + (1 - t) (dv/dA_t)^T e          the vector-Jacobian product of x1hat
    A    += dt (v + coef[k] g)                 coef[k] = min(beta, (t^2 + (1 - t)^2) / (t (1 - t))), coef[0] = beta

with flow_sig_min's 0.001 x0 offset of x1hat ignored.  With W = 0 the loop performs O.pizero_infer's operations in its
order and equals it bit for bit (tests/test_rtc_host.py).

Also here: float64 statements of the two host tables (src/agent/chunking.py) and numpy float32 restatements of the two
guidance kernels (csrc/pz_rtc.hip), every multiply and add rounded by itself, in the kernels' order.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from oracle.synth import synth_inputs
from tests.oracle_helpers import O

F32 = np.float32


# ---------------------------------------------------------------- host tables ----
def soft_mask_ref(H, delay, overlap):
    out = []
    for i in range(H):
        if i < delay:
            out.append(1.0)
        elif i < overlap:
            c = (overlap - i) / (overlap - delay + 1)
            out.append(c * (math.exp(c) - 1.0) / (math.e - 1.0))
        else:
            out.append(0.0)
    return np.asarray(out, dtype=np.float64)


def guidance_coef_ref(steps, beta):
    out = [float(beta)]
    for k in range(1, steps):
        t = k / steps
        out.append(min(float(beta), (t * t + (1 - t) * (1 - t)) / (t * (1 - t))))
    return np.asarray(out, dtype=np.float64)


# ------------------------------------------------------------ kernel restatements ----
def bf16_round(x):
    """float32 array -> the float32 values of its round-to-nearest-even bf16"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(F32)


def seed_np(action, v, target, w, t):
    """pz_rtc_seed: (e fp32 [B, H, A], bf16(e) as fp32); v holds bf16 values as fp32 [B, H, A]"""
    one = F32(1.0)
    tb = t.astype(F32)[:, None, None]
    x1 = (action.astype(F32) + ((one - tb) * v.astype(F32)).astype(F32)).astype(F32)
    e = (w.astype(F32)[:, :, None] * (target.astype(F32) - x1).astype(F32)).astype(F32)
    return e, bf16_round(e)


def euler_np(action, v, e, dA, t, coef_k, dt):
    """pz_rtc_euler: (action', t'); v and dA hold bf16 values as fp32 [B, H, A]"""
    one, dt, ck = F32(1.0), F32(dt), F32(coef_k)
    tb = t.astype(F32)[:, None, None]
    g = (e.astype(F32) + ((one - tb) * dA.astype(F32)).astype(F32)).astype(F32)
    inner = (v.astype(F32) + (ck * g).astype(F32)).astype(F32)
    return (action.astype(F32) + (dt * inner).astype(F32)).astype(F32), (t.astype(F32) + dt).astype(F32)


# ------------------------------------------------------------------ the loop ----
def denoiser(W, d, a, t, cache, action_pos, action_mask):
    """v(A_t, o, t): one evaluation of the action expert against the cached prefix, as O.pizero_infer's loop body"""
    te = O.time_embedding(d, t)
    ae = O.action_encoder(W, a, te)
    h = O.joint_forward(W, d, {"action": ae}, {"action": action_pos}, action_mask, cache=cache)["action"]
    return O.linear(h, W, "action_decoder")


def guided_step(W, d, a, t, cache, action_pos, action_mask, target, w, coef_k, dt, jacobian=True):
    """one guided Euler step; returns (a', v, e, dA) with dA = (dv/dA_t)^T e (zeros without the Jacobian term)"""
    a_in = a.detach().requires_grad_(True)
    with torch.enable_grad():
        v = denoiser(W, d, a_in, t, cache, action_pos, action_mask)
    tt = t[:, None, None]
    vd = v.detach().to(a.dtype)
    e = w[:, :, None] * (target - (a_in.detach() + (1 - tt) * vd))
    if jacobian:
        (dA,) = torch.autograd.grad(v, a_in, e.to(v.dtype))
        dA = dA.to(a.dtype)
    else:
        dA = torch.zeros_like(e)
    g = e + (1 - tt) * dA
    return a_in.detach() + dt * (vd + coef_k * g), vd, e, dA


def guided_infer(W, d, input_ids, pixel_values, itp_mask, action_mask, vlm_pos, proprio_pos, action_pos, proprios,
                 noise, target, w, coef, clip=True, jacobian=True):
    """O.pizero_infer with every Euler step guided toward ``target`` [B, H, A] with row weights ``w`` [B, H] and the
    per-step coefficients ``coef`` [steps]"""
    with torch.no_grad():
        emb = O.embed_siglip_and_text(W, d, input_ids, pixel_values)
        pe = O.linear(proprios, W, "proprio_encoder")
        _, cache = O.joint_forward(W, d, {"vlm": emb, "proprio": pe}, {"vlm": vlm_pos, "proprio": proprio_pos},
                                   itp_mask, return_cache=True)
    a = noise.clone()
    n = d["num_inference_steps"]
    dt = 1.0 / n
    t = torch.zeros(a.shape[0], dtype=a.dtype)
    for k in range(n):
        a, _, _, _ = guided_step(W, d, a, t, cache, action_pos, action_mask, target, w, float(coef[k]), dt, jacobian)
        t = t + dt
    if clip and d["final_action_clip_value"] is not None:
        c = d["final_action_clip_value"]
        a = torch.clamp(a, -c, c)
    return a


def fixture(d, bsz, ragged=True):
    """the fixture's weights (no gradient: the loop differentiates with respect to the actions only) and inputs"""
    W = O.synth_weights(d, seed=0)
    inp = synth_inputs(d, bsz, seed=0, ragged=ragged)
    T = lambda a: torch.from_numpy(a)  # noqa: E731
    mask, vpos, ppos, apos = O.build_mask_and_positions(d, T(inp["attention_mask"]))
    itp, amask = O.split_mask(d, mask)
    args = (T(inp["input_ids"]), T(inp["pixel_values"]), itp, amask, vpos, ppos, apos, T(inp["proprios"]),
            T(inp["noise"]))
    return W, inp, args


def restatement_run(d, bsz, target, w, coef, bf16=False, ragged=True, clip=False, jacobian=True):
    """the guided chunk on the fixture inputs; ``bf16`` runs the same statement under CPU autocast (every Linear and
    matmul in bf16): its deviation from the fp32 run is what a parity tolerance may widen to"""
    W, inp, args = fixture(d, bsz, ragged)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16):
        a = guided_infer(W, d, *args, torch.as_tensor(target, dtype=torch.float32),
                         torch.as_tensor(w, dtype=torch.float32), np.asarray(coef, dtype=np.float32), clip=clip,
                         jacobian=jacobian)
    return a.float(), inp
