"""Action-prefix conditioning restated on the CPU oracle's pieces.

No reference implementation of this feature exists in the project this one is modelled on; the semantics are fixed in
DESIGN 7f and this file is their executable statement, composed from oracle/pizero_oracle.py (read-only): psi_t,
time_embedding on the flattened per-row flow times, linear, joint_forward, split_mask.  With every prefix length 0 it
performs the oracle's own operations in the oracle's order, so it equals O.pizero_loss / O.pizero_infer bit for bit
(tests/test_prefix_host.py).

Row h of sample b is a prefix row iff h < prefix_len[b].  Training: a prefix row's encoder input is x1 (no noise
term), its flow time 1, and it carries no loss; the loss is the sum over the other rows divided by A * sum_b (H - d_b).
Inference: prefix rows start as the given prefix, are embedded with time 1 at every step, are never updated and are
exempt from the final clamp; the sample's t still advances by dt every step.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.synth import synth_inputs
from tests.oracle_helpers import O, frozen


def prefix_rows(prefix_len, H):
    """bool [B, H]: True on prefix rows"""
    return torch.arange(H)[None, :] < torch.as_tensor(prefix_len, dtype=torch.int64)[:, None]


def row_times(t, pre):
    """[B, H] flow time of every action row: 1 on prefix rows, the sample's t elsewhere"""
    return torch.where(pre, torch.ones((), dtype=t.dtype), t[:, None].expand(pre.shape))


def action_encoder_rows(W, d, a, t_rows):
    """O.action_encoder with one time per ROW: W3 silu(W2 [temb(t_rows[b, h]), W1 a[b, h]])"""
    B, H = t_rows.shape
    te = O.time_embedding(d, t_rows.reshape(-1)).view(B, H, -1)
    e = O.linear(a, W, "action_encoder.linear_1")
    e = torch.cat([te, e], dim=-1)
    e = F.silu(O.linear(e, W, "action_encoder.linear_2"))
    return O.linear(e, W, "action_encoder.linear_3")


def prefix_loss(W, d, input_ids, pixel_values, causal_mask, vlm_pos, proprio_pos, action_pos, proprios, actions, t, x0,
                prefix_len):
    x1 = actions
    B, H, A = x1.shape
    pre = prefix_rows(prefix_len, H)
    psi = torch.where(pre[..., None], x1, O.psi_t(d, x0, x1, t))
    emb = O.embed_siglip_and_text(W, d, input_ids, pixel_values)
    pe = O.linear(proprios, W, "proprio_encoder")
    ae = action_encoder_rows(W, d, psi, row_times(t, pre))
    out = O.joint_forward(W, d, {"vlm": emb, "proprio": pe, "action": ae},
                          {"vlm": vlm_pos, "proprio": proprio_pos, "action": action_pos}, causal_mask)["action"]
    v = O.linear(out, W, "action_decoder")
    dpsi = x1 - (1 - d["flow_sig_min"]) * x0
    live = (~pre)[..., None].to(v.dtype)
    n = A * int((H - torch.as_tensor(prefix_len, dtype=torch.int64)).sum())
    return torch.sum((v - dpsi) ** 2 * live) / n


def prefix_infer(W, d, input_ids, pixel_values, itp_mask, action_mask, vlm_pos, proprio_pos, action_pos, proprios,
                 noise, prefix, prefix_len, clip=True):
    emb = O.embed_siglip_and_text(W, d, input_ids, pixel_values)
    pe = O.linear(proprios, W, "proprio_encoder")
    _, cache = O.joint_forward(W, d, {"vlm": emb, "proprio": pe}, {"vlm": vlm_pos, "proprio": proprio_pos}, itp_mask,
                               return_cache=True)
    pre = prefix_rows(prefix_len, noise.shape[1])
    a = torch.where(pre[..., None], prefix.to(noise.dtype), noise)
    n = d["num_inference_steps"]
    dt = 1.0 / n
    t = torch.zeros(a.shape[0], dtype=a.dtype)
    for _ in range(n):
        ae = action_encoder_rows(W, d, a, row_times(t, pre))
        h = O.joint_forward(W, d, {"action": ae}, {"action": action_pos}, action_mask, cache=cache)["action"]
        a = torch.where(pre[..., None], a, a + dt * O.linear(h, W, "action_decoder"))
        t = t + dt
    if clip and d["final_action_clip_value"] is not None:
        c = d["final_action_clip_value"]
        a = torch.where(pre[..., None], a, torch.clamp(a, -c, c))
    return a


def restatement_run(d, bsz, prefix_len, prefix=None, bf16=False, want_grads=True, ragged=True, clip=False):
    """oracle_helpers.oracle_run with a prefix: loss (+ every gradient) and the action chunk on the fixture inputs.
    ``prefix`` defaults to the fixture's ground-truth actions.  ``bf16`` runs the same statement under CPU autocast
    (every Linear and matmul in bf16, fp32 weights and accumulation elsewhere): its deviation from the fp32 run is
    what the parity tolerances may widen to.  The weights require grad exactly as in oracle_run (torch's CPU kernels
    differ in the last bit between grad and no-grad mode, so the two runs must share it to compare bitwise)."""
    W = O.synth_weights(d, seed=0)
    seen = {}
    for k, v in W.items():
        if id(v) not in seen:
            seen[id(v)] = v.requires_grad_(not frozen(d, k))
    inp = synth_inputs(d, bsz, seed=0, ragged=ragged)
    T = lambda a: torch.from_numpy(a)  # noqa: E731
    ids = T(inp["input_ids"])
    mask, vpos, ppos, apos = O.build_mask_and_positions(d, T(inp["attention_mask"]))
    pl = torch.as_tensor(prefix_len, dtype=torch.int64)
    cast = torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16)
    with cast:
        loss = prefix_loss(W, d, ids, T(inp["pixel_values"]), mask, vpos, ppos, apos, T(inp["proprios"]),
                           T(inp["actions"]), T(inp["t"]), T(inp["x0"]), pl)
    out = {"loss": loss.item()}
    if want_grads:
        loss.backward()
        out["grads"] = {k: (None if v.grad is None else v.grad.detach().float().clone()) for k, v in W.items()}
    pf = T(inp["actions"]) if prefix is None else torch.as_tensor(prefix, dtype=torch.float32)
    with torch.no_grad(), cast:
        itp, amask = O.split_mask(d, mask)
        out["actions"] = prefix_infer(W, d, ids, T(inp["pixel_values"]), itp, amask, vpos, ppos, apos,
                                      T(inp["proprios"]), T(inp["noise"]), pf, pl, clip=clip).float()
    return out, inp
