"""Golden fixture of LoRA fine-tuning (lora: True), from the REFERENCE itself (build container only).

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lora.py

Same recipe as make_golden_adaln.py (make_golden.py's stubs, config and gradient probes) at TINY_DIMS, B=3,
ragged, fp32 + bf16, with ``use_lora=True`` and ``lora={r: 8, dropout: 0.0}`` in the vision, projector, joint and
``mixture.vlm`` copies of the config, then tie_action_proprio_weights(), freeze_unused_weights() and
freeze_non_lora_weights_in_vlm().  Weights: oracle.synth by name (synth_weights for the base tensors,
synth_state_dict for lora_A / lora_B), so lora_B is NOT zero (asserted) and the adapters carry signal.

Writes tests/golden/lora.npz: loss, gradient probes of EVERY named parameter (gradnorm -1 where the reference
has no grad), the reference's bf16-vs-fp32 grel / gcos, grad_names, sd_names / sd_shapes, ``trainable`` (names with
requires_grad after the three freeze calls), in/*, and ``actions_unclipped`` / ``actions_clipped`` from the
reference's cached infer_action after model.eval() (which merges W += B A).
Asserted: every trainable lora_ tensor has a non-zero fp32 gradient and a bf16 grel <= 1.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.pizero_oracle import TINY_DIMS, synth_weights  # noqa: E402
from oracle.synth import synth_inputs, synth_state_dict  # noqa: E402
from tests.golden.gradprobe import probe  # noqa: E402
from tests.golden.make_golden import REF, install_stubs, ref_cfg  # noqa: E402

RANK = 8
N_SAMPLE = 1024  # gradient samples per tensor: ~170 probed tensors stay well under 1 MiB


def lora_cfg(d, r=RANK):
    """ref_cfg with LoRA switched on in every copy the reference reads"""
    cfg = ref_cfg(d)
    lora = dict(r=r, dropout=0.0)
    cfg.vision.use_lora = True
    cfg.vision.config.lora = type(cfg.vision.config.lora)(lora)
    cfg.vision_projector.use_lora = True
    cfg.vision_projector.config.lora = type(cfg.vision_projector.config.lora)(lora)
    cfg.joint.config.lora = type(cfg.joint.config.lora)(lora)
    for mixes in (cfg.mixture, cfg.joint.config.mixture):
        mixes["vlm"].use_lora = True
    return cfg


def build_reference(d, meta=False):
    from src.model.vla import pizero as pz

    torch.manual_seed(0)
    if meta:
        with torch.device("meta"):
            model = pz.PiZero(lora_cfg(d))
    else:
        model = pz.PiZero(lora_cfg(d))
    model.tie_action_proprio_weights()
    model.freeze_unused_weights()
    model.freeze_non_lora_weights_in_vlm()
    return model


def lora_weights(d, sd_shapes):
    """name -> fp32 tensor for the reference state_dict; proprio keys alias the action tensors (tied)"""
    W = synth_weights(d, seed=0)
    need = {k: s for k, s in sd_shapes.items()
            if ".mixtures.proprio." not in k and (k not in W or tuple(W[k].shape) != tuple(s))}
    assert need and all("lora_" in k for k in need), sorted(k for k in need if "lora_" not in k)
    for k, v in synth_state_dict(need, 0).items():
        W[k] = torch.from_numpy(v)
    for k in sd_shapes:
        if ".mixtures.proprio." in k:
            W[k] = W[k.replace(".mixtures.proprio.", ".mixtures.action.")]
    for k in need:
        if k.endswith("lora_B"):
            assert float(W[k].abs().max()) > 0.0, f"{k}: synthetic lora_B is zero"
    return {k: W[k] for k in sd_shapes}


def run(d, bsz, dtype, W, inp, gnames):
    model = build_reference(d)
    model.load_state_dict(W, strict=True)
    model.to(dtype)
    model.train()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    ids = torch.from_numpy(inp["input_ids"])
    am = torch.from_numpy(inp["attention_mask"])
    mask, vpos, ppos, apos = model.build_causal_mask_and_position_ids(am, dtype)
    orig_randn_like, orig_randn = torch.randn_like, torch.randn
    out = {}
    try:
        x0 = t(inp["x0"])
        torch.randn_like = lambda *a, **k: x0.clone()
        loss = model(input_ids=ids, pixel_values=t(inp["pixel_values"]), causal_mask=mask, vlm_position_ids=vpos,
                     proprio_position_ids=ppos, action_position_ids=apos, proprios=t(inp["proprios"]),
                     actions=t(inp["actions"]), t=t(inp["t"]))
        loss.backward()
        out["loss"] = np.float64(loss.detach().double().item())
        named = dict(model.named_parameters())
        for n in gnames:
            g = named[n].grad
            if g is None:
                out["gradnorm/" + n] = np.float64(-1.0)
                continue
            pr = probe(n, g, N_SAMPLE)
            out["gradnorm/" + n] = np.float64(pr["norm"])
            out["gsamp/" + n] = pr["sample"].numpy()
            out["gproj/" + n] = pr["proj"].numpy()
        model.zero_grad(set_to_none=True)
        noise = t(inp["noise"])
        model.eval()  # LoRALinear.train(False): W += B A
        itp, amask = model.split_full_mask_into_submasks(mask)
        kw = dict(input_ids=ids, pixel_values=t(inp["pixel_values"]), vlm_position_ids=vpos,
                  proprio_position_ids=ppos, action_position_ids=apos, proprios=t(inp["proprios"]),
                  image_text_proprio_mask=itp, action_mask=amask)
        with torch.inference_mode():
            torch.randn = lambda *a, **k: noise.clone()
            cv = model.final_action_clip_value
            model.final_action_clip_value = None
            out["actions_unclipped"] = model.infer_action(**kw).float().numpy()
            model.final_action_clip_value = cv
            out["actions_clipped"] = model.infer_action(**kw).float().numpy()
    finally:
        torch.randn_like, torch.randn = orig_randn_like, orig_randn
    return out


def make(d=TINY_DIMS, bsz=3):
    install_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    meta = build_reference(d, meta=True)
    sd_shapes = {k: tuple(v.shape) for k, v in meta.state_dict().items()}
    gnames = [n for n, _ in meta.named_parameters()]
    trainable = [n for n, p in meta.named_parameters() if p.requires_grad]
    lora_train = [n for n in trainable if "lora_" in n]
    assert lora_train, "the reference built no trainable adapter"
    W = lora_weights(d, sd_shapes)
    inp = synth_inputs(d, bsz, seed=0, ragged=True)
    res = {}
    for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        print(f"[lora] reference run {tag} ...", flush=True)
        for k, v in run(d, bsz, dt, W, inp, gnames).items():
            res[f"{tag}/{k}"] = v
    worst = (0.0, None)
    for n in gnames:
        a, b = res.get(f"bf16/gsamp/{n}"), res.get(f"fp32/gsamp/{n}")
        if a is None or b is None:
            continue
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        nb = np.linalg.norm(b64)
        res[f"bf16/grel/{n}"] = np.float64(np.linalg.norm(a64 - b64) / max(nb, 1e-30))
        res[f"bf16/gcos/{n}"] = np.float64(a64 @ b64 / max(np.linalg.norm(a64) * nb, 1e-30))
        del res[f"bf16/gsamp/{n}"]
    zero_ok = []
    for n in lora_train:
        # conditions of the fixture, not measurements.  The last vlm layer's q_proj adapter is trainable but its
        # queries feed nothing (the reference skips the vlm post-attention block there): its gradient is exactly 0.
        if float(res[f"fp32/gradnorm/{n}"]) == 0.0:
            zero_ok.append(n)
            continue
        assert float(res[f"fp32/gradnorm/{n}"]) > 0.0, f"{n}: no fp32 gradient"
        assert res[f"bf16/grel/{n}"] <= 1.0, (n, res[f"bf16/grel/{n}"])
        if res[f"bf16/grel/{n}"] > worst[0]:
            worst = (float(res[f"bf16/grel/{n}"]), n)
    last = d["n_layers"] - 1
    assert all(f"vlm.layers.{last}.self_attn.q_proj." in n for n in zero_ok), zero_ok
    print(f"[lora] {len(lora_train)} trainable adapters, worst bf16 grel {worst}; exactly-zero gradients: {zero_ok}")
    for k in ("input_ids", "attention_mask", "t"):
        res["in/" + k] = inp[k]
    res["grad_names"] = np.array(gnames)
    res["trainable"] = np.array(trainable)
    res["sd_names"] = np.array(list(sd_shapes))
    res["sd_shapes"] = np.array([",".join(map(str, s)) for s in sd_shapes.values()])
    res["bsz"] = np.int64(bsz)
    res["n_sample"] = np.int64(N_SAMPLE)
    res["rank"] = np.int64(RANK)
    path = os.path.join(ROOT, "tests", "golden", "lora.npz")
    np.savez_compressed(path, **res)
    a32, a16 = res["fp32/actions_unclipped"], res["bf16/actions_unclipped"]
    print("wrote", path, os.path.getsize(path), "bytes; loss fp32", res["fp32/loss"], "bf16", res["bf16/loss"],
          "actions |a| max", np.abs(a32).max(), "bf16 dev mean/max", np.abs(a16 - a32).mean(), np.abs(a16 - a32).max())


if __name__ == "__main__":
    make()
