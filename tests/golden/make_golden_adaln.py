"""Golden fixtures of the adaLN / adaLN-Zero action expert, from the REFERENCE itself (build container only).

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_adaln.py [adaLN|adaLN-Zero|all]

Same recipe as make_golden.py (its stubs, config and gradient probes) at TINY_DIMS, B=3, ragged, fp32 + bf16,
with ``action_expert_adaptive_mode`` set in every copy of the config the reference reads
(``cfg.action_expert_adaptive_mode``, ``cfg.mixture.{proprio,action}.adaptive_mode`` and the deep copy under
``cfg.joint.config``).  Weights: oracle.synth by name -- synth_weights for the tensors whose shape the mode
leaves alone, synth_state_dict for the new / reshaped ones -- so nothing but outputs is stored.

Writes tests/golden/adaln.npz and tests/golden/adaln_zero.npz with tiny.npz's entries (loss, gradient probes of
EVERY named parameter, the reference's bf16-vs-fp32 grel / gcos, grad_names, in/*) plus
  * ``actions_naive_unclipped`` / ``actions_naive_clipped`` from infer_action_naive;
  * ``sd_names`` / ``sd_shapes``: the reference state_dict, name -> shape;
  * ``cached_infer_raises``: the reference's cached infer_action raises in this mode (its prefill runs the
    proprio mixture without the time condition); asserted here.
Also asserted: no adaLN parameter's reference bf16 gradient deviates by more than 100 % (the "noise-only"
branch of check_grads_probe must stay reserved for exactly-zero gradients).
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

FIXTURE = {"adaLN": "adaln", "adaLN-Zero": "adaln_zero"}
ADALN_KEYS = ("to_gamma", "to_beta", "to_adaln_zero_gamma")
N_SAMPLE = 2048  # gradient samples per tensor (b16.npz's count): ~120 probed tensors stay under 1 MiB per fixture


def adaptive_cfg(d, mode):
    """ref_cfg with the adaptive mode in every copy the reference reads"""
    cfg = ref_cfg(d)
    cfg.action_expert_adaptive_mode = mode
    cfg.joint.config.action_expert_adaptive_mode = mode
    for mixes in (cfg.mixture, cfg.joint.config.mixture):
        for k in ("proprio", "action"):
            mixes[k].adaptive_mode = mode
    return cfg


def build_reference(d, mode, meta=False):
    from src.model.vla import pizero as pz

    torch.manual_seed(0)
    if meta:
        with torch.device("meta"):
            model = pz.PiZero(adaptive_cfg(d, mode))
    else:
        model = pz.PiZero(adaptive_cfg(d, mode))
    model.tie_action_proprio_weights()
    model.freeze_unused_weights()
    return model


def adaptive_weights(d, sd_shapes):
    """name -> fp32 tensor for the reference state_dict; proprio keys alias the action tensors (tied)"""
    W = synth_weights(d, seed=0)
    need = {k: s for k, s in sd_shapes.items()
            if ".mixtures.proprio." not in k and (k not in W or tuple(W[k].shape) != tuple(s))}
    for k, v in synth_state_dict(need, 0).items():
        W[k] = torch.from_numpy(v)
    for k in sd_shapes:
        if ".mixtures.proprio." in k:
            W[k] = W[k.replace(".mixtures.proprio.", ".mixtures.action.")]
    return {k: W[k] for k in sd_shapes}


def run(d, mode, bsz, dtype, W, inp, gnames):
    model = build_reference(d, mode)
    model.load_state_dict(W, strict=True)
    model.to(dtype)
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
            if any(k in n for k in ADALN_KEYS):
                assert float(g.double().norm()) > 0.0, f"{n}: the reference gives no gradient signal"
            pr = probe(n, g, N_SAMPLE)
            out["gradnorm/" + n] = np.float64(pr["norm"])
            out["gsamp/" + n] = pr["sample"].numpy()
            out["gproj/" + n] = pr["proj"].numpy()
        model.zero_grad(set_to_none=True)
        noise = t(inp["noise"])
        model.eval()
        itp, amask = model.split_full_mask_into_submasks(mask)
        kw = dict(input_ids=ids, pixel_values=t(inp["pixel_values"]), vlm_position_ids=vpos,
                  proprio_position_ids=ppos, action_position_ids=apos, proprios=t(inp["proprios"]))
        with torch.inference_mode():
            torch.randn = lambda *a, **k: noise.clone()
            cv = model.final_action_clip_value
            model.final_action_clip_value = None
            out["actions_naive_unclipped"] = model.infer_action_naive(causal_mask=mask, **kw).float().numpy()
            model.final_action_clip_value = cv
            out["actions_naive_clipped"] = model.infer_action_naive(causal_mask=mask, **kw).float().numpy()
            raised = False
            try:
                model.infer_action(image_text_proprio_mask=itp, action_mask=amask, **kw)
            except AttributeError as e:
                raised = "ndim" in str(e)
            assert raised, "the reference's cached infer_action was expected to raise in an adaptive mode"
            out["cached_infer_raises"] = np.bool_(raised)
    finally:
        torch.randn_like, torch.randn = orig_randn_like, orig_randn
    return out


def make(mode, d=TINY_DIMS, bsz=3):
    install_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    meta = build_reference(d, mode, meta=True)
    sd_shapes = {k: tuple(v.shape) for k, v in meta.state_dict().items()}
    gnames = [n for n, _ in meta.named_parameters()]
    new = [n for n in gnames if any(k in n for k in ADALN_KEYS)]
    assert new, "the reference built no adaptive parameter"
    W = adaptive_weights(d, sd_shapes)
    inp = synth_inputs(d, bsz, seed=0, ragged=True)
    res = {}
    for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        print(f"[{mode}] reference run {tag} ...", flush=True)
        for k, v in run(d, mode, bsz, dt, W, inp, gnames).items():
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
        if n in new:
            # a condition of the fixture, not a measurement: the noise-only branch of check_grads_probe
            # (bf16/grel > 1) is for exactly-zero gradients only
            assert res[f"bf16/grel/{n}"] <= 1.0, (n, res[f"bf16/grel/{n}"])
            if res[f"bf16/grel/{n}"] > worst[0]:
                worst = (float(res[f"bf16/grel/{n}"]), n)
    noise_only = [n for n in gnames if float(res.get(f"bf16/grel/{n}", 0.0)) > 1.0]
    print(f"[{mode}] worst adaLN bf16 grel {worst}; noise-only tensors: {noise_only}")
    for k in ("input_ids", "attention_mask", "t"):
        res["in/" + k] = inp[k]
    res["grad_names"] = np.array(gnames)
    res["sd_names"] = np.array(list(sd_shapes))
    res["sd_shapes"] = np.array([",".join(map(str, s)) for s in sd_shapes.values()])
    res["bsz"] = np.int64(bsz)
    res["n_sample"] = np.int64(N_SAMPLE)
    path = os.path.join(ROOT, "tests", "golden", FIXTURE[mode] + ".npz")
    np.savez_compressed(path, **res)
    a32, a16 = res["fp32/actions_naive_unclipped"], res["bf16/actions_naive_unclipped"]
    print("wrote", path, "loss fp32", res["fp32/loss"], "bf16", res["bf16/loss"], "actions |a| max",
          np.abs(a32).max(), "bf16 dev mean/max", np.abs(a16 - a32).mean(), np.abs(a16 - a32).max())


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for mode in FIXTURE:
        if which in (mode, "all"):
            make(mode)
