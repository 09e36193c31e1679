"""Shared pieces of the QLoRA tests (quantize: True)."""

from __future__ import annotations

import numpy as np
import torch

from tests import quant4_ref as R
from tests.golden.make_golden import ref_cfg
from tests.golden.make_golden_lora import lora_cfg


def qlora_cfg(d, qtype=None, lora=True):
    """lora_cfg (rank 8) or ref_cfg with quantize switched on in every copy the reference's config derives from it"""
    cfg = lora_cfg(d) if lora else ref_cfg(d)
    cfg.vision.use_quantize = True
    cfg.vision_projector.use_quantize = True
    for mixes in (cfg.mixture, cfg.joint.config.mixture):
        mixes["vlm"].use_quantize = True
    if qtype is not None:
        cfg.quantize_type = qtype
    return cfg


def bits_of(t: torch.Tensor) -> np.ndarray:
    """bf16 tensor -> uint16 bit patterns (flat, host)"""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def tensor_of(bits: np.ndarray, shape, device) -> torch.Tensor:
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).reshape(shape).to(device)


def ref_roundtrip_(model, names, qtype):
    """overwrite the bf16 weights ``names`` of ``model`` with the restatement's dequant(quant(W)); returns the
    restatement's quantised states by name"""
    out = {}
    for n in names:
        v = model._arena.view(n)
        q = R.quantize(bits_of(v), qtype)
        out[n] = q
        w = R.dequantize(q["packed"], q["absmax"], q["nested_absmax"], q["offset"], q["qmap"], qtype, q["n"])
        v.copy_(tensor_of(w, v.shape, v.device))
    return out
