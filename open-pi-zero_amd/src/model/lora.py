"""LoRA adapters as parameter containers (reference src/model/lora.py:141-211).

``LoRALinear`` keeps the reference's parameter names and registration order (weight, bias, lora_A [r, in],
lora_B [out, r]) so state_dict keys and shapes match; ``y = x W^T (+ bias) + s (x A^T) B^T`` with
``s = lora_scaling = 1``.  Nothing is computed here: the owning ``PiZero`` packs the adapters into its arena and
the native engine adds the adapter term inside the GEMM (pz_gemm's rank extension), computes the adapter
gradients with pz_lora_wgrad and runs inference on merged weights (pizero_native.engine).

``quantize: True`` (the reference's Linear4bit / LoRALinear4bit, QLoRA) builds the same containers: the base weight
is constructed and loaded in bf16 and ``PiZero.quantize_base_()`` packs it to 4 bits afterwards.

Out of scope, refused with the config key in the message: ``lora_dropout > 0``.
"""

from __future__ import annotations

import torch
from torch import nn

from src.utils.config import cfg_get

LORA_SCALING = 1.0  # lora.py:155 (lora_scaling), never overridden by the reference's configs


class LoRALinear(nn.Linear):
    def __init__(self, in_features: int, out_features: int, r: int, bias: bool = True):
        super().__init__(in_features, out_features, bias=bias)
        self.r = int(r)
        self.scaling = LORA_SCALING
        self.lora_A = nn.Parameter(torch.empty(self.r, in_features))
        self.lora_B = nn.Parameter(torch.empty(out_features, self.r))
        self.weight.requires_grad = False  # lora.py:169; the bias stays trainable until freeze_non_lora_weights_in_vlm


def lora_rank(config, use_quantize: bool, use_lora: bool) -> int:
    """0 without LoRA, else config.lora.r; refuses lora_dropout > 0 by name.  use_quantize changes nothing here: the
    4-bit packing is PiZero's (quantize_base_), which also refuses a VLM quantised only in part."""
    if not use_lora:
        return 0
    r = int(cfg_get(config, "lora.r"))
    dropout = float(cfg_get(config, "lora.dropout", 0.0) or 0.0)
    if dropout > 0.0:
        raise NotImplementedError(f"lora_dropout = {dropout} (lora.dropout > 0) is not supported; set lora_dropout: 0.0")
    if r < 8 or r % 8 or r > 128:
        raise ValueError(f"lora_r = {r}: the native path takes ranks 8..128 in multiples of 8")
    return r


def make_linear(in_features: int, out_features: int, r: int, bias: bool = True) -> nn.Linear:
    return LoRALinear(in_features, out_features, r, bias=bias) if r else nn.Linear(in_features, out_features, bias=bias)
