"""Per-expert Gemma-layout decoder layers (mixture.py:23-242): parameter containers.

``Mixture`` / ``MixtureDecoderLayer`` / ``MixtureAttention`` keep the
reference attribute names (q/k/v/o_proj, mlp.{gate,up,down}_proj,
input_layernorm, post_attention_layernorm, norm) so state_dict keys match.
The arena lays q|k|v and gate|up out adjacently; the native engine runs each
layer as: RMSNorm -> fused QKV MFMA GEMM -> RoPE/split into the joint token
buffers -> joint attention -> o_proj GEMM (+residual epilogue) -> RMSNorm ->
fused gate|up GEMM with GeGLU epilogue -> down GEMM (+residual epilogue).
With ``adaptive_mode: adaLN | adaLN-Zero`` (the time-conditioned action expert, mixture.py:31-44,89-109) the
three RMSNorms of the mixture are ``AdaptiveRMSNorm`` and, for adaLN-Zero, each layer carries the two
``AdaptiveLayerscale`` gates; the engine then runs pz_adaln_fwd at those sites (csrc/pz_adaln.hip).
"""

from __future__ import annotations

from torch import nn

from src.model.lora import lora_rank, make_linear
from src.model.paligemma.modules import GemmaMLP, GemmaRMSNorm, GemmaRotaryEmbedding
from src.model.vla.modules import AdaptiveLayerscale, AdaptiveRMSNorm
from src.utils.config import cfg_get

ADAPTIVE_MODES = ("adaLN", "adaLN-Zero")


def _adaptive_mode(config):
    mode = cfg_get(config, "adaptive_mode", None)
    if mode and mode not in ADAPTIVE_MODES:
        raise ValueError(f"adaptive_mode must be one of {ADAPTIVE_MODES} or null, got {mode!r}")
    return mode or None


class Mixture(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.layers = nn.ModuleList([MixtureDecoderLayer(config) for _ in range(cfg_get(config, "num_hidden_layers"))])
        self.adaptive_mode = None
        if cfg_get(config, "use_final_norm", False):
            self.adaptive_mode = _adaptive_mode(config)
            hid, eps = cfg_get(config, "hidden_size"), float(cfg_get(config, "rms_norm_eps", 1e-6))
            if self.adaptive_mode:
                self.norm = AdaptiveRMSNorm(hid, cfg_get(config, "time_hidden_size"), eps=eps)
            else:
                self.norm = GemmaRMSNorm(hid, eps=eps)

    @property
    def head_dim(self) -> int:
        return self.layers[0].self_attn.head_dim


class MixtureDecoderLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self_attn = MixtureAttention(config)
        self.mlp = GemmaMLP(config, use_quantize=cfg_get(config, "use_quantize", False),
                            use_lora=cfg_get(config, "use_lora", False))
        self.adaptive_mode = _adaptive_mode(config)
        hid, eps = cfg_get(config, "hidden_size"), float(cfg_get(config, "rms_norm_eps", 1e-6))
        if self.adaptive_mode:
            tH = cfg_get(config, "time_hidden_size")
            self.input_layernorm = AdaptiveRMSNorm(hid, tH, eps=eps)
            self.post_attention_layernorm = AdaptiveRMSNorm(hid, tH, eps=eps)
            if self.adaptive_mode == "adaLN-Zero":
                self.post_adaptive_scale = AdaptiveLayerscale(hid, tH)
                self.final_adaptive_scale = AdaptiveLayerscale(hid, tH)
        else:
            self.input_layernorm = GemmaRMSNorm(hid, eps=eps)
            self.post_attention_layernorm = GemmaRMSNorm(hid, eps=eps)


class MixtureAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.num_heads = cfg_get(config, "num_attention_heads")
        self.head_dim = cfg_get(config, "head_dim")
        self.num_key_value_heads = cfg_get(config, "num_key_value_heads")
        self.num_key_value_groups = self.num_heads // self.num_key_value_heads
        hid = cfg_get(config, "hidden_size")
        bias = bool(cfg_get(config, "attention_bias", False))
        if bias:
            raise NotImplementedError("attention_bias=True is not used by Pi0 (bridge.yaml:179)")
        r = lora_rank(config, cfg_get(config, "use_quantize", False), cfg_get(config, "use_lora", False))
        self.q_proj = make_linear(hid, self.num_heads * self.head_dim, r, bias=False)
        self.k_proj = make_linear(hid, self.num_key_value_heads * self.head_dim, r, bias=False)
        self.v_proj = make_linear(hid, self.num_key_value_heads * self.head_dim, r, bias=False)
        self.o_proj = make_linear(self.num_heads * self.head_dim, hid, r, bias=False)
        self.rotary_emb = GemmaRotaryEmbedding(self.head_dim, base=cfg_get(config, "rope_theta", 10000.0))
