"""Action/time encoders and the adaLN modules (vla/modules.py:9-119) as parameter containers.

SinusoidalPosEmb -> pz_time_embed.  Default (mode 0): fp32 t and fp32 frequencies
= the reference module in fp32 (the fp32 oracle's semantics).  The reference in a
bf16 model computes it in bf16 (t cast to bf16 at train.py:311, ``arange`` in t.dtype
so odd indices above 256 round, every op rounded): that arithmetic is mode 1, selected
with the config key ``time_embed_bf16_reference: true``.  Measured size of the
difference (reference fp32 vs reference bf16, 1024 wide, tests/golden/time_embed.npz):
max |d| 5.3e-3, mean 2.3-4.6e-4; tests/test_kernels_gpu.py pins both modes.  ActionEncoder -> pz_gemm_small (K=7) +
pz_concat_time + MFMA GEMM with SiLU epilogue + MFMA GEMM; with ``time_cond=False`` (the adaLN expert) there
is no time concat and linear_2 is width -> width.

AdaptiveRMSNorm / AdaptiveLayerscale (``action_expert_adaptive_mode: adaLN | adaLN-Zero``) keep the reference's
attribute names, so state_dict keys match: ``to_gamma.0.{weight,bias}``, ``to_beta.weight``,
``to_adaln_zero_gamma.{weight,bias}``.  The native engine computes every layer's modulation rows with one GEMM of
the time embedding against the adjacent weights and applies them in pz_adaln_fwd (csrc/pz_adaln.hip).
"""

from __future__ import annotations

from torch import nn


class SinusoidalPosEmb(nn.Module):
    def __init__(self, dim: int, max_period: float = 10000.0):
        super().__init__()
        self.half_dim = dim // 2
        self.max_period = float(max_period)


class ActionEncoder(nn.Module):
    def __init__(self, action_dim: int, width: int, time_cond: bool = False):
        super().__init__()
        self.linear_1 = nn.Linear(action_dim, width)
        self.linear_2 = nn.Linear(2 * width if time_cond else width, width)
        self.nonlinearity = nn.SiLU()
        self.linear_3 = nn.Linear(width, width)
        self.time_cond = time_cond


class AdaptiveRMSNorm(nn.Module):
    """y = x * rsqrt(mean(x^2) + eps) * sigmoid(to_gamma(cond)) + to_beta(cond)  (vla/modules.py:78-99)"""

    def __init__(self, dim: int, dim_cond: int, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.to_gamma = nn.Sequential(nn.Linear(dim_cond, dim), nn.Sigmoid())
        self.to_beta = nn.Linear(dim_cond, dim, bias=False)


class AdaptiveLayerscale(nn.Module):
    """y = x * sigmoid(to_adaln_zero_gamma(cond)); weight 0, bias -2 at init  (vla/modules.py:102-119)"""

    def __init__(self, dim: int, dim_cond: int, adaln_zero_bias_init_value: float = -2.0):
        super().__init__()
        self.adaln_zero_bias_init_value = float(adaln_zero_bias_init_value)
        self.to_adaln_zero_gamma = nn.Linear(dim_cond, dim)
