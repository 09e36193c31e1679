"""Native layer executor for the Pi0 hot path (SigLIP + joint model, fwd/bwd/infer).

The executor walks the model with HIP kernels from libpizero_hip.so only; it
never calls torch math on the hot path (torch provides device memory and the
current stream).  Layout decisions (MI355X-first):

* residual streams are bf16 row-major ``[tokens, hidden]`` per weight group:
  the VLM group (image+text prefix, Gemma weights) and the action-expert group
  (proprio + action rows, shared weights after ``tie_action_proprio_weights``);
  every Linear is one MFMA GEMM on that stream (q|k|v and gate|up fused);
* the joint attention of the mixture-of-transformers (joint_model.py:130-304)
  gathers all groups' post-RoPE Q/K/V into joint token buffers
  ``Q[B, L, nh*hd]``, ``K/V[B, Lp, hd]`` (MQA: one KV head, so the 8 query
  heads are stacked as rows and no ``repeat_kv`` copy exists), then runs
  S = Q K^T and O = P V as per-sample batched MFMA GEMMs around a softmax
  kernel that applies the Gemma soft-cap and generates the block-causal mask
  arithmetically from per-sample prefix counts;
* backward reuses the same GEMM kernel in its k-strided layouts (dgrad /
  wgrad / attention products), writes parameter gradients straight into the
  flat gradient arena, and reports each finished layer to an optional hook
  (used by the data-parallel wrapper to start RCCL all-reduces of finished
  gradient buckets while the backward continues).
"""

from __future__ import annotations

import contextlib
import functools
import math
import os
import weakref
from dataclasses import dataclass

import torch

from . import ops
from .ops import PZ_EPI_DGEGLU, PZ_EPI_GEGLU, PZ_EPI_GELU, PZ_EPI_NONE, PZ_EPI_SILU

BF16 = torch.bfloat16
F32 = torch.float32


def _cfg(cfg, key, default=None):
    from src.utils.config import cfg_get

    return cfg_get(cfg, key, default)


@dataclass
class Dims:
    P: int
    C: int
    H: int
    A: int
    Pd: int
    vocab: int
    image_token: int
    pad_token: int
    img: int
    ps: int
    n_img: int  # image tokens per sample (= img_tok x n_images)
    vH: int
    vI: int
    vL: int
    vheads: int
    ln_eps: float
    proj: int
    nL: int
    nh: int
    nkv: int
    hd: int
    rms_eps: float
    gH: int
    gI: int
    g_theta: float
    aH: int
    aI: int
    a_theta: float
    p_theta: float
    tmax: float
    sig_min: float
    steps: int
    clip: float | None
    time_bf16: bool = False  # pz_time_embed mode 1: the reference's bf16 arithmetic (see modules.py)
    n_images: int = 1  # images per sample (C5, the Pi0-paper shape: 3)
    ada: str | None = None  # action_expert_adaptive_mode: None | "adaLN" | "adaLN-Zero"
    tH: int = 0  # time_hidden_size: width of the time condition of the adaLN expert

    @property
    def img_tok(self):
        """SigLIP tokens per image"""
        return (self.img // self.ps) ** 2

    @staticmethod
    def from_cfg(cfg):
        v = _cfg(cfg, "vision.config")
        j = _cfg(cfg, "joint.config")
        mix = _cfg(cfg, "mixture") or _cfg(j, "mixture")
        img = int(_cfg(v, "image_size"))
        ps = int(_cfg(v, "patch_size"))
        clip = _cfg(cfg, "final_action_clip_value", None)
        return Dims(
            P=int(_cfg(cfg, "max_image_text_tokens", _cfg(cfg, "max_seq_len"))), C=int(_cfg(cfg, "cond_steps")),
            H=int(_cfg(cfg, "horizon_steps")), A=int(_cfg(cfg, "action_dim")), Pd=int(_cfg(cfg, "proprio_dim")),
            vocab=int(_cfg(cfg, "vocab_size")), image_token=int(_cfg(cfg, "image_token_index")),
            pad_token=int(_cfg(cfg, "pad_token_id")), img=img, ps=ps,
            n_img=(img // ps) ** 2 * int(_cfg(cfg, "num_images", 1)),
            vH=int(_cfg(v, "hidden_size")), vI=int(_cfg(v, "intermediate_size")),
            vL=int(_cfg(v, "num_hidden_layers")), vheads=int(_cfg(v, "num_attention_heads")),
            ln_eps=float(_cfg(v, "layer_norm_eps", 1e-6)),
            proj=int(_cfg(cfg, "vision_projector.config.vision_config.projection_dim")),
            nL=int(_cfg(j, "num_hidden_layers")), nh=int(_cfg(j, "num_attention_heads")),
            nkv=int(_cfg(j, "num_key_value_heads")), hd=int(_cfg(j, "head_dim")),
            rms_eps=float(_cfg(j, "rms_norm_eps", 1e-6)),
            gH=int(_cfg(mix, "vlm.hidden_size")), gI=int(_cfg(mix, "vlm.intermediate_size")),
            g_theta=float(_cfg(mix, "vlm.rope_theta", 10000.0)),
            aH=int(_cfg(mix, "action.hidden_size")), aI=int(_cfg(mix, "action.intermediate_size")),
            a_theta=float(_cfg(mix, "action.rope_theta", 10000.0)),
            p_theta=float(_cfg(mix, "proprio.rope_theta", _cfg(mix, "action.rope_theta", 10000.0))),
            tmax=float(_cfg(cfg, "time_max_period", 10000.0)), sig_min=float(_cfg(cfg, "flow_sig_min", 0.001)),
            steps=int(_cfg(cfg, "num_inference_steps")), clip=None if clip is None else float(clip),
            time_bf16=bool(_cfg(cfg, "time_embed_bf16_reference", False)),
            n_images=int(_cfg(cfg, "num_images", 1)),
            ada=_cfg(cfg, "action_expert_adaptive_mode", None) or None,
            tH=int(_cfg(cfg, "time_hidden_size", 0) or 0),
        )

    @property
    def L(self):
        return self.P + self.C + self.H

    @property
    def Lp(self):
        return (self.L + 7) // 8 * 8

    @property
    def kcols(self):
        return (3 * self.ps * self.ps + 31) // 32 * 32


def check_finite(where, **tensors):
    """Synchronise the device and raise FloatingPointError if a floating-point tensor holds NaN / Inf, naming the
    stage, the tensor and the native launches since the previous check (PZ_CHECK_FINITE debug instrument)."""
    from ._lib import recent_launches

    torch.cuda.synchronize()
    for k, t in tensors.items():
        if isinstance(t, dict):
            for k2, t2 in t.items():
                check_finite(where, **{f"{k}[{k2}]": t2})
            continue
        if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.numel() == 0:
            continue
        if not bool(torch.isfinite(t).all()):
            bad = int((~torch.isfinite(t)).sum())
            launches = recent_launches()
            raise FloatingPointError(f"PZ_CHECK_FINITE: {where}: {k} {tuple(t.shape)} {t.dtype} has {bad} non-finite "
                                     f"values; native launches since the previous check ({len(launches)}): "
                                     f"{launches[-40:]}")
    recent_launches()


class _Token:
    """Lifetime marker of the forward state that borrows the engine's joint K/V buffers."""


class GeneralMask:
    """A caller attention mask that is NOT the Pi0 block pattern (pizero.py:271-306).

    The reference adds any additive mask to the soft-capped logits (joint_model.py:261-287); such a
    mask is applied here by the GEMM + softmax path (pz_attn_softmax mask_mode 2, fp32 additive),
    never by the fused kernels, which generate the block mask from per-sample prefix counts.
    ``full``: fp32 [B, L, L] (training); ``itp``: fp32 [B, P+C, P+C] and ``act``: fp32 [B, H, L]
    (inference, pizero.py:326-336 split)."""

    def __init__(self, full=None, itp=None, act=None):
        self.full, self.itp, self.act = full, itp, act


def _mask_kw(d, cnt, which):
    """pz_attn_softmax mask arguments: block mask from cnt, or the general additive mask."""
    if isinstance(cnt, GeneralMask):
        m = getattr(cnt, which)
        return dict(mask_mode=2, mask=m, ldm=m.shape[2], mask_bstride=m.shape[1] * m.shape[2])
    return dict(mask_mode=1, cnt=cnt, prefix=d.P, cond=d.C)


FP8_ADAPTIVE_MSG = ("fp8 inference is not available with action_expert_adaptive_mode (adaLN / adaLN-Zero): the fp8 "
                    "norm-to-codes kernels are Gemma-RMSNorm specific and the reference has no fp8 path")
PREFIX_ADAPTIVE_MSG = ("an action prefix (action_prefix_max_delay / prefix_len, DESIGN 7f) is not available with "
                       "action_expert_adaptive_mode (adaLN / adaLN-Zero): the adaLN condition is one time per sample, "
                       "and a prefix row needs its own (time 1)")
DRAWS_FROZEN_MSG = ("flow_samples_per_observation > 1 (several flow draws per observation, DESIGN 7k) needs the "
                    "frozen-VLM pass: nothing trainable in the VLM (train_vlm: False, no trainable adapters) and the "
                    "Pi0 block mask, because the draws share one forward-only VLM prefill and the joint attention "
                    "kernels would need the VLM rows' dK / dV from every draw")


# inference-time guidance toward the previous chunk: what it does not combine with, by config key
GUIDE_ADAPTIVE_MSG = ("action guidance (action_guidance_beta / overlap, DESIGN 7i) is not available with "
                      "action_expert_adaptive_mode (adaLN / adaLN-Zero): the guided step differentiates the plain "
                      "expert's saved activations only")
GUIDE_FP8_MSG = ("action guidance (action_guidance_beta / overlap, DESIGN 7i) is not available with fp8 inference "
                 "(prepare_fp8 / infer_fp8): the vector-Jacobian product runs on the bf16 weights")
GUIDE_MASK_MSG = ("action guidance (action_guidance_beta / overlap, DESIGN 7i) needs the Pi0 block mask: a GeneralMask "
                  "is not supported")
GUIDE_PREFIX_MSG = ("action guidance (overlap, DESIGN 7i) and a hard action prefix (prefix_len, DESIGN 7f) do not "
                    "compose: guidance replaces the prefix inside the loop")


class Ada:
    """Time modulation of one adaLN expert group for one forward / denoise step: ``mod`` fp32 [B, nslots * hidden],
    every site's gamma_pre / beta / gate_pre rows (cond @ W^T, biases added by the row kernels), from ONE GEMM of
    the time embedding against the mixture's adjacent conditioning weights (pizero.adaln_slots); ``dmod``: the
    matching per-sample gradient rows, filled by the backward row kernels."""

    def __init__(self, eng, g, cond):
        self.eng, self.D, self.zero = eng, g.hid, eng.d.ada == "adaLN-Zero"
        self.sl = eng.ada_slots(g.prefix[: -len("layers.")])
        self.W = eng.ar.span(self.sl["w"][0], self.sl["w"][-1])
        self.mod = torch.empty(cond.shape[0], self.W.shape[0], device=cond.device, dtype=F32)
        ops.linear(cond, self.W, self.mod)
        self.dmod = None

    def biased(self, layer, site):
        """(first column, bias [hidden]) of a to_gamma / layer-scale gate slot"""
        i = self.sl["slot"][(layer, site)]
        return i * self.D, self.eng.w(self.sl["b"][i])

    def beta(self, layer, site):
        return self.sl["slot"][(layer, site)] * self.D

    def norm_fwd(self, x, layer, site, T, h, rstd=None, y=None, gate=None, xm=None):
        """h = AdaptiveRMSNorm_site(xm), xm = x (+ y * gate); site: "in" | "post" | "" (the final norm)"""
        ops.adaln_fwd(x, self.mod, T, self.eng.d.rms_eps, y=y, gate=None if y is None else self.biased(layer, gate),
                      xm=xm, gamma=self.biased(layer, site + "g"), beta=self.beta(layer, site + "b"), h=h, rstd=rstd)

    def norm_bwd(self, dh, x, rstd, layer, site, T, dx, dres=None):
        return ops.adaln_norm_bwd(dh, x, rstd, self.mod, self.biased(layer, site + "g"), dx, self.dmod,
                                  self.beta(layer, site + "b"), T, dres=dres)

    def weight_grads(self, cond, ws, beta):
        """every conditioning weight gradient from one wgrad GEMM of dmod against the time embedding, every bias
        gradient from one column sum over the biased slots"""
        eng, w, b = self.eng, self.sl["w"], self.sl["b"]
        dm = torch.empty(self.dmod.shape, device=self.dmod.device, dtype=BF16)
        ops.cast_to_bf16(self.dmod, dm)
        if all(eng.rg(n) for n in w):
            ops.linear_wgrad(dm, cond, eng.ar.grad_span(w[0], w[-1]), beta=beta)
        else:
            for i, n in enumerate(w):
                if eng.rg(n):
                    ops.linear_wgrad(dm[:, i * self.D:(i + 1) * self.D], cond, eng.gw(n), beta=beta)
        if all(eng.rg(n) for n in b):
            ops.colsum(dm[:, : len(b) * self.D], eng.ar.grad_span(b[0], b[-1]), ws, beta=beta)
        else:
            for i, n in enumerate(b):
                if eng.rg(n):
                    ops.colsum(dm[:, i * self.D:(i + 1) * self.D], eng.gw(n), ws, beta=beta)


class LoraSite:
    """The LoRA adapters of one Linear site of the training path (reference lora.py:141-211): S projections that
    share their input and are fused along the output columns (q|k|v: 3, gate|up: 2, else 1), rank r each.
      forward   y = x W^T + u B2^T          u = x A^T [M, S r], A = the adjacent lora_A span [S r, in];
                                            B2 [N, S r] = the lora_B blocks packed block-diagonally (S = 1: lora_B)
      backward  dx = dy W + v A             v = dy B2 [M, S r]
                dA_i = s v_i^T x, dB_i = s dy_i^T u_i   (pz_lora_wgrad per projection, column slices of v / u / dy)
    The adapter terms are summed inside the main GEMMs (pz_gemm's rank extension), so the fused RoPE / GeGLU / GELU /
    residual epilogues stay.  The packed B2 is an engine-owned buffer rebuilt when the arena's weight version changes
    (packed operand rather than per-column-segment addressing in the kernel: the extension stays one more K range of
    the same pipeline, and the packing is 2-3 small copies per site and optimizer step)."""

    def __init__(self, eng, wnames):
        self.eng = eng
        self.a = [n[: -len("weight")] + "lora_A" for n in wnames]
        self.b = [n[: -len("weight")] + "lora_B" for n in wnames]
        sl = eng.ar.slots
        self.r = sl[self.a[0]].shape[0]
        self.S = len(wnames)
        self.outs = [sl[n].shape[0] for n in self.b]
        self._b2 = None
        self._b2_ver = None

    def A(self):
        return self.eng.ar.span(self.a[0], self.a[-1])

    def B2(self):
        ar = self.eng.ar
        if self.S == 1:
            return ar.view(self.b[0])
        ver = self.eng.weights_version()
        if self._b2 is None or self._b2_ver != ver or self._b2.device != ar.data.device:
            if self._b2 is None or self._b2.device != ar.data.device:
                self._b2 = torch.zeros(sum(self.outs), self.S * self.r, device=ar.data.device, dtype=ar.data.dtype)
            r0 = 0
            for i, (n, o) in enumerate(zip(self.b, self.outs)):
                self._b2[r0:r0 + o, i * self.r:(i + 1) * self.r].copy_(ar.view(n))
                r0 += o
            self._b2_ver = ver
        return self._b2

    def fwd(self, x):
        """(u, B2): the ``lora=`` operands of the site's forward GEMM; u is kept for the backward"""
        u = torch.empty(x.shape[0], self.S * self.r, device=x.device, dtype=x.dtype)
        ops.linear(x, self.A(), u)
        return u, self.B2()

    def bwd(self, dy):
        """(v, A): the ``lora=`` operands of the site's input-gradient GEMM"""
        v = torch.empty(dy.shape[0], self.S * self.r, device=dy.device, dtype=dy.dtype)
        ops.linear_dgrad(dy, self.B2(), v)
        return v, self.A()

    def grads(self, x, u, dy, v, beta):
        from src.model.lora import LORA_SCALING

        eng, r, c0 = self.eng, self.r, 0
        for i, o in enumerate(self.outs):
            if eng.rg(self.a[i]):
                ops.lora_wgrad(x, v[:, i * r:(i + 1) * r], eng.gw(self.a[i]), alpha=LORA_SCALING, beta=beta)
            if eng.rg(self.b[i]):
                ops.lora_wgrad(dy[:, c0:c0 + o], u[:, i * r:(i + 1) * r], eng.gw(self.b[i]), transposed=True,
                               alpha=LORA_SCALING, beta=beta)
            c0 += o


def _merged_weights(fn):
    """Inference entry point of a LoRA or 4-bit model: refresh the merged shadow weights and read them in place of the
    base"""

    @functools.wraps(fn)
    def wrap(self, *a, **k):
        if not self._shadow_w:
            return fn(self, *a, **k)
        if not torch.cuda.is_current_stream_capturing():
            self.lora_refresh()
        prev, self._infer = self._infer, True
        try:
            return fn(self, *a, **k)
        finally:
            self._infer = prev

    return wrap


class Group:
    """Rows of the joint sequence that share one set of mixture weights."""

    def __init__(self, name, prefix, T, joint_off, hidden, inter, theta, skip_last):
        self.name, self.prefix = name, prefix
        self.T, self.off, self.hid, self.inter, self.theta = T, joint_off, hidden, inter, theta
        self.skip_last = skip_last


class Engine:
    def __init__(self, model):
        self.m = model
        self.d = Dims.from_cfg(model.cfg)
        self._tables = {}
        self._ws = {}
        self._jkv_holder = None
        # joint attention kernel: "gemm" = MFMA GEMMs around the soft-cap/block-mask softmax, "flash" = the
        # fused pz_flash kernels fwd + bwd (no L x L tensors), "probs" = fused forward that exports the
        # bf16 softmax (pz_flash_fwd_probs: no fp32 S, no softmax launch) + the GEMM-path backward
        # ("probs": measured 237.5 vs 235.4 samples/s for "gemm" and 227.5 vs 231.1 for "flash").  The GEMM-path
        # backward takes dS and dQ = dS K from pz_flash_bwd_ds (the exported P, no fp32 dP) where its shape allows.
        self.joint_flash = False
        self.joint_probs = True
        # inference (prefill / denoise) attention: the fused kernel (False: the GEMM path)
        self.infer_flash = True
        # Activation backward of the training MLPs.  SigLIP: plain dgrad GEMM + a vectorised elementwise GELU pass
        # (fused into the dgrad epilogue, which the 8-phase kernel cannot overlap with its main loop, measured 0.7 %
        # fewer samples/s).  Gemma GeGLU: d(gate|up) in the down-proj dgrad epilogue, the faster form since the
        # activations run on the hardware exp / rcp (vlm layer 1.390 vs 1.553 ms, action 24.2 vs 26.0 us with the
        # separate geglu_bwd pass, profiles/r03/dact_ab.log).
        # q|k|v GEMM with the RoPE + Q/K/V scatter in its epilogue (pz_gemm_qkv_rope) where the 8-phase kernel
        # runs, bit-identical to GEMM + pz_qkv_rope_split (which other shapes fall back to)
        self.fuse_qkv_rope = self.d.hd == 256
        # backward of the action-expert group (M = B*(C+H) = 320 rows: latency-bound GEMMs) on a second HIP
        # stream, concurrent with the vlm group's (False: one stream)
        self.expert_stream = True
        # ... and in the forward: measured no faster than backward-only (bench 238.9 vs 239.3 samples/s), and its
        # expert GEMMs then share the CUs with the vlm GeGLU GEMM (the dominant kernel: live roofline 2.32 vs
        # 2.19 ms per launch), so off
        self.expert_stream_fwd = False
        # a model whose VLM has nothing trainable (train_vlm: False) under the block mask: the VLM runs forward-only
        # into the joint K/V buffers and only the expert groups keep activations and run a backward.
        # False: the full joint pass, whose VLM backward then feeds nothing.
        self.vlm_forward_only = True
        # row pitch of SigLIP's MLP activations (fc1 output / pre-activation / their gradient, 4304 wide): rounded up
        # to 64 elements, so every row starts on a 128-B line (8704 B instead of 8608 B).  The GEMMs that stream
        # these rows run 2-8 % faster with bitwise-equal results (profiles/r04/ld_pad_ab.txt); the pad columns are
        # never read (K tails clamp their sources into the row).
        self.sig_pitch = (self.d.vI + 63) // 64 * 64
        self._side = {}
        # PZ_CHECK_FINITE=1 (debug): after every layer / stage of the training forward and backward (and in
        # FusedAdamW.step) synchronise and check the stage's outputs; the first non-finite tensor raises
        # FloatingPointError naming the stage, the tensor and the kernels launched since the previous check
        self.check_finite = os.environ.get("PZ_CHECK_FINITE", "0") == "1"
        # fp8 inference (C5): weight key -> (e4m3 codes, per-tensor scale); built by prepare_fp8()
        # in fp8 mode the prefill's joint attention runs S = Q K^T and P V on the fp8 MFMA (pz_flash_fwd_f8) and the
        # 65..1024-row q|k|v / o projections run W8A8 on the row-slab kernel (activation rows quantised per row)
        self.f8 = None
        self.f8_version = None
        # LoRA (lora: True): adapter sites of the training path, and the merged shadow the inference paths read
        self._lora_sites = {}
        self._lora_w = frozenset(n[: -len("lora_A")] + "weight" for n in self.ar.slots if n.endswith(".lora_A"))
        self._merged = None
        self._merged_ver = None
        self._infer = False
        # 4-bit base weights (quantize: True): the packed store; training dequantises a site's weights into
        # one scratch buffer right before the GEMM that reads them (forward and input gradient), inference reads the
        # shadow, which for these weights is laid out like the arena's side buffer
        self._q4 = model._q4
        self._q4_w = frozenset(self._q4.w) if self._q4 is not None else frozenset()
        self._shadow_w = self._lora_w | self._q4_w
        self._merged_side = None
        self._q4_buf = None
        # the guided denoise step runs the training backward of the expert rows for the input gradient
        # alone: while set, no weight gradient, column sum, norm-weight partial or hook notification is launched
        # (rg() answers False, requires_grad is not touched) and no adapter site is used (the merged weights are read)
        self._dgrad_only = False
        # ... and its few-row input-gradient GEMMs take pz_dgrad_rows where it measured faster (_dgrad_gemm; False:
        # always pz_gemm, the A/B arm)
        self.dgrad_rows = True
        if self.d.nkv != 1:
            raise NotImplementedError("joint attention kernel path assumes MQA (num_key_value_heads=1, bridge.yaml:176)")

    def ada_slots(self, prefix):
        """pizero.adaln_slots of one mixture, built once per engine (every denoise step asks for it)"""
        key = ("ada_slots", prefix)
        sl = self._tables.get(key)
        if sl is None:
            from src.model.vla.pizero import adaln_slots

            sl = self._tables[key] = adaln_slots(prefix, self.d.nL, self.d.ada)
        return sl

    def _chk(self, where, **tensors):
        """PZ_CHECK_FINITE: raise on the first non-finite tensor of this stage (no-op otherwise)"""
        if not self.check_finite or torch.cuda.is_current_stream_capturing():
            return
        check_finite(where, **tensors)

    # ------------------------------------------------------------- weights --
    @property
    def ar(self):
        return self.m._arena

    def w(self, name):
        if name in self._q4_w:
            return self.span(name, name).view(self.ar.slots[name].shape)
        return self.ar.view(name, self._merged if self._infer and name in self._lora_w else None)

    def span(self, first, last):
        if first in self._q4_w:
            return self.ar.span(first, last, self._merged_side) if self._infer else self._q4_dequant(first, last)
        return self.ar.span(first, last, self._merged if self._infer and first in self._lora_w else None)

    def _q4_dequant(self, first, last):
        """The bf16 weights of the adjacent 4-bit slots first..last, dequantised into the scratch buffer by one
        pz_q4_dequant launch: the [rows, in] view Arena.span gives of a bf16 span -- same shape, contiguous, 16-byte
        aligned.  One scratch (sized for the largest fused site) serves every site: a site's GEMM is enqueued before
        the next site's dequantisation on the same stream; only the vlm group reads these weights, and it never runs
        on the side stream (_on), nor do the data-parallel hooks read a weight."""
        ar = self.ar
        names = ar.order[ar.order.index(first): ar.order.index(last) + 1]
        a, z = ar.slots[first], ar.slots[last]
        n = z.offset + z.numel - a.offset
        assert sum(self._q4.w[nm].n for nm in names) == n, f"{first}..{last}: padding inside a 4-bit span"
        if self._q4_buf is None or self._q4_buf.device != ar.data.device:
            most = max(sum(ar.slots[f"{pre}{pr}.weight"].numel for pr in projs)
                       for pre, projs in self.m._vlm_linear_sites())
            self._q4_buf = torch.empty(most, device=ar.data.device, dtype=BF16)
        return self._q4.dequant(names, self._q4_buf).view(n // a.shape[-1], a.shape[-1])

    # --------------------------------------------------------------- LoRA --
    def lora(self, *wnames):
        """LoraSite of the Linear(s) ``wnames`` (fused along N, in column order) or None without adapters"""
        if wnames[0] not in self._lora_w or self._dgrad_only:
            return None
        st = self._lora_sites.get(wnames)
        if st is None:
            st = self._lora_sites[wnames] = LoraSite(self, wnames)
        return st

    def _linear(self, x, names, W, out, train, fp8=True, gemm=ops.linear, **kw):
        """out = x W^T of the Linear site ``names`` (fused along N; W their weights).  Training: ops.linear (``gemm``
        in its place: a q|k|v projection with its RoPE epilogue) + the site's adapter term u B2^T inside the GEMM;
        returns u (None without adapters), which the backward reads.  Inference: self.lin -- fp8 codes (prepare_fp8)
        where ``fp8`` allows them, merged weights, no adapter term."""
        if not train:
            if fp8:
                self.lin(x, names[0], W, out, **kw)
            else:
                ops.linear(x, W, out, **kw)
            return None
        site = self.lora(*names)
        lo = site.fwd(x) if site is not None else None
        gemm(x, W, out, lora=lo, **kw)
        return lo[0] if lo else None

    def _dgrad(self, names, x, u, dy, W, dx, beta, wgrad=None, **kw):
        """dx = dy W of the Linear site ``names`` (input x, saved u): the adapters' v = dy B2 and their gradients,
        then the input-gradient GEMM with v A summed inside.  wgrad: the base weights' gradient launches where they go
        out between the two (the joint q|k|v site)."""
        site = self.lora(*names)
        lo = None
        if site is not None:
            lo = site.bwd(dy)
            site.grads(x, u, dy, lo[0], beta)
        if wgrad is not None:
            wgrad()
        self._dgrad_gemm(dy, W, dx, lora=lo, **kw)

    def _dgrad_gemm(self, dy, W, dx, lora=None, **kw):
        """ops.linear_dgrad; in the guided denoise step (a handful of rows) pz_dgrad_rows where it measured faster and
        takes the call: W [N, K] with N < K (down_proj 1024 -> 4096: 12.3 vs 13.2 us, o_proj 1024 -> 2048: 11.3 vs
        11.6 us at M = 5), not N > K (gate|up 8192 -> 1024: 18.2 vs 16.4 us, q|k|v 2560 -> 1024: 12.5 vs 11.5 us;
        profiles/rtc/rtc_bench.txt); N = K was not measured and stays on pz_gemm"""
        if self._dgrad_only and self.dgrad_rows and lora is None and set(kw) <= {"epi", "aux"} and \
                W.shape[0] < W.shape[1] and ops.linear_dgrad_rows(dy, W, dx, **kw):
            return
        ops.linear_dgrad(dy, W, dx, lora=lora, **kw)

    def lora_refresh(self):
        """Merged inference weights W + s B A of every adapted Linear (the reference merges on eval(), lora.py:186-199)
        in a shadow of the arena: one pz_gemm per Linear, C = s (B A) + resid(W).  The base weights are never written,
        so they come back bit for bit after any train -> infer -> train sequence and state_dict() always holds the
        unmerged tensors.  Rebuilt in place (captured graphs keep their pointers) when the weight version changed.
        Returns True if it rebuilt."""
        if not self._shadow_w:
            return False
        ver = self.weights_version()
        dev = self.ar.data.device
        main = bool(self._lora_w - self._q4_w)  # adapted bf16 weights: their shadow has the arena's layout
        stale = lambda need, buf: need and (buf is None or buf.device != dev)  # noqa: E731
        if self._merged_ver == ver and not stale(main, self._merged) and not stale(self._q4_w, self._merged_side):
            return False
        from src.model.lora import LORA_SCALING

        if stale(main, self._merged):
            self._merged = torch.empty_like(self.ar.data)
        if stale(self._q4_w, self._merged_side):
            # 4-bit base: the shadow is the only bf16 copy of these weights, allocated at the first inference call
            self._merged_side = torch.empty(self.ar.side_total, device=dev, dtype=BF16)
        for wn in sorted(self._shadow_w):
            q4 = wn in self._q4_w
            dst = self.ar.view(wn, self._merged_side if q4 else self._merged)
            if wn not in self._lora_w:  # quantize without adapters: the shadow is dequant(W4)
                self._q4.dequant([wn], dst.view(-1))
                continue
            W = self._q4_dequant(wn, wn).view(dst.shape) if q4 else self.ar.view(wn)  # 4-bit: through the scratch
            A = self.ar.view(wn[: -len("weight")] + "lora_A")
            Bm = self.ar.view(wn[: -len("weight")] + "lora_B")
            out, inn = W.shape
            ops.gemm(out, inn, A.shape[0], Bm, A.shape[0], True, A, inn, False, dst, inn,
                     alpha=LORA_SCALING, resid=W, ld_resid=inn)
        self._merged_ver = ver
        return True

    def gw(self, name):
        return self.ar.grad_view(name)

    def rg(self, name):
        return not self._dgrad_only and self.m._requires_grad(name)

    def qkv_w(self, p):
        return self.span(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight")

    def gu_w(self, p):
        return self.span(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight")

    # ------------------------------------------------------------ fp8 (C5) --
    @_merged_weights
    def prepare_fp8(self):
        """fp8 e4m3 copies (per-tensor scale max|W|/448) of every inference Linear of SigLIP, the vlm
        mixture and the action expert (BASELINE.json configs[4]: fp8 attention / MLP GEMMs).  Prefill
        GEMMs (>= 65 rows) run W8A8 on the fp8 MFMA with per-row activation scales, except the row-slab
        shapes (<= 1024 rows, K <= 2048, <= 4096 columns: q|k|v / o), which run W8A16 like the denoise rows
        (<= 64: codes expanded to bf16 in registers, RMSNorm still fused).  Taken from the
        current weights; the codes carry the arena's weight version (``weights_version``) and every
        inference entry point re-quantises them when the weights changed since (fp8_refresh)."""
        d = self.d
        if d.ada:
            raise NotImplementedError(FP8_ADAPTIVE_MSG)
        self.f8_version = self.weights_version()
        vt = "vision_tower.vision_model.encoder.layers."
        keys = []
        for i in range(d.vL):
            p = f"{vt}{i}."
            keys += [("span", p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight"),
                     ("w", p + "self_attn.out_proj.weight"), ("w", p + "mlp.fc1.weight"), ("w", p + "mlp.fc2.weight")]
        for mix in ("vlm", "action"):
            for l in range(d.nL):
                p = f"joint_model.mixtures.{mix}.layers.{l}."
                keys += [("span", p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight"),
                         ("w", p + "self_attn.o_proj.weight"),
                         ("span", p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"),
                         ("w", p + "mlp.down_proj.weight")]
        f8 = {}
        for k in keys:
            W = self.span(k[1], k[2]) if k[0] == "span" else self.w(k[1])
            sc = ops.fp8_weight_scale(W)
            q = torch.empty(W.shape, device=W.device, dtype=torch.uint8)
            ops.fp8_quant_tensor(W, q, sc)
            f8[k[1]] = (q, sc)
        self.f8 = f8

    def weights_version(self):
        """Version of the weight arena: the shared version counter of arena.data, which torch bumps for
        every in-place write through a parameter view (load_state_dict, load_pretrained_weights,
        ``p.copy_``) and FusedAdamW.step bumps after its raw-pointer kernel writes."""
        return self.ar.data._version

    def fp8_refresh(self):
        """Re-quantise the fp8 weight copies if the weights changed after prepare_fp8 (stale
        e4m3 codes after an optimizer step / checkpoint load).  Returns True if it re-quantised."""
        if self.f8 is None or self.f8_version == self.weights_version():
            return False
        self.prepare_fp8()
        return True

    def lin(self, x, key, W, out, *, bias=None, resid=None, epi=PZ_EPI_NONE, aux=None, norm=None):
        """ops.linear, or its fp8 form when prepare_fp8() holds codes for ``key`` (the weight name; the
        first name of a span): W8A16 for <= 64 rows (norm may stay fused), else per-row quantised
        activations (norm must already be applied) and W8A8."""
        f = self.f8.get(key) if self.f8 else None
        if f is None:
            return ops.linear(x, W, out, bias=bias, resid=resid, epi=epi, aux=aux, norm=norm)
        q, sc = f
        if isinstance(x, tuple):  # (e4m3 codes, row scales) from a fused norm + quantisation (w8a8_in): W8A8
            return ops.linear_fp8(x[0], q, sc, out, bias=bias, resid=resid, epi=epi, aux=aux, x_scale=x[1])
        M, K = x.shape
        if M <= 64:
            if K % 64:  # (SigLIP fc2, K = 4304, never has so few rows in practice)
                return ops.linear(x, W, out, bias=bias, resid=resid, epi=epi, aux=aux, norm=norm)
            return ops.linear_fp8(x, q, sc, out, bias=bias, resid=resid, epi=epi, aux=aux, norm=norm)
        ncols = W.shape[0] // 2 if epi == PZ_EPI_GEGLU else W.shape[0]
        if norm is None and ops.rows_w8a16_ok(M, K, ncols):
            # bf16 rows from a producer that cannot emit codes (the attention output into o_proj): W8A16 on the
            # row-slab kernel -- quantising them costs a launch (~5 us) that the latency-bound W8A8 GEMM does not win
            # back (profiles/r06/c5_fp8_ab.txt)
            return ops.linear_fp8(x, q, sc, out, bias=bias, resid=resid, epi=epi, aux=aux)
        if norm is not None:
            raise ValueError("lin: a fused norm needs <= 64 rows")
        if K % 16 or x.stride(0) % 16:  # W8A8 stages K in 16-code steps (tiny test widths: bf16)
            return ops.linear(x, W, out, bias=bias, resid=resid, epi=epi, aux=aux)
        xq = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
        xs = torch.empty(M, device=x.device, dtype=F32)
        ops.fp8_quant_rows(x, xq, xs)
        return ops.linear_fp8(xq, q, sc, out, bias=bias, resid=resid, epi=epi, aux=aux, x_scale=xs)

    def w8a8_in(self, key, M, K):
        """fp8 mode: True if the Linear ``key`` on M > 64 rows should get its A operand as e4m3 codes from a fused norm
        (pz_rmsnorm_fwd_f8 / pz_layernorm_fwd_f8): W8A8 on the fp8 MFMA (row slab or 8-phase) with no quantisation
        launch"""
        return self.f8 is not None and key in self.f8 and M > 64 and K % 16 == 0

    def norm_codes(self, x, w, eps, b=None):
        """(codes [M, K], row scales [M]) of RMSNorm (b None) / LayerNorm (b given) of x, in one launch"""
        xq = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
        xs = torch.empty(x.shape[0], device=x.device, dtype=F32)
        if b is None:
            ops.rmsnorm_f8(x, w, xq, xs, eps)
        else:
            ops.layernorm_f8(x, w, b, xq, xs, eps)
        return xq, xs

    def rope(self, theta, maxpos=None):
        """fp32 cos|sin table for positions 0..maxpos (default L + 8: every training / action position);
        text generation asks for longer tables (a new, power-of-two sized table: graphs captured on the
        default one keep it)"""
        dev = self.ar.data.device
        base = self.d.L + 8
        if maxpos is not None and maxpos > base:
            base = 1 << (int(maxpos) - 1).bit_length()
        key = (float(theta), dev, base)
        if key not in self._tables:
            maxpos = base
            cs = torch.empty((maxpos + 1) * self.d.hd, device=dev, dtype=F32)
            ops.rope_table(cs, maxpos, self.d.hd, theta)
            self._tables[key] = cs
        return self._tables[key]

    def colsum_ws_rows(self, rows, n):
        """fp32 [rows, n] partial-sum scratch (pz_act_bwd_colsum), one per device, grown on demand"""
        dev = self.ar.data.device
        t = self._ws.get(("colsum_rows", dev))
        if t is None or t.numel() < rows * n:
            t = torch.empty(rows * n, device=dev, dtype=F32)
            self._ws[("colsum_rows", dev)] = t
        return t[: rows * n].view(rows, n)

    def colsum_ws(self, n):
        dev = self.ar.data.device
        t = self._ws.get(("colsum", dev))
        if t is None or t.numel() < 64 * n:
            t = torch.empty(64 * max(n, 4608), device=dev, dtype=F32)
            self._ws[("colsum", dev)] = t
        return t

    def groups(self, tied, active=("vlm", "proprio", "action"), text=None):
        """The weight groups of the ``active`` mixtures in joint-token order (the group that holds the action rows
        last); a group's name also keys its rows / positions in the callers' dicts.  text = q (text generation): the
        vlm group over q new tokens, every layer run to its end."""
        d = self.d
        out = []
        mp = "joint_model.mixtures."
        if "vlm" in active:
            out.append(Group("vlm", mp + "vlm.layers.", d.P if text is None else text, 0, d.gH, d.gI, d.g_theta,
                             text is None))
        if tied:
            mix = [m for m in ("proprio", "action") if m in active]
            T = (d.C if "proprio" in mix else 0) + (d.H if "action" in mix else 0)
            if T:
                off = d.P if "proprio" in mix else d.P + d.C
                out.append(Group("expert", mp + "action.layers.", T, off, d.aH, d.aI, d.a_theta, mix == ["proprio"]))
        else:
            if "proprio" in active:
                out.append(Group("proprio", mp + "proprio.layers.", d.C, d.P, d.aH, d.aI, d.p_theta, True))
            if "action" in active:
                out.append(Group("action", mp + "action.layers.", d.H, d.P + d.C, d.aH, d.aI, d.a_theta, False))
        return out

    # ------------------------------------------------------- second stream --
    def _side_stream(self, dev):
        st = self._side.get(dev)
        if st is None:
            st = self._side[dev] = torch.cuda.Stream(device=dev)
        return st

    @staticmethod
    def _on(side, g):
        """Context of one group's work: the action-expert group on the side stream with its own GEMM scratch
        (ops.workspace_slot), the vlm group on the current stream."""
        if side is None or g.name == "vlm":
            return contextlib.nullcontext()
        stack = contextlib.ExitStack()
        stack.enter_context(torch.cuda.stream(side))
        stack.enter_context(ops.workspace_slot(1))
        return stack

    # ================================================================ SigLIP ==
    def _sig_rows(self, M, dev):
        """[M, vI] bf16 rows at the SigLIP MLP row pitch (a view of [M, sig_pitch])"""
        return torch.empty(M, self.sig_pitch, device=dev, dtype=BF16)[:, : self.d.vI]

    def siglip_forward(self, pix, save):
        """siglip.py:34-300 + projector (siglip.py:9-31). pix bf16 [B,3,H,W] or [B,n_images,3,H,W] ->
        img [B*n_img, proj] (a sample's images' tokens consecutive, in image order)."""
        d = self.d
        pix = pix.reshape(-1, 3, d.img, d.img)
        B = pix.shape[0]  # images
        Nt = d.img_tok
        M = B * Nt
        dev = pix.device
        vt = "vision_tower.vision_model."
        kc = d.kcols
        cols = torch.empty(M, kc, device=dev, dtype=BF16)
        ops.patchify(pix, cols, d.ps)
        # patch-embedding weight with its K padded to a multiple of 32 columns: an engine-owned buffer whose
        # pad columns are zeroed once; the weight columns are refreshed by every forward (weights change)
        wpad = self._ws.get(("wpad", dev))
        if wpad is None:
            wpad = self._ws[("wpad", dev)] = torch.zeros(d.vH, kc, device=dev, dtype=BF16)
        wpatch = self.w(vt + "embeddings.patch_embedding.weight").view(d.vH, -1)
        ops.copy_rows(wpatch, wpatch.shape[1], 0, wpad, kc, 0, 1, d.vH, wpatch.shape[1])
        x = torch.empty(M, d.vH, device=dev, dtype=BF16)
        ops.gemm(Nt, d.vH, kc, cols, kc, True, wpad, kc, True, x, d.vH, batch=B, sA=(Nt * kc, 0),
                 sC=(Nt * d.vH, 0), bias=self.w(vt + "embeddings.patch_embedding.bias"),
                 resid=self.w(vt + "embeddings.position_embedding.weight"), ld_resid=d.vH, sR=(0, 0))
        if save is not None:
            save["cols"] = cols
        nh, hd = d.vheads, d.vH // d.vheads
        Np = Nt
        layers = []
        train = save is not None
        for i in range(d.vL):
            p = f"{vt}encoder.layers.{i}."
            st = {"x": x}
            if save is None and self.w8a8_in(p + "self_attn.q_proj.weight", M, d.vH):  # fp8: LayerNorm -> codes
                h1 = self.norm_codes(x, self.w(p + "layer_norm1.weight"), d.ln_eps, self.w(p + "layer_norm1.bias"))
                mu1 = r1 = None
            else:
                h1 = torch.empty_like(x)
                mu1 = torch.empty(M, device=dev, dtype=F32)
                r1 = torch.empty(M, device=dev, dtype=F32)
                ops.layernorm(x, self.w(p + "layer_norm1.weight"), self.w(p + "layer_norm1.bias"), h1, mu1, r1,
                              d.ln_eps)
            qkv = torch.empty(M, 3 * d.vH, device=dev, dtype=BF16)
            u_qkv = self._linear(h1, [p + f"self_attn.{k}_proj.weight" for k in "qkv"], self.qkv_siglip(p), qkv, train,
                                 bias=self.span(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias"))
            # fused attention (siglip.py:108-166) in place on the q|k|v rows: O and one fp32
            # log-sum-exp per (head, query) row; no [B, heads, N, N] tensor exists
            O = torch.empty(M, d.vH, device=dev, dtype=BF16)
            lse = torch.empty(B * nh, Np, device=dev, dtype=F32)
            ops.flash_fwd(ops.siglip_flash_args(qkv, O, lse, B, nh, hd, Np))
            xm = torch.empty_like(x)
            u_o = self._linear(O, [p + "self_attn.out_proj.weight"], self.w(p + "self_attn.out_proj.weight"), xm, train,
                               bias=self.w(p + "self_attn.out_proj.bias"), resid=x)
            if save is None and self.w8a8_in(p + "mlp.fc1.weight", M, d.vH):  # fp8: LayerNorm -> codes
                h2 = self.norm_codes(xm, self.w(p + "layer_norm2.weight"), d.ln_eps, self.w(p + "layer_norm2.bias"))
                mu2 = r2 = None
            else:
                h2 = torch.empty_like(x)
                mu2 = torch.empty(M, device=dev, dtype=F32)
                r2 = torch.empty(M, device=dev, dtype=F32)
                ops.layernorm(xm, self.w(p + "layer_norm2.weight"), self.w(p + "layer_norm2.bias"), h2, mu2, r2,
                              d.ln_eps)
            a1 = self._sig_rows(M, dev) if save is not None else None
            g1 = self._sig_rows(M, dev)
            u_fc1 = self._linear(h2, [p + "mlp.fc1.weight"], self.w(p + "mlp.fc1.weight"), g1, train,
                                 bias=self.w(p + "mlp.fc1.bias"), epi=PZ_EPI_GELU, aux=a1)
            xn = torch.empty_like(x)
            u_fc2 = self._linear(g1, [p + "mlp.fc2.weight"], self.w(p + "mlp.fc2.weight"), xn, train,
                                 bias=self.w(p + "mlp.fc2.bias"), resid=xm)
            if save is not None:
                st.update(u_qkv=u_qkv, u_o=u_o, u_fc1=u_fc1, u_fc2=u_fc2)
                st.update(h1=h1, mu1=mu1, r1=r1, qkv=qkv, lse=lse, O=O, xm=xm, h2=h2, mu2=mu2, r2=r2, a1=a1, g1=g1)
                layers.append(st)
                self._chk(f"siglip fwd layer {i}", h1=h1, qkv=qkv, O=O, lse=lse, xm=xm, h2=h2, g1=g1, x=xn)
            x = xn
        y = torch.empty_like(x)
        mu = torch.empty(M, device=dev, dtype=F32)
        r = torch.empty(M, device=dev, dtype=F32)
        ops.layernorm(x, self.w(vt + "post_layernorm.weight"), self.w(vt + "post_layernorm.bias"), y, mu, r, d.ln_eps)
        img = torch.empty(M, d.proj, device=dev, dtype=BF16)
        u_proj = self._linear(y, ["multi_modal_projector.linear.weight"], self.w("multi_modal_projector.linear.weight"),
                              img, train, bias=self.w("multi_modal_projector.linear.bias"))
        if save is not None:
            save["u_proj"] = u_proj
            save.update(layers=layers, x_last=x, y=y, mu=mu, r=r, B=B)
            self._chk("siglip fwd post-LN + projector", y=y, img=img)
        return img

    def siglip_backward(self, sv, dimg, beta):
        d = self.d
        B = sv["B"]  # images
        M = B * d.img_tok
        dev = dimg.device
        vt = "vision_tower.vision_model."
        rpp = ops.rows_per_part()
        P = (M + rpp - 1) // rpp
        ws = self.colsum_ws(max(d.vI, 3 * d.vH))
        pw = torch.empty(P, d.vH, device=dev, dtype=F32)
        pb = torch.empty(P, d.vH, device=dev, dtype=F32)
        # bias gradients fused into the passes that produce their output gradients (LayerNorm backward -> the
        # column sums of dx: fc2 / out_proj; GELU backward -> fc1); separate colsum passes under PZ_NORM_BWD=wave,
        # whose LayerNorm backward yields no partials
        fb = os.environ.get("PZ_NORM_BWD", "row")[:1] != "w"
        pd = torch.empty(P, d.vH, device=dev, dtype=F32) if fb else None  # column partials of the current dx
        pdn = torch.empty(P, d.vH, device=dev, dtype=F32) if fb else None  # ... of the next layer's dx
        pd2 = torch.empty(P, d.vH, device=dev, dtype=F32) if fb else None  # ... of dxm
        # a layer's LayerNorm weight / bias and Linear bias reductions go out as one launch at its end
        # (pz_reduce_parts_multi), so its two LayerNorms keep their own partials
        pw2 = torch.empty(P, d.vH, device=dev, dtype=F32)
        pb2 = torch.empty(P, d.vH, device=dev, dtype=F32)
        ws_act = self.colsum_ws_rows(1024, d.vI) if fb else None
        # projector
        nm = "multi_modal_projector.linear."
        if self.rg(nm + "weight"):
            ops.linear_wgrad(dimg, sv["y"], self.gw(nm + "weight"), beta=beta)
        if self.rg(nm + "bias"):
            ops.colsum(dimg, self.gw(nm + "bias"), ws, beta=beta)
        dy = torch.empty(M, d.vH, device=dev, dtype=BF16)
        self._dgrad([nm + "weight"], sv["y"], sv["u_proj"], dimg, self.w(nm + "weight"), dy, beta)
        dx = torch.empty_like(dy)
        ops.layernorm_bwd(dy, sv["x_last"], self.w(vt + "post_layernorm.weight"), sv["mu"], sv["r"], dx,
                          dw_part=pw, db_part=pb, dx_part=pd)
        self._norm_grads(vt + "post_layernorm.", pw, pb, beta)
        nh, hd = d.vheads, d.vH // d.vheads
        Np = d.img_tok
        W3 = 3 * d.vH
        dg = self._sig_rows(M, dev)
        delta = torch.empty(B * nh, Np, device=dev, dtype=F32)
        dqkv = torch.empty(M, W3, device=dev, dtype=BF16)
        dh = torch.empty(M, d.vH, device=dev, dtype=BF16)
        dxm = torch.empty(M, d.vH, device=dev, dtype=BF16)
        dO = torch.empty(M, d.vH, device=dev, dtype=BF16)
        for i in reversed(range(d.vL)):
            p = f"{vt}encoder.layers.{i}."
            st = sv["layers"][i]
            red = []  # deferred (partials, gradient) reductions of this layer
            # MLP: x' = xm + fc2(gelu(fc1(ln2(xm))))
            # dgrad through fc2, then the GELU derivative at the saved pre-activation a1
            fc1b = self.rg(p + "mlp.fc1.bias")
            # plain dgrad GEMM, then the GELU backward (HBM-bound) in place
            self._dgrad([p + "mlp.fc2.weight"], st["g1"], st["u_fc2"], dx, self.w(p + "mlp.fc2.weight"), dg, beta)
            if fb and fc1b:  # + the fc1 bias gradient from the same pass
                ops.act_bwd_colsum(dg, st["a1"], dg, PZ_EPI_GELU, ws_act, self.gw(p + "mlp.fc1.bias"), beta=beta)
            else:
                ops.act_bwd(dg, st["a1"], dg, None, PZ_EPI_GELU)
            if self.rg(p + "mlp.fc2.weight"):
                ops.linear_wgrad(dx, st["g1"], self.gw(p + "mlp.fc2.weight"), beta=beta)
            st["g1"] = None
            if self.rg(p + "mlp.fc2.bias"):
                if fb:  # column sums of dx from the LayerNorm backward that produced it
                    self._reduce(red, pd, self.gw(p + "mlp.fc2.bias"), beta)
                else:
                    ops.colsum(dx, self.gw(p + "mlp.fc2.bias"), ws, beta=beta)
            if self.rg(p + "mlp.fc1.weight"):
                ops.linear_wgrad(dg, st["h2"], self.gw(p + "mlp.fc1.weight"), beta=beta)
            if fc1b and not fb:
                ops.colsum(dg, self.gw(p + "mlp.fc1.bias"), ws, beta=beta)
            self._dgrad([p + "mlp.fc1.weight"], st["h2"], st["u_fc1"], dg, self.w(p + "mlp.fc1.weight"), dh, beta)
            ops.layernorm_bwd(dh, st["xm"], self.w(p + "layer_norm2.weight"), st["mu2"], st["r2"], dxm, dres=dx,
                              dw_part=pw2, db_part=pb2, dx_part=pd2)
            self._norm_grads(p + "layer_norm2.", pw2, pb2, beta, red)
            # attention out-proj
            if self.rg(p + "self_attn.out_proj.weight"):
                ops.linear_wgrad(dxm, st["O"], self.gw(p + "self_attn.out_proj.weight"), beta=beta)
            if self.rg(p + "self_attn.out_proj.bias"):
                if fb:
                    self._reduce(red, pd2, self.gw(p + "self_attn.out_proj.bias"), beta)
                else:
                    ops.colsum(dxm, self.gw(p + "self_attn.out_proj.bias"), ws, beta=beta)
            self._dgrad([p + "self_attn.out_proj.weight"], st["O"], st["u_o"], dxm,
                        self.w(p + "self_attn.out_proj.weight"), dO, beta)
            # fused attention backward: dQ | dK | dV straight into the q|k|v gradient rows
            ops.flash_bwd(ops.siglip_flash_args(st["qkv"], st["O"], st["lse"], B, nh, hd, Np, dO=dO, delta=delta,
                                                dqkv=dqkv))
            qn, vn = p + "self_attn.q_proj.", p + "self_attn.v_proj."
            if all(self.rg(p + f"self_attn.{k}_proj.weight") for k in "qkv"):
                ops.linear_wgrad(dqkv, st["h1"], self.ar.grad_span(qn + "weight", vn + "weight"), beta=beta)
            else:
                for k, c0 in (("q", 0), ("k", d.vH), ("v", 2 * d.vH)):
                    if self.rg(p + f"self_attn.{k}_proj.weight"):
                        ops.linear_wgrad(dqkv[:, c0:c0 + d.vH], st["h1"], self.gw(p + f"self_attn.{k}_proj.weight"),
                                         beta=beta)
            if all(self.rg(p + f"self_attn.{k}_proj.bias") for k in "qkv"):
                ops.colsum(dqkv, self.ar.grad_span(qn + "bias", vn + "bias"), ws, beta=beta)
            self._dgrad([p + f"self_attn.{k}_proj.weight" for k in "qkv"], st["h1"], st["u_qkv"], dqkv,
                        self.qkv_siglip(p), dh, beta)
            dxn = torch.empty_like(dx)
            ops.layernorm_bwd(dh, st["x"], self.w(p + "layer_norm1.weight"), st["mu1"], st["r1"], dxn, dres=dxm,
                              dw_part=pw, db_part=pb, dx_part=pdn)
            self._norm_grads(p + "layer_norm1.", pw, pb, beta, red)
            if red:
                ops.reduce_parts_multi(red, beta=beta)
            pd, pdn = pdn, pd  # this layer's dxn partials: the next (lower) layer's fc2 bias gradient
            dx = dxn
            self._chk(f"siglip bwd layer {i}", dg=dg, dO=dO, dqkv=dqkv, dxm=dxm, dx=dxn)
            self._notify("vision", i)
        # patch embedding + position embedding
        pe = vt + "embeddings."
        if self.rg(pe + "position_embedding.weight"):
            ops.batch_sum(dx, B, d.img_tok * d.vH, d.img_tok * d.vH, self.gw(pe + "position_embedding.weight"),
                          beta=beta)
        if self.rg(pe + "patch_embedding.bias"):
            ops.colsum(dx, self.gw(pe + "patch_embedding.bias"), ws, beta=beta)
        if self.rg(pe + "patch_embedding.weight"):
            kc = d.kcols
            tmp = torch.empty(d.vH, kc, device=dev, dtype=BF16)
            ops.linear_wgrad(dx, sv["cols"], tmp)
            g = self.gw(pe + "patch_embedding.weight").view(d.vH, -1)
            ops.copy_rows(tmp, kc, 0, g, g.shape[1], 0, 1, d.vH, g.shape[1], beta=beta)
        self._notify("vision", -1)

    def qkv_siglip(self, p):
        return self.span(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight")

    def _norm_grads(self, prefix, pw, pb, beta, red=None):
        if pw is not None and self.rg(prefix + "weight"):
            self._reduce(red, pw, self.gw(prefix + "weight"), beta)
        if pb is not None and self.rg(prefix + "bias"):
            self._reduce(red, pb, self.gw(prefix + "bias"), beta)

    @staticmethod
    def _rms_name(g, l, site):
        if site == "":
            return g.prefix[: -len("layers.")] + "norm."
        return f"{g.prefix}{l}." + ("input_layernorm." if site == "in_" else "post_attention_layernorm.")

    def _norm_fwd(self, A, g, x, l, site, h, rstd=None):
        """h = the norm ``site`` of group g over x: the AdaptiveRMSNorm of its Ada, or (A None) the Gemma RMSNorm.
        site: "in_" | "post_" of layer l, or "" with l = "norm" (the mixture's final norm)"""
        if A is not None:
            A.norm_fwd(x, l, site, g.T, h, rstd)
        else:
            ops.rmsnorm(x, self.w(self._rms_name(g, l, site) + "weight"), h, rstd, self.d.rms_eps)

    def _norm_bwd(self, A, g, dh, x, rstd, l, site, dx, dres, beta):
        """backward of _norm_fwd: dx = d norm(x) (+ dres); the RMSNorm weight gradient from its row partials (an Ada
        accumulates its modulation gradient rows instead, Ada.weight_grads)"""
        if A is not None:
            return A.norm_bwd(dh, x, rstd, l, site, g.T, dx, dres=dres)
        name = self._rms_name(g, l, site)
        if self._dgrad_only:
            return ops.rmsnorm_bwd(dh, x, self.w(name + "weight"), rstd, dx, dres=dres)
        rpp = ops.rows_per_part()
        part = torch.empty((x.shape[0] + rpp - 1) // rpp, g.hid, device=x.device, dtype=F32)
        ops.rmsnorm_bwd(dh, x, self.w(name + "weight"), rstd, dx, dres=dres, dw_part=part)
        self._norm_grads(name, part, None, beta)

    @staticmethod
    def _reduce(red, part, out, beta):
        """reduce_parts now (red None) or deferred into the layer's list for one pz_reduce_parts_multi launch"""
        if red is None:
            ops.reduce_parts(part, out, beta=beta)
        else:
            red.append((part, out))

    # ============================================================ embeddings ==
    def embed_prefix(self, ids, img):
        d = self.d
        B = ids.shape[0]
        X = torch.empty(B * d.P, d.gH, device=ids.device, dtype=BF16)
        # pizero.py:395 (/sqrt(hidden)) and joint_model.py:355 (*sqrt(hidden)) cancel for image rows
        ops.embed_merge(ids, self.w("embed_tokens.weight"), img, X, d.n_img, d.image_token, d.pad_token,
                        math.sqrt(d.gH), 1.0)
        return X

    def _action_embed_tail(self, cat, alpha=1.0):
        """the action encoder after its concat input (inference): Linear + SiLU, Linear -- the last one times alpha
        (a power of two: the bias is pre-scaled by it, exactly, and cached per weight version)"""
        d = self.d
        e2 = torch.empty(cat.shape[0], d.aH, device=cat.device, dtype=BF16)
        ops.linear(cat, self.w("action_encoder.linear_2.weight"), e2, bias=self.w("action_encoder.linear_2.bias"),
                   epi=PZ_EPI_SILU)
        e3 = torch.empty_like(e2)
        b3 = self.w("action_encoder.linear_3.bias")
        if alpha != 1.0:
            if getattr(self, "_b3s_alpha", None) != alpha:
                self._b3s = torch.empty_like(b3)
                self._b3s_alpha, self._b3s_version = alpha, None
            self.derived_refresh()
            b3 = self._b3s
        ops.linear(e2, self.w("action_encoder.linear_3.weight"), e3, bias=b3, alpha=alpha)
        return e3

    def derived_refresh(self):
        """Recompute the weight-derived bf16 tensors (the alpha-scaled action-encoder bias) IN PLACE when the
        weights changed: a captured InferenceGraph holds their pointers, so InferenceGraph.replay calls this
        before every replay.  Returns True if it recomputed."""
        if getattr(self, "_b3s_alpha", None) is None or self._b3s_version == self.weights_version():
            return False
        b3 = self.w("action_encoder.linear_3.bias")
        self._b3s.copy_(b3.float() * self._b3s_alpha)  # exact: alpha is a power of two
        self._b3s_version = self.weights_version()
        return True

    def action_embed(self, psi_bf, t, save, prefix_len=None):
        """ActionEncoder (vla/modules.py:39-53) with time embedding (vla/modules.py:15-22).  Inference (save None):
        the first Linear and the time embedding write straight into the concat input (pz_time_embed_rows: no
        separate embedding buffer or concat launch) and no pre-activation is kept.  ``prefix_len`` (int32 [B], DESIGN
        7f): the time columns of rows h < prefix_len[b] are the embedding of 1.0."""
        d = self.d
        if d.ada and prefix_len is not None:
            raise NotImplementedError(PREFIX_ADAPTIVE_MSG)
        rows = psi_bf.shape[0]
        B = t.shape[0]
        dev = psi_bf.device
        if d.ada:  # time_cond=False (vla/modules.py:33-34,46): no time concat, linear_2 is width -> width
            e1 = torch.empty(rows, d.aH, device=dev, dtype=BF16)
            ops.small_linear(psi_bf, self.w("action_encoder.linear_1.weight"), e1,
                             bias=self.w("action_encoder.linear_1.bias"))
            pre = None if save is None else torch.empty(rows, d.aH, device=dev, dtype=BF16)
            e2 = torch.empty(rows, d.aH, device=dev, dtype=BF16)
            ops.linear(e1, self.w("action_encoder.linear_2.weight"), e2, bias=self.w("action_encoder.linear_2.bias"),
                       epi=PZ_EPI_SILU, aux=pre)
            e3 = torch.empty(rows, d.aH, device=dev, dtype=BF16)
            ops.linear(e2, self.w("action_encoder.linear_3.weight"), e3, bias=self.w("action_encoder.linear_3.bias"))
            if save is not None:
                save.update(ae_psi=psi_bf, ae_cat=e1, ae_pre=pre, ae_e2=e2)
            return e3
        if save is None:
            cat = torch.empty(rows, 2 * d.aH, device=dev, dtype=BF16)
            ops.small_linear(psi_bf, self.w("action_encoder.linear_1.weight"), cat[:, d.aH:],
                             bias=self.w("action_encoder.linear_1.bias"))
            ops.time_embed_rows(t, cat[:, : d.aH], rows // B, d.tmax, ref_bf16=d.time_bf16, prefix_len=prefix_len)
            e2 = torch.empty(rows, d.aH, device=dev, dtype=BF16)
            ops.linear(cat, self.w("action_encoder.linear_2.weight"), e2, bias=self.w("action_encoder.linear_2.bias"),
                       epi=PZ_EPI_SILU)
            e3 = torch.empty(rows, d.aH, device=dev, dtype=BF16)
            ops.linear(e2, self.w("action_encoder.linear_3.weight"), e3, bias=self.w("action_encoder.linear_3.bias"))
            return e3
        e1 = torch.empty(rows, d.aH, device=dev, dtype=BF16)
        ops.small_linear(psi_bf, self.w("action_encoder.linear_1.weight"), e1, bias=self.w("action_encoder.linear_1.bias"))
        temb = torch.empty(B, d.aH, device=dev, dtype=BF16)
        ops.time_embed(t, temb, d.tmax, ref_bf16=d.time_bf16)
        cat = torch.empty(rows, 2 * d.aH, device=dev, dtype=BF16)
        ops.concat_time(temb, e1, cat, B, rows // B, d.aH, prefix_len=prefix_len, max_period=d.tmax,
                        ref_bf16=d.time_bf16)
        pre = torch.empty(rows, d.aH, device=dev, dtype=BF16)
        e2 = torch.empty(rows, d.aH, device=dev, dtype=BF16)
        ops.linear(cat, self.w("action_encoder.linear_2.weight"), e2, bias=self.w("action_encoder.linear_2.bias"),
                   epi=PZ_EPI_SILU, aux=pre)
        e3 = torch.empty(rows, d.aH, device=dev, dtype=BF16)
        ops.linear(e2, self.w("action_encoder.linear_3.weight"), e3, bias=self.w("action_encoder.linear_3.bias"))
        if save is not None:
            save.update(ae_psi=psi_bf, ae_cat=cat, ae_pre=pre, ae_e2=e2)
        return e3

    # ======================================================== joint layers ==
    def _joint_flash(self, groups, Q, K, V, Os, lse, cnt, B, Lq, dO=None, delta=None, dq=None, dk=None, dv=None):
        """pz_flash_args of the joint attention: query rows r = token*nh + head of Q [B, Lq*nh, hd],
        keys/values K, V [B, Lp, hd]; output groups = the mixtures' O buffers [B*T, nh*hd] in
        token order (joint_model.py:259-292 with the Pi0 block mask, pizero.py:271-306)."""
        d = self.d
        nh, hd, Lp = d.nh, d.hd, K.shape[1]
        gs = sorted(groups, key=lambda g: g.off)
        return ops.flash_args(
            B, 1, Lq * nh, d.L, hd, Q, (hd, Lq * nh * hd, 0), K, (hd, Lp * hd, 0), V, (hd, Lp * hd, 0),
            [(g.off * nh, Os[g.name], g.T * nh * hd, hd) for g in gs], 0, lse, 1.0 / math.sqrt(hd), cap=50.0,
            mask_mode=1, cnt=cnt, prefix=d.P, cond=d.C, rows_per_token=nh,
            dgroups=None if dO is None else [dO.get(g.name) for g in gs], delta=delta, dq=dq, dk=dk, dv=dv)

    def _attn_gemm(self, Q, K, V, S, Os, groups, qoff, Lq, nk, which, cnt, B, export=False):
        """The GEMM attention path: S = Q K^T per sample into the caller's fp32 scratch S [B, Lq*nh, Lp] (MQA heads
        stacked as rows), soft-cap + mask softmax (the block mask from cnt or its GeneralMask field ``which``), then
        O = P V of every group of ``groups`` into Os.  The Lq query tokens start at joint token qoff and see the first
        nk keys.  Returns (P, tanh(cap) export or None), bf16 [B, Lq*nh, Lp]; export: for the training backward."""
        d = self.d
        nh, hd, Lp = d.nh, d.hd, d.Lp
        ops.gemm(Lq * nh, nk, hd, Q, hd, True, K, hd, True, S, Lp, batch=B, sA=(Lq * nh * hd, 0), sB=(Lp * hd, 0),
                 sC=(Lq * nh * Lp, 0))
        Pm = torch.empty(B, Lq * nh, Lp, device=Q.device, dtype=BF16)
        tc = torch.empty_like(Pm) if export else None
        ops.attn_softmax(S, Lp, Pm, Lp, B * Lq * nh, nk, 1.0 / math.sqrt(hd), cap=50.0, tcap=tc,
                         rows_per_batch=Lq * nh, heads=nh, qoff=qoff, **_mask_kw(d, cnt, which))
        for g in groups:
            ops.gemm(g.T * nh, hd, Lp, Pm[:, (g.off - qoff) * nh:], Lp, True, V, hd, False, Os[g.name], hd, batch=B,
                     sA=(Lq * nh * Lp, 0), sB=(Lp * hd, 0), sC=(g.T * nh * hd, 0))
        return Pm, tc

    def _joint_kv(self, B, Lp, dev, save):
        """Joint K/V buffers [nL, B, Lp, hd] for one training forward.  The engine owns one zeroed set
        (the Lp - L pad rows stay zero for the GEMM path; rows < L are rewritten by every forward) and
        lends it to the forward whose saved state (``save``) holds the token; while that state is alive
        (its backward has not run and its graph still exists) another forward gets fresh buffers, so
        interleaved forwards never share saved K/V."""
        holder = self._jkv_holder() if self._jkv_holder is not None else None
        if holder is not None:
            k = torch.zeros(self.d.nL, B, Lp, self.d.hd, device=dev, dtype=BF16)
            return k, torch.zeros_like(k)
        key = ("jkv", B, Lp, dev)
        kv = self._ws.get(key)
        if kv is None:
            self._ws = {k: v for k, v in self._ws.items() if k[0] != "jkv"}  # one shape at a time
            k = torch.zeros(self.d.nL, B, Lp, self.d.hd, device=dev, dtype=BF16)
            kv = self._ws[key] = (k, torch.zeros_like(k))
        tok = _Token()
        save["_jkv_token"] = tok
        self._jkv_holder = weakref.ref(tok)
        return kv

    def _pre_attn_train(self, g, l, X, pos, st, Qj, Kj, Vj, dev, ada=None, Lq=None, qoff=None, Lk=None, koff=None):
        """One group's input RMSNorm + q|k|v projection + RoPE + joint Q / K / V scatter of joint layer l
        (paligemma/modules.py:7-21, mixture.py:162-215, joint_model.py:170-257).  Lq / qoff: Qj holds Lq query tokens
        per sample and the group's start at qoff (default: all L joint tokens, the group at g.off).  Lk / koff: Kj / Vj
        hold Lk key rows per sample and the group's start at koff (default: the Lp joint rows, the group at g.off)."""
        d = self.d
        L, Lp, nh, hd = d.L if Lq is None else Lq, d.Lp if Lk is None else Lk, d.nh, d.hd
        qoff = g.off if qoff is None else qoff
        koff = g.off if koff is None else koff
        B = Qj.shape[0]
        p = f"{g.prefix}{l}."
        x = X[g.name]
        M = x.shape[0]
        h = torch.empty_like(x)
        r = torch.empty(M, device=dev, dtype=F32)
        self._norm_fwd(ada.get(g.name) if ada else None, g, x, l, "in_", h, r)

        def proj(h, W, _, lora):
            # q|k|v projection + RoPE + joint scatter: one 8-phase GEMM whose epilogue rotates and writes
            # Q / K / V (N1: no [M, 2560] qkv tensor, no split launch); rows too few for the 8-phase
            # kernel (the action expert's 320) take GEMM + qkv_rope_split (same bits)
            if not (self.fuse_qkv_rope and ops.gemm_qkv_rope(h, W, pos[g.name], self.rope(g.theta), Qj, Kj, Vj, g.T,
                                                             nh, hd, L, qoff, Lp, koff, lora=lora)):
                qkv = torch.empty(M, (nh + 2) * hd, device=dev, dtype=BF16)
                ops.linear(h, W, qkv, lora=lora)
                ops.qkv_rope_split(qkv, pos[g.name], self.rope(g.theta), Qj, Kj, Vj, B, g.T, nh, 1, hd, L, qoff, Lp,
                                   koff)

        u = self._linear(h, [p + f"self_attn.{k}_proj.weight" for k in "qkv"], self.qkv_w(p), None, True, gemm=proj)
        st["g"][g.name] = {"x": x, "h": h, "r": r, "u_qkv": u}

    def _post_attn(self, g, l, x, O, A=None, gs=None, plain=False):
        """One group's o_proj (+ residual), post-attention norm and GeGLU MLP (+ residual) of joint layer l
        (mixture.py:216-242, paligemma/modules.py:86-95) on the attention output O; returns the layer's output rows.
        A (an adaLN group): AdaptiveRMSNorm after the attention; adaLN-Zero gates both branch outputs before their
        residual adds (joint_model.py:70-79,117-126), each in the row pass that follows it: o_proj's with the
        post-attention norm, the MLP's alone.  gs (training): the activations and the adapters' u are saved in it for
        the backward; inference keeps no pre-activation and runs the few-row / fp8 forms of the Gemma norm + gate|up.
        plain: the inference pass behind the GEMM attention (infer_flash False, a GeneralMask), which has always run
        norm + bf16 GEMMs here -- with fp8 codes prepared too, and for the few rows whose norm the flash path fuses;
        kept as it is because routing it like the flash path changes its outputs (fp8 for certain)."""
        d = self.d
        p = f"{g.prefix}{l}."
        M, dev = x.shape[0], x.device
        train = gs is not None
        zero = A is not None and A.zero
        o_n, gu_n, dn_n = [p + "self_attn.o_proj.weight"], [p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"], \
            [p + "mlp.down_proj.weight"]
        nw = None if A is not None else (self.w(p + "post_attention_layernorm.weight"), d.rms_eps)
        xm = torch.empty_like(x)
        yo = torch.empty_like(x) if zero else None
        u_o = self._linear(O, o_n, self.w(o_n[0]), yo if zero else xm, train, not plain, resid=None if zero else x)
        hm = torch.empty(M, g.inter, device=dev, dtype=BF16)
        r2 = torch.empty(M, device=dev, dtype=F32) if train else None
        norm = None
        if zero:
            h2 = torch.empty_like(x)
            A.norm_fwd(x, l, "post_", g.T, h2, r2, y=yo, gate="post_z", xm=xm)
        elif nw and not train and not plain and self.few_rows(M, g.hid):
            h2, norm = xm, nw  # few rows (denoise / proprio): RMSNorm fused into the gate|up GEMM
        elif nw and not train and not plain and self.w8a8_in(gu_n[0], M, g.hid):
            h2 = self.norm_codes(xm, *nw)  # fp8: RMSNorm -> codes -> W8A8 GeGLU
        else:
            h2 = torch.empty_like(x)
            self._norm_fwd(A, g, xm, l, "post_", h2, r2)
        gu = torch.empty(M, 2 * g.inter, device=dev, dtype=BF16) if train else None
        u_gu = self._linear(h2, gu_n, self.gu_w(p), hm, train, not plain, epi=PZ_EPI_GEGLU, aux=gu, norm=norm)
        xn = torch.empty_like(x)
        yd = torch.empty_like(x) if zero else None
        u_dn = self._linear(hm, dn_n, self.w(dn_n[0]), yd if zero else xn, train, not plain,
                            resid=None if zero else xm)
        if zero:
            ops.adaln_fwd(xm, A.mod, g.T, d.rms_eps, y=yd, gate=A.biased(l, "final_z"), xm=xn)
        if train:
            gs.update(O=O, xm=xm, h2=h2, r2=r2, gu=gu, hm=hm, yo=yo, yd=yd, skip=False, u_o=u_o, u_gu=u_gu, u_dn=u_dn)
        return xn

    def _joint_layers_train(self, groups, X, pos, cnt, B, save):
        """joint_model.py:24-304 x nL for the training pass (all mixtures active)."""
        d = self.d
        dev = X[groups[0].name].device
        L, Lp, nh, hd = d.L, d.Lp, d.nh, d.hd
        S = None
        layers = []
        Kall, Vall = self._joint_kv(B, Lp, dev, save)
        ada = save.get("ada")
        # the action-expert group's pre- and post-attention work on the second stream, concurrent with the vlm
        # group's; the streams meet at the joint attention (as in _joint_layers_backward)
        main = torch.cuda.current_stream(dev)
        side = None
        if self.expert_stream and self.expert_stream_fwd and len(groups) > 1 and dev.type == "cuda":
            side = self._side_stream(dev)
            side.wait_stream(main)
            for t in X.values():
                if t is not None:
                    t.record_stream(side)
            for A in (ada or {}).values():
                A.mod.record_stream(side)
        for l in range(d.nL):
            last = l == d.nL - 1
            Qj = torch.empty(B, L, nh * hd, device=dev, dtype=BF16)
            if side is not None:
                Qj.record_stream(side)
            Kj, Vj = Kall[l], Vall[l]
            st = {"Q": Qj, "K": Kj, "V": Vj, "g": {}}
            for g in groups:
                with self._on(side, g):
                    self._pre_attn_train(g, l, X, pos, st, Qj, Kj, Vj, dev, ada)
            if side is not None:
                main.wait_stream(side)  # every group's Q / K / V rows before the joint attention
            Os = {g.name: torch.empty(B * g.T, nh * hd, device=dev, dtype=BF16) for g in groups}
            if self.joint_flash and not isinstance(cnt, GeneralMask):
                # fused joint attention (joint_model.py:259-292): soft-cap, block mask from cnt, O rows
                # scattered into each mixture's o_proj input; one fp32 log-sum-exp per (token, head) row
                lse = torch.empty(B, L * nh, device=dev, dtype=F32)
                ops.flash_fwd(self._joint_flash(groups, Qj, Kj, Vj, Os, lse, cnt, B, L))
                st["lse"], st["O"] = lse, Os
            elif self.joint_probs and not isinstance(cnt, GeneralMask) and L <= 320 and hd == 256:
                # (pz_flash_fwd_probs keeps a whole score row in registers: <= 320 keys; C5's 839 take the
                # GEMM path)
                # one fused kernel: S = Q K^T with K staged in LDS, soft-cap + block mask + exact row softmax
                # in registers, P / tanh(cap) exported in bf16 for the GEMM-path backward, O = P V
                Pm = torch.empty(B, L * nh, Lp, device=dev, dtype=BF16)
                tc = torch.empty(B, L * nh, Lp, device=dev, dtype=BF16)
                ops.flash_fwd_probs(self._joint_flash(groups, Qj, Kj, Vj, Os, None, cnt, B, L), Pm, tc, Lp)
                st["P"], st["tc"], st["O"] = Pm, tc, Os
            else:
                if S is None:
                    S = torch.empty(B, L * nh, Lp, device=dev, dtype=F32)
                live = [g for g in groups if not (last and g.skip_last)]
                st["P"], st["tc"] = self._attn_gemm(Qj, Kj, Vj, S, Os, live, 0, L, L, "full", cnt, B, export=True)
                st["O"] = Os
            if side is not None:
                side.wait_stream(main)  # the attention outputs
                for t in Os.values():
                    t.record_stream(side)
            for g in groups:
                gs = st["g"][g.name]
                if last and g.skip_last:
                    X[g.name] = None
                    gs["skip"] = True
                    continue
                with self._on(side, g):
                    X[g.name] = self._post_attn(g, l, X[g.name], Os[g.name], ada.get(g.name) if ada else None, gs)
            layers.append(st)
            self._chk(f"joint fwd layer {l}", Q=Qj, K=Kj, V=Vj, O=Os, P=st.get("P"), tc=st.get("tc"), X=X)
        if side is not None:  # the expert output and its saved activations are read on the main stream later
            main.wait_stream(side)
            for t in X.values():
                if t is not None:
                    t.record_stream(main)
            for st in layers:
                for g in groups:
                    if g.name != "vlm":
                        for t in st["g"][g.name].values():
                            if isinstance(t, torch.Tensor):
                                t.record_stream(main)
        save["joint"] = layers
        return X

    def _mlp_oproj_backward(self, g, gs, p, dX, dO, dXm, beta, nh, hd, dev, A=None, l=None):
        """One group's GeGLU MLP + post-attention RMSNorm + o_proj backward of a joint layer
        (paligemma/modules.py:86-95, mixture.py:216-242): dX[g] -> dO[g] (the attention output gradient)
        and dXm[g] (the residual gradient into the input RMSNorm backward)."""
        dx = dres = dX[g.name]
        M = dx.shape[0]
        if A is not None and A.zero:
            # adaLN-Zero: the MLP branch was gated before its residual add -- the branch gradient is dx * sigma (and the
            # sample's gate gradient), the residual path keeps dx
            dx = ops.adaln_gate_bwd(dres, gs["yd"], A.mod, A.biased(l, "final_z"), torch.empty_like(dres), A.dmod, g.T)
            gs["yd"] = None
        # MLP
        # dgrad through down_proj with the GeGLU derivative fused into its epilogue:
        # gu (saved g|u) <- d(gate|up) in place; hm (saved GeGLU output) feeds the down_proj wgrad
        gu = gs["gu"]
        self._dgrad([p + "mlp.down_proj.weight"], gs["hm"], gs["u_dn"], dx, self.w(p + "mlp.down_proj.weight"), gu,
                    beta, epi=PZ_EPI_DGEGLU, aux=gu)
        if self.rg(p + "mlp.down_proj.weight"):
            ops.linear_wgrad(dx, gs["hm"], self.gw(p + "mlp.down_proj.weight"), beta=beta)
        gs["hm"] = None
        if self.rg(p + "mlp.gate_proj.weight") and self.rg(p + "mlp.up_proj.weight"):
            ops.linear_wgrad(gu, gs["h2"], self.ar.grad_span(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"),
                             beta=beta)
        dh2 = torch.empty(M, g.hid, device=dev, dtype=BF16)
        self._dgrad([p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"], gs["h2"], gs["u_gu"], gu, self.gu_w(p), dh2,
                    beta)
        dxm = torch.empty_like(dx)
        self._norm_bwd(A, g, dh2, gs["xm"], gs["r2"], l, "post_", dxm, dres, beta)
        # o_proj (adaLN-Zero: its output was gated before the residual add)
        dyo = dxm
        if A is not None and A.zero:
            dyo = ops.adaln_gate_bwd(dxm, gs["yo"], A.mod, A.biased(l, "post_z"), torch.empty_like(dxm), A.dmod, g.T)
            gs["yo"] = None
        if self.rg(p + "self_attn.o_proj.weight"):
            ops.linear_wgrad(dyo, gs["O"], self.gw(p + "self_attn.o_proj.weight"), beta=beta)
        o = torch.empty(M, nh * hd, device=dev, dtype=BF16)
        self._dgrad([p + "self_attn.o_proj.weight"], gs["O"], gs["u_o"], dyo, self.w(p + "self_attn.o_proj.weight"), o,
                    beta)
        dO[g.name] = o
        dXm[g.name] = dxm

    def _qkv_backward(self, g, gs, p, dQ, dK, dV, dX, dXm, pos, B, L, Lp, beta, nh, hd, dev, A=None, l=None, qoff=None,
                      koff=None):
        """One group's q|k|v projection + input RMSNorm backward of a joint layer (mixture.py:162-215,
        joint_model.py:170-257 + inverse RoPE): dQ / dK / dV rows of the group -> dX[g].  dQ holds L query tokens per
        sample, the group's from qoff (default g.off); dK / dV hold Lp key rows per sample, the group's from koff
        (default g.off)."""
        qoff = g.off if qoff is None else qoff
        koff = g.off if koff is None else koff
        x = gs["x"]
        M = x.shape[0]
        W = (nh + 2) * hd
        dqkv = torch.empty(M, W, device=dev, dtype=BF16)
        ops.qkv_rope_split_bwd(None if gs.get("skip") else dQ, dK, dV, pos[g.name], self.rope(g.theta), dqkv,
                               B, g.T, nh, 1, hd, L, qoff, Lp, koff)
        names = [p + f"self_attn.{k}_proj.weight" for k in "qkv"]
        rgs = [self.rg(n) for n in names]
        dh = torch.empty(M, g.hid, device=dev, dtype=BF16)
        if gs.get("skip") and self.lora(*names) is None:
            # last vlm layer: its query rows feed nothing (the post-attention block is skipped), so dQ = 0 exactly --
            # the q_proj gradient is zero (written as such, not computed: pizero.py:231's frozen v_proj and the zero
            # q_proj grad) and only the k|v columns enter the weight / input gradients
            if rgs[0] and not beta:
                self.gw(names[0]).zero_()
            for n, rgk, c0, c1 in zip(names[1:], rgs[1:], (nh * hd, (nh + 1) * hd), ((nh + 1) * hd, W)):
                if rgk:
                    ops.linear_wgrad(dqkv[:, c0:c1], gs["h"], self.gw(n), beta=beta)
            ops.linear_dgrad(dqkv[:, nh * hd:], self.span(names[1], names[2]), dh)
        else:
            def wgrad():
                if all(rgs):
                    ops.linear_wgrad(dqkv, gs["h"], self.ar.grad_span(names[0], names[2]), beta=beta)
                elif rgs[0] and rgs[1]:  # e.g. last-layer vlm v_proj frozen (pizero.py:231)
                    ops.linear_wgrad(dqkv[:, : (nh + 1) * hd], gs["h"], self.ar.grad_span(names[0], names[1]),
                                     beta=beta)
                else:
                    for n, rgk, c0, c1 in zip(names, rgs, (0, nh * hd, (nh + 1) * hd), (nh * hd, (nh + 1) * hd, W)):
                        if rgk:
                            ops.linear_wgrad(dqkv[:, c0:c1], gs["h"], self.gw(n), beta=beta)

            # adapters: v = dqkv B2 over all three projections (a skipped layer's dQ columns are exactly zero, so its
            # q adapter gets the zero gradient the reference gives it) and the general input gradient
            self._dgrad(names, gs["h"], gs["u_qkv"], dqkv, self.qkv_w(p), dh, beta, wgrad=wgrad)
        dxn = torch.empty(M, g.hid, device=dev, dtype=BF16)
        self._norm_bwd(A, g, dh, x, gs["r"], l, "in_", dxn, dXm.get(g.name), beta)
        dX[g.name] = dxn

    def _joint_layers_backward(self, groups, dX, pos, cnt, B, sv, beta):
        d = self.d
        L, Lp, nh, hd = d.L, d.Lp, d.nh, d.hd
        dev = next(v for v in dX.values() if v is not None).device
        delta = dP = dS = None
        # the non-vlm group (action expert, 320 rows at micro-batch 64) runs its MLP / o_proj / q|k|v backward
        # on a second stream while the vlm group's run on the main stream; they meet at the joint attention
        # backward (events both ways).  Tensors one stream allocated and the other reads are record_stream'ed,
        # so the caching allocator never hands their memory out while the other stream may still read it.
        main = torch.cuda.current_stream(dev)
        side = None
        if self.expert_stream and len(groups) > 1 and dev.type == "cuda":
            side = self._side_stream(dev)
            side.wait_stream(main)
            for st in sv["joint"]:
                for g in groups:
                    if g.name != "vlm":
                        for t in st["g"][g.name].values():
                            if isinstance(t, torch.Tensor):
                                t.record_stream(side)
            for t in dX.values():
                if t is not None:
                    t.record_stream(side)
            for A in (sv.get("ada") or {}).values():
                A.mod.record_stream(side)
                A.dmod.record_stream(side)
        ada = sv.get("ada") or {}
        for l in reversed(range(d.nL)):
            st = sv["joint"][l]
            dQ = torch.empty(B, L, nh * hd, device=dev, dtype=BF16)
            dK = torch.empty(B, Lp, hd, device=dev, dtype=BF16)
            dV = torch.empty(B, Lp, hd, device=dev, dtype=BF16)
            dO = {}
            dXm = {}
            any_skip = False
            for g in groups:
                gs = st["g"][g.name]
                p = f"{g.prefix}{l}."
                if gs.get("skip"):
                    any_skip = True
                    continue
                with self._on(side, g):
                    self._mlp_oproj_backward(g, gs, p, dX, dO, dXm, beta, nh, hd, dev, ada.get(g.name), l)
                if side is not None and g.name != "vlm":
                    dO[g.name].record_stream(main)
            if side is not None:
                main.wait_stream(side)  # the expert dO for the joint attention backward
            if "lse" in st:
                # fused attention backward (skipped mixtures' outputs reach nothing: dO = 0)
                for g in groups:
                    if g.name not in dO:
                        dO[g.name] = torch.zeros(B * g.T, nh * hd, device=dev, dtype=BF16)
                if delta is None:
                    delta = torch.empty(B, L * nh, device=dev, dtype=F32)
                ops.flash_bwd(self._joint_flash(groups, st["Q"], st["K"], st["V"], st["O"], st["lse"], cnt, B, L,
                                                dO=dO, delta=delta, dq=dQ, dk=dK, dv=dV))
            else:
                Pm, tc, Qj, Kj, Vj = st["P"], st["tc"], st["Q"], st["K"], st["V"]
                dq_done = False
                if not isinstance(cnt, GeneralMask) and L <= 320 and hd == 256:
                    # dS in one kernel: dP = dO V^T in registers, delta and the soft-cap/softmax backward
                    # from the exported P / tanh(cap) (no fp32 dP tensor), then dQ = dS K in the same launch;
                    # a mixture without dO adds 0
                    if dS is None:
                        dS = torch.empty(B, L * nh, Lp, device=dev, dtype=BF16)
                    ops.flash_bwd_ds(self._joint_flash(groups, Qj, Kj, Vj, st["O"], None, cnt, B, L, dO=dO,
                                                       dq=dQ), Pm, tc, dS, Lp)
                    dq_done = True
                else:
                    if dP is None:
                        dP = torch.empty(B, L * nh, Lp, device=dev, dtype=F32)
                    if dS is None:
                        dS = torch.empty(B, L * nh, Lp, device=dev, dtype=BF16)
                    if any_skip:
                        dP.zero_()
                    for g in groups:
                        if g.name not in dO:
                            continue
                        ops.gemm(g.T * nh, L, hd, dO[g.name], hd, True, Vj, hd, True, dP[:, g.off * nh:], Lp,
                                 batch=B, sA=(g.T * nh * hd, 0), sB=(Lp * hd, 0), sC=(L * nh * Lp, 0))
                    ops.attn_softmax_bwd(Pm, dP, Lp, tc, dS, Lp, B * L * nh, L, 1.0 / math.sqrt(hd), 50.0)
                # dQ = dS K ; dK = dS^T Q ; dV = sum_g P_g^T dO_g
                if not dq_done:
                    ops.gemm(L * nh, hd, Lp, dS, Lp, True, Kj, hd, False, dQ, hd, batch=B, sA=(L * nh * Lp, 0),
                             sB=(Lp * hd, 0), sC=(L * nh * hd, 0))
                ops.gemm(Lp, hd, L * nh, dS, Lp, False, Qj, hd, False, dK, hd, batch=B, sA=(L * nh * Lp, 0),
                         sB=(L * nh * hd, 0), sC=(Lp * hd, 0))
                first = True
                # the shortest mixture first (the action expert's 5 rows x heads: its launch then writes dV
                # instead of reading + writing it, and the long vlm launch accumulates in its epilogue)
                for g in sorted(groups, key=lambda g: g.T):
                    if g.name not in dO:
                        continue
                    ops.gemm(Lp, hd, g.T * nh, Pm[:, g.off * nh:], Lp, False, dO[g.name], hd, False, dV, hd, batch=B,
                             sA=(L * nh * Lp, 0), sB=(g.T * nh * hd, 0), sC=(Lp * hd, 0), beta=not first)
                    first = False
                if first:
                    dV.zero_()
            if side is not None:  # dQ / dK / dV of the joint attention backward feed the expert's q|k|v backward
                side.wait_stream(main)
                for t in (dQ, dK, dV):
                    t.record_stream(side)
            for g in groups:
                with self._on(side, g):
                    self._qkv_backward(g, st["g"][g.name], f"{g.prefix}{l}.", dQ, dK, dV, dX, dXm, pos, B, L, Lp, beta,
                                       nh, hd, dev, ada.get(g.name), l)
            # the layer's expert gradients were produced on the side stream: the reducer's communication stream waits
            # for both streams before it reads them (the compute streams keep running; no main <- side join per layer)
            self._chk(f"joint bwd layer {l}", dO=dO, dS=dS, dQ=dQ, dK=dK, dV=dV, dX=dX)
            self._notify("joint", l, (side,) if side is not None else ())
        if side is not None:
            main.wait_stream(side)
            for t in dX.values():
                if t is not None:
                    t.record_stream(main)
        sv.pop("_jkv_token", None)  # the joint K/V buffers are free for the next forward
        return dX

    # ================================== frozen VLM: expert-only joint layers ==
    @contextlib.contextmanager
    def _bf16_weights(self):
        """the inference routes on bf16 weights only (the forward-only VLM pass of training never reads fp8 codes)"""
        f8, self.f8 = self.f8, None
        try:
            yield
        finally:
            self.f8 = f8

    def _expert_kernels_ok(self, T):
        """pz_expert_attn_fwd / _bwd take head_dim 256 and up to 1024 query rows per sample; other shapes run the GEMM
        attention path on the expert's query rows"""
        return self.d.hd == 256 and T * self.d.nh <= 1024

    def _expert_layers_train(self, groups, X, pos, cnt, B, save, Kall, Vall, draws=1):
        """The expert groups' joint layers against the K/V rows [0, P) that the forward-only VLM pass left in
        Kall / Vall [nL, B, Lp, hd]: their q|k|v epilogue scatters their K/V into rows [P, P + T), their T * nh query
        rows per sample attend to all L keys (pz_expert_attn_fwd: O + log-sum-exp; outside its limits the GEMM path
        with its P / tanh exports on those rows), their activations are saved as in _joint_layers_train.

        draws > 1 (several flow draws per observation): B and cnt count (observation, draw) pairs, every
        row-wise stage runs on them unchanged, and Kall / Vall stay [nL, B / draws, Lp, hd].  A pair's own K/V go to
        compact [B, T, hd] buffers per layer and pz_expert_attn_fwd_shared reads rows [0, P) from the pair's
        observation; the GEMM path copies those rows into per-pair [B, Lp, hd] buffers first and runs as above."""
        d = self.d
        dev = X[groups[0].name].device
        L, Lp, nh, hd, P = d.L, d.Lp, d.nh, d.hd, d.P
        T = sum(g.T for g in groups)
        W = nh * hd
        kern = self._expert_kernels_ok(T)
        ada = save.get("ada")
        S = None
        layers = []
        for l in range(d.nL):
            last = l == d.nL - 1
            Qe = torch.empty(B, T, W, device=dev, dtype=BF16)
            Kj, Vj = Kall[l], Vall[l]
            if draws > 1 and not kern:  # per-pair copies of the observation's rows [0, P); pad rows zero
                Ks, Vs = Kj, Vj
                Kj = torch.zeros(B, Lp, hd, device=dev, dtype=BF16)
                Vj = torch.zeros(B, Lp, hd, device=dev, dtype=BF16)
                for s in range(draws):
                    ops.copy_rows(Ks, hd, Lp * hd, Kj[s:], hd, draws * Lp * hd, B // draws, P, hd)
                    ops.copy_rows(Vs, hd, Lp * hd, Vj[s:], hd, draws * Lp * hd, B // draws, P, hd)
            st = {"Q": Qe, "K": Kj, "V": Vj, "g": {}}
            if draws > 1 and kern:
                Ko = torch.empty(B, T, hd, device=dev, dtype=BF16)
                Vo = torch.empty(B, T, hd, device=dev, dtype=BF16)
                st["Ko"], st["Vo"] = Ko, Vo
            for g in groups:
                if draws > 1 and kern:
                    self._pre_attn_train(g, l, X, pos, st, Qe, Ko, Vo, dev, ada, Lq=T, qoff=g.off - P, Lk=T,
                                         koff=g.off - P)
                else:
                    self._pre_attn_train(g, l, X, pos, st, Qe, Kj, Vj, dev, ada, Lq=T, qoff=g.off - P)
            if kern:
                Oall = torch.empty(B * T, W, device=dev, dtype=BF16)
                lse = torch.empty(B, T * nh, device=dev, dtype=F32)
                if draws > 1:
                    ops.expert_attn_fwd_shared(Qe, T, 0, Kj, Vj, Ko, Vo, draws, Oall, lse, B, nh, T, L,
                                               1.0 / math.sqrt(hd), 50.0, cnt, P, d.C, P)
                else:
                    ops.expert_attn_fwd(Qe, T, 0, Kj, Vj, Oall, lse, B, nh, T, L, 1.0 / math.sqrt(hd), 50.0, cnt, P,
                                        d.C, P)
                st["lse"], st["Oall"] = lse, Oall
                if len(groups) == 1:
                    Os = {groups[0].name: Oall}
                else:  # untied proprio / action: each mixture's o_proj reads its own rows
                    Os = {g.name: torch.empty(B * g.T, W, device=dev, dtype=BF16) for g in groups}
                    for g in groups:
                        ops.copy_rows(Oall[g.off - P:], W, T * W, Os[g.name], W, g.T * W, B, g.T, W)
            else:
                if S is None:
                    S = torch.empty(B, T * nh, Lp, device=dev, dtype=F32)
                Os = {g.name: torch.empty(B * g.T, W, device=dev, dtype=BF16) for g in groups}
                live = [g for g in groups if not (last and g.skip_last)]
                st["P"], st["tc"] = self._attn_gemm(Qe, Kj, Vj, S, Os, live, P, T, L, "full", cnt, B, export=True)
            for g in groups:
                gs = st["g"][g.name]
                if last and g.skip_last:
                    X[g.name] = None
                    gs["skip"] = True
                    continue
                X[g.name] = self._post_attn(g, l, X[g.name], Os[g.name], ada.get(g.name) if ada else None, gs)
            layers.append(st)
            self._chk(f"expert fwd layer {l} (frozen VLM)", Q=Qe, O=Os, lse=st.get("lse"), P=st.get("P"), X=X)
        save["joint"] = layers
        return X

    def _expert_layers_backward(self, groups, dX, pos, cnt, B, sv, beta, draws=1):
        """Backward of _expert_layers_train: per layer the expert groups' MLP / o_proj backward, the attention backward
        for their query rows (pz_expert_attn_bwd: dQ and the dK / dV of key rows [P, P + T) only; outside its limits
        the backward GEMMs on those rows), and their q|k|v backward.  Nothing is computed for the VLM rows.
        draws > 1: B and cnt count pairs; pz_expert_attn_bwd_shared writes dK / dV into compact [B, T, hd] buffers."""
        d = self.d
        L, Lp, nh, hd, P = d.L, d.Lp, d.nh, d.hd, d.P
        dev = next(v for v in dX.values() if v is not None).device
        T = sum(g.T for g in groups)
        W = nh * hd
        ada = sv.get("ada") or {}
        scale = 1.0 / math.sqrt(hd)
        dP = dS = None
        for l in reversed(range(d.nL)):
            st = sv["joint"][l]
            dQ = torch.empty(B, T, W, device=dev, dtype=BF16)
            own = "Ko" in st  # several draws on the kernels: compact dK / dV, the pair's rows from 0
            Lk, k0 = (T, 0) if own else (Lp, P)
            dK = torch.empty(B, Lk, hd, device=dev, dtype=BF16)
            dV = torch.empty(B, Lk, hd, device=dev, dtype=BF16)
            dO, dXm = {}, {}
            for g in groups:
                gs = st["g"][g.name]
                if not gs.get("skip"):
                    self._mlp_oproj_backward(g, gs, f"{g.prefix}{l}.", dX, dO, dXm, beta, nh, hd, dev, ada.get(g.name), l)
            Qe, Kj, Vj = st["Q"], st["K"], st["V"]
            if "lse" in st:
                if len(groups) == 1:
                    dOall = dO[groups[0].name]
                else:  # a skipped mixture's output reaches nothing: dO = 0
                    dOall = torch.zeros(B * T, W, device=dev, dtype=BF16)
                    for g in groups:
                        if g.name in dO:
                            ops.copy_rows(dO[g.name], W, g.T * W, dOall[g.off - P:], W, T * W, B, g.T, W)
                if own:
                    ops.expert_attn_bwd_shared(Qe, T, 0, Kj, Vj, st["Ko"], st["Vo"], draws, st["Oall"], st["lse"], dOall,
                                               dQ, dK, dV, P, T, B, nh, T, L, scale, 50.0, cnt, P, d.C, P)
                else:
                    ops.expert_attn_bwd(Qe, T, 0, Kj, Vj, st["Oall"], st["lse"], dOall, dQ, dK[:, P:], dV[:, P:], P, T, B,
                                        nh, T, L, scale, 50.0, cnt, P, d.C, P)
            else:
                Pm, tc = st["P"], st["tc"]
                if dP is None:
                    dP = torch.empty(B, T * nh, Lp, device=dev, dtype=F32)
                    dS = torch.empty(B, T * nh, Lp, device=dev, dtype=BF16)
                if len(dO) < len(groups):
                    dP.zero_()
                for g in groups:
                    if g.name in dO:
                        ops.gemm(g.T * nh, L, hd, dO[g.name], hd, True, Vj, hd, True, dP[:, (g.off - P) * nh:], Lp,
                                 batch=B, sA=(g.T * nh * hd, 0), sB=(Lp * hd, 0), sC=(T * nh * Lp, 0))
                ops.attn_softmax_bwd(Pm, dP, Lp, tc, dS, Lp, B * T * nh, L, scale, 50.0)
                ops.gemm(T * nh, hd, Lp, dS, Lp, True, Kj, hd, False, dQ, hd, batch=B, sA=(T * nh * Lp, 0),
                         sB=(Lp * hd, 0), sC=(T * nh * hd, 0))
                ops.gemm(Lp, hd, T * nh, dS, Lp, False, Qe, hd, False, dK, hd, batch=B, sA=(T * nh * Lp, 0),
                         sB=(T * nh * hd, 0), sC=(Lp * hd, 0))
                first = True
                for g in groups:
                    if g.name in dO:
                        ops.gemm(Lp, hd, g.T * nh, Pm[:, (g.off - P) * nh:], Lp, False, dO[g.name], hd, False, dV, hd,
                                 batch=B, sA=(T * nh * Lp, 0), sB=(g.T * nh * hd, 0), sC=(Lp * hd, 0), beta=not first)
                        first = False
            for g in groups:
                self._qkv_backward(g, st["g"][g.name], f"{g.prefix}{l}.", dQ, dK, dV, dX, dXm, pos, B, T, Lk, beta, nh,
                                   hd, dev, ada.get(g.name), l, qoff=g.off - P, koff=g.off - P + k0)
            self._chk(f"expert bwd layer {l} (frozen VLM)", dO=dO, dQ=dQ, dK=dK[:, k0:k0 + T], dV=dV[:, k0:k0 + T], dX=dX)
            self._notify("joint", l)
        sv.pop("_jkv_token", None)  # the joint K/V buffers are free for the next forward
        return dX

    # ============================================================ training ==
    def _expert_rows(self, Xp, e3, B, sp):
        """{group: input rows} of the expert groups from the proprio rows Xp [B*C, aH] times sp and the action rows e3
        [B*H, aH] times sqrt(hidden) (joint_model.py:355): a sample's proprio then action rows in the tied group, else
        one group each.  sp None: Xp is scaled already (an untied proprio group takes it as it is)."""
        d = self.d
        sa = math.sqrt(d.aH)
        if self.m._tied:
            T = d.C + d.H
            Xe = torch.empty(B * T, d.aH, device=e3.device, dtype=BF16)
            ops.copy_rows(Xp, d.aH, d.C * d.aH, Xe, d.aH, T * d.aH, B, d.C, d.aH, scale=sp or 1.0)
            ops.copy_rows(e3, d.aH, d.H * d.aH, Xe[d.C:], d.aH, T * d.aH, B, d.H, d.aH, scale=sa)
            return {"expert": Xe}
        if sp is not None:
            Xs = torch.empty_like(Xp)
            ops.copy_rows(Xp, d.aH, 0, Xs, d.aH, 0, 1, B * d.C, d.aH, scale=sp)
            Xp = Xs
        Xa = torch.empty_like(e3)
        ops.copy_rows(e3, d.aH, 0, Xa, d.aH, 0, 1, B * d.H, d.aH, scale=sa)
        return {"proprio": Xp, "action": Xa}

    def _expert_rows_bwd(self, dX, B, dpe, de3):
        """inverse of _expert_rows: the expert groups' input gradients into dpe [B*C, aH] and de3 [B*H, aH]"""
        d = self.d
        sa = math.sqrt(d.aH)
        if "expert" in dX:
            T = d.C + d.H
            ops.copy_rows(dX["expert"], d.aH, T * d.aH, dpe, d.aH, d.C * d.aH, B, d.C, d.aH, scale=sa)
            ops.copy_rows(dX["expert"][d.C:], d.aH, T * d.aH, de3, d.aH, d.H * d.aH, B, d.H, d.aH, scale=sa)
        else:
            ops.copy_rows(dX["proprio"], d.aH, 0, dpe, d.aH, 0, 1, B * d.C, d.aH, scale=sa)
            ops.copy_rows(dX["action"], d.aH, 0, de3, d.aH, 0, 1, B * d.H, d.aH, scale=sa)

    def train_forward(self, ids, pix, cnt, pos, proprios, actions, t, x0, save, prefix_len=None, draws=1):
        """pizero.py:607-661: returns fp32 loss [1]; ``save`` collects activations.  ``prefix_len`` (int32 [B] on the
        device): rows h < prefix_len[b] are fed clean (psi = bf16(x1), time 1) and carry no loss; None
        launches exactly the kernels of a run without the option.

        With nothing trainable in the VLM (train_vlm: False; PiZero._vlm_needs_grad() false) and the block mask, the
        frozen-VLM pass runs (``vlm_forward_only``): SigLIP, the projector and the vlm mixture forward-only
        on the bf16 inference routes into the joint K/V buffers (no VLM activation and no SigLIP state is saved), then
        the expert groups alone with their activations saved.  A GeneralMask keeps the full joint pass.

        ``draws`` = S > 1 (flow_samples_per_observation; the frozen-VLM pass only): ids, pix, cnt and
        pos["vlm"] hold the observations, proprios / actions / t / x0 / prefix_len and the expert positions hold the
        S pairs of each, pair e = b * S + s.  The prefill runs once, on the observations; the loss is the mean over
        all pairs -- the loss and gradients of this pass on the batch with every observation repeated S times."""
        d = self.d
        if d.ada and prefix_len is not None:
            raise NotImplementedError(PREFIX_ADAPTIVE_MSG)
        dev = pix.device
        nobs = ids.shape[0]
        B = nobs * draws  # (observation, draw) pairs: the batch of every expert stage
        tied = self.m._tied
        frozen = self.vlm_forward_only and not isinstance(cnt, GeneralMask) and not self.m._vlm_needs_grad()
        if draws < 1 or (draws > 1 and not frozen):
            raise ValueError(DRAWS_FROZEN_MSG if draws > 1 else f"draws must be >= 1, got {draws}")
        if frozen:
            sv_v = Xv = None
            Kall, Vall = self._joint_kv(nobs, d.Lp, dev, save)
            with self._bf16_weights():
                self.prefill(ids, pix, cnt, pos["vlm"], None, None, Kall, Vall, with_proprio=False)
            if draws > 1:  # the expert attention's prefix counts, per pair
                cnt = cnt.repeat_interleave(draws).contiguous()
        else:
            sv_v = {}
            img = self.siglip_forward(pix, sv_v)
            Xv = self.embed_prefix(ids, img)
        prop = proprios.reshape(B * d.C, d.Pd).to(BF16)
        pe = torch.empty(B * d.C, d.aH, device=dev, dtype=BF16)
        ops.small_linear(prop, self.w("proprio_encoder.weight"), pe, bias=self.w("proprio_encoder.bias"))
        psi = torch.empty(B * d.H, d.A, device=dev, dtype=BF16)
        ops.flow_psi(x0, actions, t, psi, d.sig_min, prefix_len=prefix_len)
        e3 = self.action_embed(psi, t, save, prefix_len)
        X = self._expert_rows(pe, e3, B, math.sqrt(d.aH))
        if not frozen:
            X = {"vlm": Xv, **X}
        groups = self.groups(tied, active=("proprio", "action")) if frozen else self.groups(tied)
        if d.ada:
            # the time condition (pizero.py:634; no parameters, t is data: no gradient flows into it) and every
            # adaLN site's modulation rows of the step, one GEMM per expert group
            cond = torch.empty(B, d.tH, device=dev, dtype=BF16)
            ops.time_embed(t, cond, d.tmax, ref_bf16=d.time_bf16)
            save["cond"] = cond
            save["ada"] = {g.name: Ada(self, g, cond) for g in groups if g.name != "vlm"}
        if frozen:
            X = self._expert_layers_train(groups, X, pos, cnt, B, save, Kall, Vall, draws)
        else:
            X = self._joint_layers_train(groups, X, pos, cnt, B, save)
        ag, Tg = groups[-1].name, groups[-1].T
        aoff = d.C if tied else 0
        Xl = X[ag]
        ya = torch.empty_like(Xl)
        ra = torch.empty(Xl.shape[0], device=dev, dtype=F32)
        self._norm_fwd(save["ada"][ag] if d.ada else None, groups[-1], Xl, "norm", "", ya, ra)
        v = torch.empty(B * Tg, 8, device=dev, dtype=BF16)  # columns 0..A-1 written and read (8: 16-B rows)
        ops.small_linear(ya, self.w("action_decoder.weight"), v, bias=self.w("action_decoder.bias"))
        loss = torch.empty(1, device=dev, dtype=F32)
        ops.flow_loss(v[aoff:], 8, Tg * 8, x0, actions, loss, None, None, B, d.H, d.A, d.sig_min,
                      prefix_len=prefix_len)
        save.update(sv_v=sv_v, ids=ids, cnt=cnt, pos=pos, B=B, prop=prop, pe=pe, Xl=Xl, ya=ya, ra=ra,
                    x0=x0, x1=actions, v=v, ag=ag, aoff=aoff, Tg=Tg, groups=groups, prefix_len=prefix_len,
                    frozen=frozen, draws=draws)
        self._chk("train fwd head (action norm, decoder, flow loss)", embed=Xv, ya=ya, v=v, loss=loss)
        return loss

    def train_backward(self, sv, grad_loss, beta):
        """Backward of train_forward; grad_loss: device fp32 [1] (d loss)."""
        d = self.d
        B = sv["B"]
        dev = sv["v"].device
        Tg, aoff = sv["Tg"], sv["aoff"]
        ws = self.colsum_ws(2 * d.aH)
        # loss + decoder
        dv = torch.zeros(B * Tg, 8, device=dev, dtype=BF16)
        tmp = torch.empty(1, device=dev, dtype=F32)
        ops.flow_loss(sv["v"][aoff:], 8, Tg * 8, sv["x0"], sv["x1"], tmp, dv[aoff:], grad_loss, B, d.H, d.A, d.sig_min,
                      prefix_len=sv.get("prefix_len"))
        R = B * Tg
        if self.rg("action_decoder.weight"):
            ops.small_gemm(d.A, d.aH, R, dv, 1, 8, sv["ya"], d.aH, 1, self.gw("action_decoder.weight"), d.aH, beta=beta)
        if self.rg("action_decoder.bias"):
            ops.colsum(dv[:, : d.A], self.gw("action_decoder.bias"), ws, beta=beta)
        dya = torch.empty(R, d.aH, device=dev, dtype=BF16)
        ops.small_gemm(R, d.aH, d.A, dv, 8, 1, self.w("action_decoder.weight"), d.aH, 1, dya, d.aH)
        dXl = torch.empty_like(dya)
        ada = sv.get("ada") or {}
        for A in ada.values():  # sites that feed nothing (an untied proprio's last layer and final norm) stay 0
            A.dmod = torch.zeros_like(A.mod)
        groups = sv["groups"]
        self._norm_bwd(ada.get(sv["ag"]), groups[-1], dya, sv["Xl"], sv["ra"], "norm", "", dXl, None, beta)
        self._chk("train bwd head", dv=dv, dya=dya, dXl=dXl)
        dX = {g.name: None for g in groups}
        dX[sv["ag"]] = dXl
        if sv.get("frozen"):
            dX = self._expert_layers_backward(groups, dX, sv["pos"], sv["cnt"], B, sv, beta, sv.get("draws", 1))
        else:
            dX = self._joint_layers_backward(groups, dX, sv["pos"], sv["cnt"], B, sv, beta)
        if ada:
            # the expert's layer-0 backward is complete: every conditioning Linear's gradient (the arena block that
            # follows the expert layers) before the encoders' notification
            for A in ada.values():
                A.weight_grads(sv["cond"], self.colsum_ws(A.mod.shape[1]), beta)
        # expert embeddings (joint_model.py:355 scale) -> encoders
        dpe = torch.empty(B * d.C, d.aH, device=dev, dtype=BF16)
        de3 = torch.empty(B * d.H, d.aH, device=dev, dtype=BF16)
        self._expert_rows_bwd(dX, B, dpe, de3)
        if self.rg("proprio_encoder.weight"):
            ops.small_gemm(d.aH, d.Pd, B * d.C, dpe, 1, d.aH, sv["prop"], d.Pd, 1, self.gw("proprio_encoder.weight"),
                           d.Pd, beta=beta)
        if self.rg("proprio_encoder.bias"):
            ops.colsum(dpe, self.gw("proprio_encoder.bias"), ws, beta=beta)
        ae = "action_encoder."
        if self.rg(ae + "linear_3.weight"):
            ops.linear_wgrad(de3, sv["ae_e2"], self.gw(ae + "linear_3.weight"), beta=beta)
        if self.rg(ae + "linear_3.bias"):
            ops.colsum(de3, self.gw(ae + "linear_3.bias"), ws, beta=beta)
        de2 = torch.empty_like(de3)
        ops.linear_dgrad(de3, self.w(ae + "linear_3.weight"), de2)
        ops.act_bwd(de2, sv["ae_pre"], de2, None, PZ_EPI_SILU)
        if self.rg(ae + "linear_2.weight"):
            ops.linear_wgrad(de2, sv["ae_cat"], self.gw(ae + "linear_2.weight"), beta=beta)
        if self.rg(ae + "linear_2.bias"):
            ops.colsum(de2, self.gw(ae + "linear_2.bias"), ws, beta=beta)
        if d.ada:  # no time concat: linear_2's input gradient is linear_1's output gradient
            de1 = torch.empty_like(de3)
            ops.linear_dgrad(de2, self.w(ae + "linear_2.weight"), de1)
        else:
            dcat = torch.empty(B * d.H, 2 * d.aH, device=dev, dtype=BF16)
            ops.linear_dgrad(de2, self.w(ae + "linear_2.weight"), dcat)
            de1 = torch.empty_like(de3)
            ops.split_time_grad(dcat, de1, B * d.H, d.aH)
        if self.rg(ae + "linear_1.weight"):
            ops.small_gemm(d.aH, d.A, B * d.H, de1, 1, d.aH, sv["ae_psi"], d.A, 1, self.gw(ae + "linear_1.weight"), d.A,
                           beta=beta)
        if self.rg(ae + "linear_1.bias"):
            ops.colsum(de1, self.gw(ae + "linear_1.bias"), ws, beta=beta)
        self._notify("encoders", -1)
        # VLM prefix -> projector -> SigLIP
        if not sv.get("frozen") and self.m._vlm_needs_grad():
            dimg = torch.empty(B * d.n_img, d.gH, device=dev, dtype=BF16)
            ops.embed_merge_bwd(sv["ids"], dX["vlm"], dimg, d.n_img, d.image_token, 1.0)
            self._chk("train bwd embed-merge", dimg=dimg)
            self.siglip_backward(sv["sv_v"], dimg, beta)
        self._chk("train bwd end (gradient arena)", grad=self.ar.grad)
        if self.post_backward is not None:
            self.post_backward()

    # ================================================== JointModel alone ==
    def joint_train(self, embeds, pos, cnt, dout, beta=False):
        """JointModel.forward + backward alone (joint_model.py:328-383) on given embeddings -- the
        harness of config C5 (3 images + chunk 50, which the reference composes at this level since
        its PiZero takes one image per sample).  embeds: {"vlm": [B, P, gH], "proprio": [B, C, aH],
        "action": [B, H, aH]} bf16 (scaled by sqrt(hidden) here, joint_model.py:348-355); dout: d(loss)
        wrt the final-normed action hidden states [B, H, aH].  Accumulates parameter gradients into
        the gradient arena and returns (action hidden [B, H, aH] bf16, {name: d embeds})."""
        d = self.d
        Ev, Ep, Ea = embeds["vlm"], embeds["proprio"], embeds["action"]
        B = Ev.shape[0]
        dev = Ev.device
        if not self.m._tied:
            raise NotImplementedError("joint_train expects tie_action_proprio_weights() (pizero.py:262-264)")
        if d.ada:
            raise NotImplementedError("joint_train takes no time condition: run the adaLN expert through PiZero.forward")
        Xv = torch.empty(B * d.P, d.gH, device=dev, dtype=BF16)
        ops.copy_rows(Ev.reshape(B * d.P, d.gH), d.gH, 0, Xv, d.gH, 0, 1, B * d.P, d.gH, scale=math.sqrt(d.gH))
        T = d.C + d.H
        Xe = self._expert_rows(Ep.reshape(B * d.C, d.aH), Ea.reshape(B * d.H, d.aH), B, math.sqrt(d.aH))
        groups = self.groups(True)
        save = {}
        X = self._joint_layers_train(groups, {"vlm": Xv, **Xe}, pos, cnt, B, save)
        Xl = X["expert"]
        ya = torch.empty_like(Xl)
        ra = torch.empty(Xl.shape[0], device=dev, dtype=F32)
        self._norm_fwd(None, groups[-1], Xl, "norm", "", ya, ra)
        dya = torch.zeros_like(ya)  # proprio rows are not outputs (joint_model.py:375-380 skip list)
        ops.copy_rows(dout.reshape(B * d.H, d.aH).to(BF16), d.aH, d.H * d.aH, dya[d.C:], d.aH, T * d.aH, B, d.H, d.aH)
        dXl = torch.empty_like(dya)
        self._norm_bwd(None, groups[-1], dya, Xl, ra, "norm", "", dXl, None, beta)
        dX = self._joint_layers_backward(groups, {"vlm": None, "expert": dXl}, pos, cnt, B, save, beta)
        dEv = torch.empty(B, d.P, d.gH, device=dev, dtype=BF16)
        ops.copy_rows(dX["vlm"], d.gH, 0, dEv.view(B * d.P, d.gH), d.gH, 0, 1, B * d.P, d.gH, scale=math.sqrt(d.gH))
        dEp = torch.empty(B, d.C, d.aH, device=dev, dtype=BF16)
        dEa = torch.empty(B, d.H, d.aH, device=dev, dtype=BF16)
        self._expert_rows_bwd(dX, B, dEp.view(B * d.C, d.aH), dEa.view(B * d.H, d.aH))
        out = torch.empty(B, d.H, d.aH, device=dev, dtype=BF16)
        ops.copy_rows(ya[d.C:], d.aH, T * d.aH, out.view(B * d.H, d.aH), d.aH, d.H * d.aH, B, d.H, d.aH)
        return out, {"vlm": dEv, "proprio": dEp, "action": dEa}

    # ============================================================ inference ==
    def decode_attn_ok(self):
        """pz_decode_attn for the denoise attention (head_dim 256, up to 1024 query rows per sample in 32-row
        tiles: C4's 4 tokens x 8 heads = one tile, C5's 50 x 8 = 13 tiles with 2 key chunks per workgroup --
        measured 23.5 vs 24.3 ms per C5 chunk against the key-split flash kernel); other shapes use
        the flash kernel + combine"""
        d = self.d
        return d.hd == 256 and d.H * d.nh <= 1024

    def _qkv_w_f8(self, p):
        """(q|k|v weights, fp8 scale): the e4m3 codes and their scale when prepare_fp8() holds them for layer p,
        else (bf16 weights, None)"""
        f = self.f8.get(p + "self_attn.q_proj.weight") if self.f8 else None
        return (self.qkv_w(p), None) if f is None else (f[0], f[1])

    def few_rows(self, M, K):
        """row counts the few-row GEMM kernels take with the RMSNorm fused (pz_gemm skinny paths:
        M <= 16 with K % 32 == 0, 16 < M <= 64 with K % 64 == 0)"""
        return (M <= 16 and K % 32 == 0) or (M <= 64 and K % 64 == 0)

    def gemv_ok(self, M, K):
        """few-row GEMV kernels (pz_gemv.hip): M <= 8 rows, K % 512 == 0 (PZ_GEMV=0 disables)"""
        return M <= 8 and K % 512 == 0 and os.environ.get("PZ_GEMV", "1") != "0"

    def _proprio_rows(self, proprios, B, dev):
        """proprio encoder output times sqrt(hidden) (pizero.py:100, joint_model.py:355): [B*C, aH] bf16"""
        d = self.d
        prop = proprios.reshape(B * d.C, d.Pd).to(BF16)
        pe = torch.empty(B * d.C, d.aH, device=dev, dtype=BF16)
        ops.small_linear(prop, self.w("proprio_encoder.weight"), pe, bias=self.w("proprio_encoder.bias"))
        Xp = torch.empty(B * d.C, d.aH, device=dev, dtype=BF16)
        ops.copy_rows(pe, d.aH, 0, Xp, d.aH, 0, 1, B * d.C, d.aH, scale=math.sqrt(d.aH))
        return Xp

    def _qkv_infer(self, g, l, x, pos, Q, Kj, Vj, B, Lq, qo, ko, route, A=None, kv_only=False, gemv=None, cs=None):
        """One group's input norm + q|k|v projection + RoPE (table cs; default: the group's own) of joint layer l in an
        inference pass, its rows
        scattered to query tokens [qo, qo + g.T) of Q [B, Lq, nh*hd] and to rows [ko, ko + g.T) of the K / V caches.
        kv_only (the last layer of a prefix pass): only K/V are consumed downstream (pizero.py:451, skipped
        post-attn).  gemv: take the one-launch GEMV (default: wherever gemv_ok and the norm is the Gemma RMSNorm).
        route names what the passes do differently with the same rows (unmeasured against each other):
          "prefix"  prefill: fp8 codes from the norm for > 64 rows, the 8-phase GEMM with the RoPE epilogue
          "decode"  denoise_step: <= 64 rows through the few-row kernels with the norm fused
          "plain"   text_forward, the adaLN expert: norm, bf16 GEMM, RoPE split -- never fp8 codes"""
        d = self.d
        nh, hd, Lp = d.nh, d.hd, Kj.shape[1]
        p = f"{g.prefix}{l}."
        M, K = x.shape
        key = p + "self_attn.q_proj.weight"
        nw = None if A is not None else (self.w(p + "input_layernorm.weight"), d.rms_eps)
        if gemv is None:
            gemv = A is None and self.gemv_ok(M, K)

        def rope():  # (a table not built yet is built where the pass first rotates, after its norm)
            return cs if cs is not None else self.rope(g.theta)

        if gemv:  # one launch: RMSNorm + q|k|v GEMV + RoPE + Q / K-cache / V-cache scatter
            if kv_only:
                ops.gemv_qkv_rope(x, self.span(p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"), pos,
                                  rope(), None, Kj, Vj, g.T, 0, hd, Lq, qo, Lp, ko, norm=nw)
            else:
                ops.gemv_qkv_rope(x, self.qkv_w(p), pos, rope(), Q, Kj, Vj, g.T, nh, hd, Lq, qo, Lp, ko, norm=nw)
            return
        qkv = None
        # the decode pass alone fuses the norm of its 9..64 non-GEMV rows; the prefix pass normalises them in a launch
        if route == "decode" and self.few_rows(M, K):
            W, sc = self._qkv_w_f8(p)
            if self.fuse_qkv_rope and ops.gemm_qkv_rope(x, W, pos, rope(), Q, Kj, Vj, g.T, nh, hd, Lq, qo, Lp, ko,
                                                        norm=nw, w_scale=sc):
                return  # C5's 50-row chunk: RMSNorm + skinny-64 q|k|v (bf16 or W8A16) + RoPE + scatter in one launch
            qkv = torch.empty(M, (nh + 2) * hd, device=x.device, dtype=BF16)
            self.lin(x, key, self.qkv_w(p), qkv, norm=nw)  # RMSNorm fused into the q|k|v GEMM
        # the prefix pass alone takes fp8 codes straight from the norm (C5); > 64 decode rows are quantised inside lin
        elif route == "prefix" and not kv_only and self.w8a8_in(key, M, K):
            qkv = torch.empty(M, (nh + 2) * hd, device=x.device, dtype=BF16)
            self.lin(self.norm_codes(x, *nw), key, self.qkv_w(p), qkv)  # q|k|v W8A8 on the fp8 MFMA
        else:
            h = torch.empty_like(x)
            self._norm_fwd(A, g, x, l, "in_", h)
            # the prefix pass alone has the 8-phase GEMM rotate and scatter: many rows (B >= 16), bf16 weights
            if route == "prefix" and not kv_only and self.fuse_qkv_rope and not (self.f8 and key in self.f8) and \
                    ops.gemm_qkv_rope(h, self.qkv_w(p), pos, rope(), Q, Kj, Vj, g.T, nh, hd, Lq, qo, Lp, ko):
                return
            qkv = torch.empty(M, (nh + 2) * hd, device=x.device, dtype=BF16)
            if kv_only:
                kv = torch.empty(M, 2 * hd, device=x.device, dtype=BF16)
                ops.linear(h, self.span(p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"), kv)
                ops.copy_rows(kv, 2 * hd, 0, qkv[:, nh * hd:], (nh + 2) * hd, 0, 1, M, 2 * hd)
                Q = None
            elif route == "plain":  # text generation keeps bf16 q|k|v weights with fp8 codes prepared
                ops.linear(h, self.qkv_w(p), qkv)
            else:
                self.lin(h, key, self.qkv_w(p), qkv)
        ops.qkv_rope_split(qkv, pos, rope(), Q, Kj, Vj, B, g.T, nh, 1, hd, Lq, qo, Lp, ko)

    @_merged_weights
    def prefill(self, ids, pix, cnt, vpos, ppos, proprios, kcache, vcache, with_proprio=True):
        """pizero.py:430-451: SigLIP + prefix pass over {vlm, proprio}; writes post-RoPE K/V caches.
        with_proprio False (the adaLN expert, whose proprio rows depend on t): the vlm mixture alone -- its rows
        attend only to vlm rows, so their K/V need neither t nor proprio."""
        d = self.d
        dev = pix.device
        B = ids.shape[0]
        nh, hd = d.nh, d.hd
        L1 = d.P + (d.C if with_proprio else 0)
        img = self.siglip_forward(pix, None)
        groups = self.groups(self.m._tied, active=("vlm", "proprio") if with_proprio else ("vlm",))
        X, pos = {"vlm": self.embed_prefix(ids, img)}, {"vlm": vpos}
        if with_proprio:
            X[groups[1].name], pos[groups[1].name] = self._proprio_rows(proprios, B, dev), ppos
        Q = torch.empty(B, L1, nh * hd, device=dev, dtype=BF16)
        S = None
        flash = self.infer_flash and not isinstance(cnt, GeneralMask)
        for l in range(d.nL):
            last = l == d.nL - 1
            Kj, Vj = kcache[l], vcache[l]
            for g in groups:
                self._qkv_infer(g, l, X[g.name], pos[g.name], Q, Kj, Vj, B, L1, g.off, g.off,
                                "prefix", kv_only=last)
            if last:
                break
            Os = {g.name: torch.empty(B * g.T, nh * hd, device=dev, dtype=BF16) for g in groups}
            if flash:  # fused attention over the L1 prefix keys
                fa = self._attn_flash_infer(Q, Kj, Vj, [(g.off, g.T, Os[g.name]) for g in groups], L1, L1, 0, cnt, B)
                if self.f8 is not None and hd == 256:
                    self._flash_f8(fa, Q, Kj, Vj, B, L1 * nh, L1)  # fp8 MFMA attention (C5, configs[4])
                else:
                    ops.flash_fwd(fa)
            else:
                if S is None:
                    S = torch.empty(B, L1 * nh, d.Lp, device=dev, dtype=F32)
                self._attn_gemm(Q, Kj, Vj, S, Os, groups, 0, L1, L1, "itp", cnt, B)
            for g in groups:
                X[g.name] = self._post_attn(g, l, X[g.name], Os[g.name], plain=not flash)
        return kcache, vcache

    # ========================================================= text generation ==
    @_merged_weights
    def text_forward(self, ids, pix, pos, kc, vc, start, n_img, maxpos):
        """PiZero.infer_text (pizero.py:559-593): the vlm mixture alone through all layers (cache_mode
        "append", no last-layer skip, the all-zeros text mask of pizero.py:336-365 -> no masking), the
        new tokens ids [B, q] written at cache rows [start, start + q) of kc / vc [nL, B, Lcap, hd] and
        attending to rows [0, start + q); then the vlm final norm (if the mixture has one) and the
        lm_head tied to embed_tokens (pizero.py:106-112).  pix / n_img: images of a prefill (None / 0
        for decode steps).  maxpos: an upper bound of the positions (sizes the RoPE table).  Returns bf16
        logits [B, q, vocab]."""
        d = self.d
        B, q = ids.shape
        dev = ids.device
        nh, hd = d.nh, d.hd
        Lcap = kc.shape[2]
        self.fp8_refresh()
        nk = start + q
        table = self.w("embed_tokens.weight")
        img = table if pix is None else self.siglip_forward(pix, None)
        X = torch.empty(B * q, d.gH, device=dev, dtype=BF16)
        ops.embed_merge(ids, table, img, X, n_img, d.image_token, d.pad_token, math.sqrt(d.gH), 1.0)
        g, = self.groups(False, active=("vlm",), text=q)
        Q = torch.empty(B, q, nh * hd, device=dev, dtype=BF16)
        O = torch.empty(B * q, nh * hd, device=dev, dtype=BF16)
        few = self.gemv_ok(B * q, d.gH) and q * nh <= 32  # (pz_decode_attn's one 32-row tile)
        cs = self.rope(g.theta, maxpos)
        x = X
        for l in range(d.nL):
            Kl, Vl = kc[l], vc[l]
            self._qkv_infer(g, l, x, pos, Q, Kl, Vl, B, q, 0, start, "plain", gemv=few, cs=cs)
            if few:
                ops.decode_attn(Q, q, 0, Kl, Vl, O, B, nh, q, nk, 1.0 / math.sqrt(hd), 50.0, None, 0, 0, start)
            else:
                ops.flash_fwd(ops.flash_args(
                    B, 1, q * nh, nk, hd, Q, (hd, q * nh * hd, 0), Kl, (hd, Lcap * hd, 0), Vl, (hd, Lcap * hd, 0),
                    [(0, O, q * nh * hd, hd)], 0, None, 1.0 / math.sqrt(hd), cap=50.0, mask_mode=0,
                    rows_per_token=nh, key_split=True))
            x = self._post_attn(g, l, x, O)
        nw = "joint_model.mixtures.vlm.norm.weight"
        if nw in self.ar.slots:
            y = torch.empty_like(x)
            ops.rmsnorm(x, self.w(nw), y, None, d.rms_eps)
            x = y
        logits = torch.empty(B * q, table.shape[0], device=dev, dtype=BF16)
        ops.linear(x, table, logits)
        return logits.view(B, q, -1)

    def _flash_f8(self, fa, Q, K, V, B, nq, nk):
        """the joint attention of fa on the fp8 MFMA: Q rows / key rows quantised per row, V^T per head dim
        (pz_fp8_quant_rows, pz_fp8_quant_vt), then pz_flash_fwd_f8 (+ its key-split combine)"""
        dev = Q.device
        hd, Lp = self.d.hd, K.shape[1]
        qc = torch.empty(B * nq, hd, device=dev, dtype=torch.uint8)
        qs = torch.empty(B * nq, device=dev, dtype=F32)
        kc = torch.empty(B * Lp, hd, device=dev, dtype=torch.uint8)
        ks = torch.empty(B * Lp, device=dev, dtype=F32)
        vt = torch.empty(B, hd, (nk + 127) // 128 * 128, device=dev, dtype=torch.uint8)
        vs = torch.empty(B, hd, device=dev, dtype=F32)
        ops.fp8_quant_attn(Q.reshape(B * nq, hd), K.reshape(B * Lp, hd), V, B, nk, qc, qs, kc, ks, vt, vs)
        ops.flash_fwd_f8(fa, qc, qs, kc, ks, Lp, vt, vs)

    def _attn_flash_infer(self, Q, K, V, outs, Lq, nk, tok0, cnt, B):
        """pz_flash_args for the inference attention: queries = Lq tokens starting at joint token tok0
        (rows token*nh + head of Q [B, Lq*nh, hd]), keys = the first nk cached tokens; outs =
        [(token offset, T, O [B*T, nh*hd])] in token order."""
        d = self.d
        nh, hd, Lp = d.nh, d.hd, K.shape[1]
        return ops.flash_args(
            B, 1, Lq * nh, nk, hd, Q, (hd, Lq * nh * hd, 0), K, (hd, Lp * hd, 0), V, (hd, Lp * hd, 0),
            [((off - tok0) * nh, O, T * nh * hd, hd) for off, T, O in outs], 0, None, 1.0 / math.sqrt(hd), cap=50.0,
            mask_mode=1, cnt=cnt, prefix=d.P, cond=d.C, rows_per_token=nh, mask_row0=tok0 * nh,
            key_split=True)

    @_merged_weights
    def denoise_step(self, action, t, apos, cnt, kcache, vcache, B, prefix_len=None):
        """One Euler step of pizero.py:461-481 against the cached vlm+proprio K/V.  ``prefix_len`` (int32 [B], DESIGN
        7f): rows h < prefix_len[b] of ``action`` are embedded with time 1 and not updated, on both glue routes, with
        the launch count of a step without it."""
        d = self.d
        dev = action.device
        nh, hd, L = d.nh, d.hd, d.L
        # the step's glue in two launches (pz_action_in / pz_action_out, bit-identical to cast + Linear + time
        # embedding and RMSNorm + decoder + Euler; PZ_FUSED_GLUE=0: the separate kernels)
        glue = (d.aH <= 1024 and d.aH % 8 == 0 and d.A <= 8 and os.environ.get("PZ_FUSED_GLUE", "1") != "0" and
                all(self.w(k).data_ptr() % 16 == 0 for k in ("joint_model.mixtures.action.norm.weight",
                                                             "action_decoder.weight")))
        if glue:
            cat = torch.empty(B * d.H, 2 * d.aH, device=dev, dtype=BF16)
            ops.action_in(action, self.w("action_encoder.linear_1.weight"), self.w("action_encoder.linear_1.bias"), t,
                          cat, B, d.H, d.aH, d.tmax, ref_bf16=d.time_bf16, prefix_len=prefix_len)
            sq = math.sqrt(d.aH)
            if sq.is_integer() and (int(sq) & (int(sq) - 1)) == 0:
                # the joint model's sqrt(hidden) input scaling is a power of two (32 at hidden 1024): folded into the
                # last encoder Linear as alpha with a pre-scaled bias -- 2^k (acc + b) rounds exactly like rounding
                # first and scaling the bf16 after (the copy_rows launch it replaces), so the bits are unchanged
                x = self._action_embed_tail(cat, alpha=sq)
            else:
                e3 = self._action_embed_tail(cat)
                x = torch.empty_like(e3)
                ops.copy_rows(e3, d.aH, 0, x, d.aH, 0, 1, B * d.H, d.aH, scale=sq)
        else:
            psi = torch.empty(B * d.H, d.A, device=dev, dtype=BF16)
            ops.cast_to_bf16(action, psi)
            e3 = self.action_embed(psi, t, None, prefix_len)
            x = torch.empty_like(e3)
            ops.copy_rows(e3, d.aH, 0, x, d.aH, 0, 1, B * d.H, d.aH, scale=math.sqrt(d.aH))
        g, = self.groups(self.m._tied, active=("action",))
        Q = torch.empty(B, d.H, nh * hd, device=dev, dtype=BF16)
        O = torch.empty(B * d.H, nh * hd, device=dev, dtype=BF16)
        S = None
        flash = self.infer_flash and not isinstance(cnt, GeneralMask)
        for l in range(d.nL):
            Kj, Vj = kcache[l], vcache[l]
            self._qkv_infer(g, l, x, apos, Q, Kj, Vj, B, d.H, 0, g.off, "decode")
            if not flash:
                if S is None:
                    S = torch.empty(B, d.H * nh, d.Lp, device=dev, dtype=F32)
                self._attn_gemm(Q, Kj, Vj, S, {g.name: O}, [g], g.off, d.H, L, "act", cnt, B)
            elif self.decode_attn_ok():  # one workgroup per (head, sample), no key split / combine launch
                ops.decode_attn(Q, d.H, 0, Kj, Vj, O, B, nh, d.H, L, 1.0 / math.sqrt(hd), 50.0, cnt, d.P, d.C, g.off)
            else:  # fused attention over every cached key
                ops.flash_fwd(self._attn_flash_infer(Q, Kj, Vj, [(g.off, d.H, O)], d.H, L, g.off, cnt, B))
            x = self._post_attn(g, l, x, O, plain=not flash)
        if glue:
            ops.action_out(x, self.w("joint_model.mixtures.action.norm.weight"), d.rms_eps,
                           self.w("action_decoder.weight"), self.w("action_decoder.bias"), action, t, B, d.H,
                           1.0 / d.steps, prefix_len=prefix_len)
            return
        y = torch.empty_like(x)
        ops.rmsnorm(x, self.w("joint_model.mixtures.action.norm.weight"), y, None, d.rms_eps)
        v = torch.empty(B * d.H, 8, device=dev, dtype=BF16)
        ops.small_linear(y, self.w("action_decoder.weight"), v[:, : d.A], bias=self.w("action_decoder.bias"))
        ops.euler_step(action, v, 8, d.H * 8, t, B, d.H, d.A, 1.0 / d.steps, prefix_len=prefix_len)

    @_merged_weights
    def denoise_step_ada(self, action, t, Xp, pos, cnt, kcache, vcache, B):
        """One Euler step of the adaLN expert with the semantics of the reference's infer_action_naive
        (pizero.py:492-557): the proprio AND action rows of every sample run again with cond(t) -- the proprio K/V
        depend on t, so only the vlm K/V are cached -- under the block mask (proprio -> vlm + proprio, action ->
        all).  Unfused sites: adaptive norm launches, plain q|k|v GEMM + RoPE split, the flash kernel with the query
        rows starting at token P (or GEMM + softmax), the adaptive final norm + decoder + Euler tail.  Xp: the proprio
        rows, already times sqrt(hidden)."""
        d = self.d
        dev = action.device
        nh, hd, L = d.nh, d.hd, d.L
        T = d.C + d.H
        cond = torch.empty(B, d.tH, device=dev, dtype=BF16)
        ops.time_embed(t, cond, d.tmax, ref_bf16=d.time_bf16)
        groups = self.groups(self.m._tied, active=("proprio", "action"))
        ada = {g.name: Ada(self, g, cond) for g in groups}
        psi = torch.empty(B * d.H, d.A, device=dev, dtype=BF16)
        ops.cast_to_bf16(action, psi)
        X = self._expert_rows(Xp, self.action_embed(psi, t, None), B, None)
        Q = torch.empty(B, T, nh * hd, device=dev, dtype=BF16)
        S = None
        flash = self.infer_flash and not isinstance(cnt, GeneralMask)
        for l in range(d.nL):
            last = l == d.nL - 1
            Kj, Vj = kcache[l], vcache[l]
            for g in groups:
                self._qkv_infer(g, l, X[g.name], pos[g.name], Q, Kj, Vj, B, T, g.off - d.P, g.off,
                                "plain", A=ada[g.name])
            # (an untied proprio mixture's last-layer output feeds nothing: computed with the rest -- every query row
            # belongs to an output group -- and dropped)
            live = [g for g in groups if not (last and g.skip_last)]
            Os = {g.name: torch.empty(B * g.T, nh * hd, device=dev, dtype=BF16) for g in groups}
            if flash:
                ops.flash_fwd(self._attn_flash_infer(Q, Kj, Vj, [(g.off, g.T, Os[g.name]) for g in groups], T, L, d.P,
                                                     cnt, B))
            else:
                if S is None:
                    S = torch.empty(B, T * nh, d.Lp, device=dev, dtype=F32)
                self._attn_gemm(Q, Kj, Vj, S, Os, live, d.P, T, L, "act", cnt, B)
            for g in live:
                X[g.name] = self._post_attn(g, l, X[g.name], Os[g.name], ada[g.name])
        ga = groups[-1]  # the group that holds the action rows: the tied group's follow its proprio rows
        aoff = ga.T - d.H
        y = torch.empty_like(X[ga.name])
        self._norm_fwd(ada[ga.name], ga, X[ga.name], "norm", "", y)
        v = torch.empty(B * ga.T, 8, device=dev, dtype=BF16)
        ops.small_linear(y, self.w("action_decoder.weight"), v[:, : d.A], bias=self.w("action_decoder.bias"))
        ops.euler_step(action, v[aoff:], 8, ga.T * 8, t, B, d.H, d.A, 1.0 / d.steps)

    @_merged_weights
    def denoise_step_guided(self, action, t, Xp, pos, cnt, kcache, vcache, B, guide, k):
        """Euler step k of the loop guided toward the previous chunk:

            v = expert(A_t, t);  e = w (.) (target - (A_t + (1 - t) v));  g = e + (1 - t) (dv/dA_t)^T e
            A_t += dt (v + coef[k] g);  t += dt

        guide = (target fp32 [B, H, A], w fp32 [B, H], coef fp32 [steps]) on the device.  The expert rows of every
        sample (its proprio rows again, then the action rows: the frozen-VLM training pass, _expert_layers_train) run
        forward with saved activations against the cached vlm K/V, their own K/V scattered into the cache rows as
        denoise_step does; pz_rtc_seed turns v into the backward seed; the training backward then runs down to the
        action encoder's input with every weight-gradient launch switched off (_dgrad_only; the proprio rows' input
        gradient is dropped), and pz_rtc_euler applies the update.  Xp: the proprio rows times sqrt(hidden)."""
        d = self.d
        dev = action.device
        target, w, coef = guide
        groups = self.groups(self.m._tied, active=("proprio", "action"))
        ga = groups[-1]  # the group that holds the action rows: the tied group's follow its proprio rows
        aoff = ga.T - d.H
        R = B * ga.T
        save = {}
        psi = torch.empty(B * d.H, d.A, device=dev, dtype=BF16)
        ops.cast_to_bf16(action, psi)
        X = self._expert_rows(Xp, self.action_embed(psi, t, save), B, None)
        prev, self._dgrad_only = self._dgrad_only, True
        try:
            X = self._expert_layers_train(groups, X, pos, cnt, B, save, kcache, vcache)
            Xl = X[ga.name]
            ya = torch.empty_like(Xl)
            ra = torch.empty(R, device=dev, dtype=F32)
            self._norm_fwd(None, ga, Xl, "norm", "", ya, ra)
            v = torch.empty(R, 8, device=dev, dtype=BF16)
            wd = self.w("action_decoder.weight")
            ops.small_linear(ya, wd, v, bias=self.w("action_decoder.bias"))
            e = torch.empty(B, d.H, d.A, device=dev, dtype=F32)
            dv = torch.empty(R, 8, device=dev, dtype=BF16)
            ops.rtc_seed(action, v[aoff:], 8, ga.T * 8, target, w, t, e, dv, ga.T, aoff)
            # the backward of train_backward from dv down to de1, input gradients only
            dya = torch.empty(R, d.aH, device=dev, dtype=BF16)
            ops.small_gemm(R, d.aH, d.A, dv, 8, 1, wd, d.aH, 1, dya, d.aH)
            dXl = torch.empty_like(dya)
            self._norm_bwd(None, ga, dya, Xl, ra, "norm", "", dXl, None, False)
            dX = {g.name: None for g in groups}
            dX[ga.name] = dXl
            dX = self._expert_layers_backward(groups, dX, pos, cnt, B, save, False)
            dpe = torch.empty(B * d.C, d.aH, device=dev, dtype=BF16)
            de3 = torch.empty(B * d.H, d.aH, device=dev, dtype=BF16)
            self._expert_rows_bwd(dX, B, dpe, de3)
            ae = "action_encoder."
            de2 = torch.empty_like(de3)
            self._dgrad_gemm(de3, self.w(ae + "linear_3.weight"), de2)
            ops.act_bwd(de2, save["ae_pre"], de2, None, PZ_EPI_SILU)
            dcat = torch.empty(B * d.H, 2 * d.aH, device=dev, dtype=BF16)
            self._dgrad_gemm(de2, self.w(ae + "linear_2.weight"), dcat)
            de1 = torch.empty_like(de3)
            ops.split_time_grad(dcat, de1, B * d.H, d.aH)
            dA = torch.empty(B * d.H, 8, device=dev, dtype=BF16)  # columns 0..A-1 written and read
            ops.small_gemm(B * d.H, d.A, d.aH, de1, d.aH, 1, self.w(ae + "linear_1.weight"), d.A, 1, dA, 8)
            ops.rtc_euler(action, v[aoff:], 8, ga.T * 8, e, dA[:, : d.A], t, coef, k, 1.0 / d.steps)
        finally:
            self._dgrad_only = prev
        return dA

    def _guide_args(self, guide, B, cnt, prefix_len):
        """the refusals of the guided loop (by config key) and its device inputs"""
        d = self.d
        if d.ada:
            raise NotImplementedError(GUIDE_ADAPTIVE_MSG)
        if self.f8 is not None:
            raise NotImplementedError(GUIDE_FP8_MSG)
        if isinstance(cnt, GeneralMask):
            raise NotImplementedError(GUIDE_MASK_MSG)
        if prefix_len is not None:
            raise NotImplementedError(GUIDE_PREFIX_MSG)
        target, w, coef = guide
        for name, x, shape in (("target", target, (B, d.H, d.A)), ("w", w, (B, d.H)), ("coef", coef, (d.steps,))):
            if not (torch.is_tensor(x) and x.is_cuda and x.dtype == F32 and x.is_contiguous()
                    and tuple(x.shape) == shape):
                raise ValueError(f"infer_action: guide {name} must be a contiguous fp32 device tensor of shape {shape}")
        return target, w, coef

    @_merged_weights
    def infer_action(self, ids, pix, cnt, vpos, ppos, apos, proprios, noise, kcache, vcache, clip=True, prefix=None,
                     prefix_len=None, guide=None):
        """pizero.py:416-490.  With an adaLN expert both this and PiZero.infer_action_naive compute the naive
        semantics (pizero.py:492-557): the reference's cached infer_action raises AttributeError there ('NoneType'
        object has no attribute 'ndim' -- its prefill runs the proprio mixture without the time condition), and
        cannot work, since the proprio K/V depend on t.

        ``prefix`` (fp32 [B, H, A], normalised action units) with ``prefix_len`` (int32 [B] on the device):
        rows h < prefix_len[b] of the chunk are the committed actions -- written over the noise before the first step
        (one launch more per chunk), embedded with time 1, never updated, exempt from the final clamp and returned
        bit for bit; the other rows are denoised around them.  Neither given: exactly the launches of before.

        ``guide`` = (target fp32 [B, H, A] in normalised action units, w fp32 [B, H], coef fp32 [steps]) on the device
        (src/agent/chunking.py makes w and coef): every Euler step is steered toward ``target`` by the
        vector-Jacobian product of the denoiser (denoise_step_guided).  No row is frozen, every row is embedded with
        the sample's t, and the final clamp covers every row.  None: exactly the launches of before."""
        d = self.d
        B = ids.shape[0]
        dev = pix.device
        if (prefix is None) != (prefix_len is None):
            raise ValueError("infer_action: prefix and prefix_len go together")
        if guide is not None:
            guide = self._guide_args(guide, B, cnt, prefix_len)
        if prefix_len is not None and d.ada:
            raise NotImplementedError(PREFIX_ADAPTIVE_MSG)
        self.fp8_refresh()
        if d.ada:
            self.prefill(ids, pix, cnt, vpos, None, None, kcache, vcache, with_proprio=False)
            Xp = self._proprio_rows(proprios, B, dev)
            if self.m._tied:
                pos = {"expert": torch.cat([ppos, apos], dim=1).contiguous()}
            else:
                pos = {"proprio": ppos, "action": apos}
            if isinstance(cnt, GeneralMask):  # rows P.. of the caller's mask: [B, C + H, L] fp32
                m = torch.full((B, d.C + d.H, d.L), torch.finfo(F32).min, device=dev, dtype=F32)
                m[:, : d.C, : d.P + d.C] = cnt.itp[:, d.P:, :]
                m[:, d.C:, :] = cnt.act
                cnt = GeneralMask(itp=cnt.itp, act=m)
            step = functools.partial(self.denoise_step_ada, Xp=Xp, pos=pos)
        elif guide is not None:
            self.prefill(ids, pix, cnt, vpos, ppos, proprios, kcache, vcache)
            if self.m._tied:
                pos = {"expert": torch.cat([ppos, apos], dim=1).contiguous()}
            else:
                pos = {"proprio": ppos, "action": apos}
            Xp = self._proprio_rows(proprios, B, dev)
            action = noise.clone()
            t = torch.zeros(B, device=dev, dtype=F32)
            for k in range(d.steps):
                self.denoise_step_guided(action, t, Xp, pos, cnt, kcache, vcache, B, guide, k)
            if clip and d.clip is not None:
                ops.clamp_(action, -d.clip, d.clip)
            return action
        else:
            self.prefill(ids, pix, cnt, vpos, ppos, proprios, kcache, vcache)
            step = functools.partial(self.denoise_step, apos=apos)
            if prefix_len is not None:
                step = functools.partial(step, prefix_len=prefix_len)
        action = noise.clone()
        if prefix_len is not None:
            ops.action_prefix_init(action, prefix, prefix_len)
        t = torch.zeros(B, device=dev, dtype=F32)
        for _ in range(d.steps):
            step(action, t, cnt=cnt, kcache=kcache, vcache=vcache, B=B)
        if clip and d.clip is not None:
            ops.clamp_(action, -d.clip, d.clip, prefix_len=prefix_len)
        return action

    # --------------------------------------------------------------- hooks --
    hook = None  # called as hook(stage, layer, streams) when a layer's parameter gradients are final
    post_backward = None  # called once at the end of train_backward (gradient all-reduce flush)

    def _notify(self, stage, layer, streams=()):
        """streams: side streams (besides the current one) whose enqueued work produced some of those gradients"""
        if self.hook is not None and not self._dgrad_only:
            self.hook(stage, layer, streams)
