"""PiZero (Pi0 VLA) with the reference's nn.Module surface, executed natively on MI355X.

Drop-in for src/model/vla/pizero.py of shroglck/open-pi-zero:
  * same constructor ``PiZero(cfg, use_ddp=False)`` and ``PiZeroInference``;
  * same kwargs for ``forward`` (flow-matching loss, pizero.py:607-661),
    ``infer_action`` (KV-cached prefill + Euler denoising, pizero.py:416-490),
    ``infer_action_naive`` (pizero.py:492-557), mask/position builders
    (pizero.py:271-336), parameter groups / freezing / tying
    (pizero.py:114-264), ``load_pretrained_weights`` (pizero.py:160-222);
  * same state_dict keys (checkpoints load with strict=True).
Differences (all documented in DESIGN.md):
  * all weights live in one flat arena (pizero_native/arena.py) and every
    kernel of the path is a HIP kernel from libpizero_hip.so, launched by
    pizero_native/engine.py; ``loss.backward()`` runs the native backward and
    writes .grad views of the flat gradient arena;
  * RNG: ``noise=`` may be passed explicitly (parity tests); otherwise noise
    is drawn with torch.randn on the device like the reference;
  * ``torch.compile`` is unnecessary: wrapping is harmless but the native
    path is what runs.
"""

from __future__ import annotations

import logging
import math
from typing import Optional, Tuple

import torch
from torch import nn

from src.model.kv_cache import KVCache
from src.model.vla.modules import ActionEncoder, SinusoidalPosEmb
from src.utils.config import cfg_get, instantiate
from src.utils.decorator import NoSyncBase

log = logging.getLogger(__name__)


def _resolve(root, dotted):
    mod = root
    parts = dotted.split(".")
    for p in parts[:-1]:
        mod = mod[p] if isinstance(mod, (nn.ModuleDict,)) else (mod[int(p)] if isinstance(mod, nn.ModuleList) else getattr(mod, p))
    return mod, parts[-1]


def adaln_slots(prefix: str, n_layers: int, mode: str):
    """Modulation layout of one adaLN mixture (``prefix`` = "joint_model.mixtures.<name>."): the names of its
    time-conditioning Linears in arena order and the slot index of each site.  The biased Linears (every
    to_gamma, and for adaLN-Zero the two layer-scale gates) come first, then the bias-free to_beta, so one
    [B, time_hidden] x [time_hidden, nslots * hidden] GEMM gives every site's rows, one wgrad GEMM every weight
    gradient and one column sum over the first ``len(b)`` slots every bias gradient.
    Returns {"w": weight names, "b": bias names, "slot": {(layer | "norm", site): index}}."""
    zero = mode == "adaLN-Zero"
    w, b, beta, slot = [], [], [], {}

    def biased(key, name):
        slot[key] = len(w)
        w.append(prefix + name + ".weight")
        b.append(prefix + name + ".bias")

    for l in range(n_layers):
        p = f"layers.{l}."
        biased((l, "in_g"), p + "input_layernorm.to_gamma.0")
        biased((l, "post_g"), p + "post_attention_layernorm.to_gamma.0")
        if zero:
            biased((l, "post_z"), p + "post_adaptive_scale.to_adaln_zero_gamma")
            biased((l, "final_z"), p + "final_adaptive_scale.to_adaln_zero_gamma")
        beta += [((l, "in_b"), p + "input_layernorm.to_beta"), ((l, "post_b"), p + "post_attention_layernorm.to_beta")]
    biased(("norm", "g"), "norm.to_gamma.0")
    beta.append((("norm", "b"), "norm.to_beta"))
    for key, name in beta:
        slot[key] = len(w)
        w.append(prefix + name + ".weight")
    return {"w": w, "b": b, "slot": slot}


def flow_draws(B, H, A, t_shape, noise_shape=None, prefix_len_shape=None):
    """Number of flow draws per observation S (``flow_samples_per_observation``) that the shapes of
    PiZero.forward's ``t`` ([B] -> 1, [B, S] -> S), ``noise`` ([B, H, A] or [B, S, H, A]) and ``prefix_len`` ([B],
    broadcast over the draws, or [B, S]) ask for, for B observations; shapes that disagree are refused.  Shapes only:
    runs without a device."""
    key = "flow_samples_per_observation"
    t_shape = tuple(t_shape)
    if len(t_shape) not in (1, 2) or t_shape[0] != B or (len(t_shape) == 2 and t_shape[1] < 1):
        raise ValueError(f"t must be [B] or [B, S] ({key}: S >= 1 draws per observation) with B = {B}, got "
                         f"{list(t_shape)}")
    two = len(t_shape) == 2
    S = t_shape[1] if two else 1
    if noise_shape is not None:
        want = (B, S, H, A) if two else (B, H, A)
        if tuple(noise_shape) != want:
            raise ValueError(f"{key}: noise must be {list(want)} for t of shape {list(t_shape)} (one x0 per draw), got "
                             f"{list(noise_shape)}")
    if prefix_len_shape is not None and len(tuple(prefix_len_shape)) == 2 and tuple(prefix_len_shape) != (B, S):
        raise ValueError(f"{key}: prefix_len must be [B] (shared by an observation's draws) or [B, S] = [{B}, {S}], got "
                         f"{list(prefix_len_shape)}")
    return S


class _PiZeroLoss(torch.autograd.Function):
    """Whole-model autograd node: native forward, native backward into the grad arena."""

    @staticmethod
    def forward(ctx, anchor, model, batch):
        save = {}
        loss = model._engine().train_forward(save=save, **batch)
        ctx.model = model
        ctx.save = save
        return loss.view(())

    @staticmethod
    def backward(ctx, gloss):
        model = ctx.model
        beta = model._grads_live()
        gscale = gloss.reshape(1).to(torch.float32).contiguous()
        model._engine().train_backward(ctx.save, gscale, beta)
        ctx.save = None
        model._attach_grads()
        return None, None, None


class PiZero(nn.Module, NoSyncBase):
    def __init__(self, cfg, use_ddp: bool = False, *, device=None, dtype=None, init: str = "default"):
        super().__init__()
        self.cfg = cfg
        self.use_ddp = use_ddp
        self.vocab_size = cfg_get(cfg, "vocab_size")
        self.pad_token_id = cfg_get(cfg, "pad_token_id")
        self.image_token_index = cfg_get(cfg, "image_token_index")
        self.use_lm_head = cfg_get(cfg, "use_lm_head", False)
        self.max_image_text_tokens = cfg_get(cfg, "max_image_text_tokens", cfg_get(cfg, "max_seq_len"))
        self.num_proprio_tokens = cfg_get(cfg, "cond_steps")
        self.num_action_tokens = cfg_get(cfg, "horizon_steps")
        self.total_num_tokens = self.max_image_text_tokens + self.num_proprio_tokens + self.num_action_tokens
        self.image_text_hidden_size = cfg_get(cfg, "mixture.vlm.hidden_size")
        self.proprio_hidden_size = cfg_get(cfg, "mixture.proprio.hidden_size")
        self.action_hidden_size = cfg_get(cfg, "mixture.action.hidden_size")
        self.num_inference_steps = cfg_get(cfg, "num_inference_steps")
        self.horizon_steps = cfg_get(cfg, "horizon_steps")
        self.action_dim = cfg_get(cfg, "action_dim")
        self.proprio_dim = cfg_get(cfg, "proprio_dim")
        self.final_action_clip_value = cfg_get(cfg, "final_action_clip_value", None)
        self.flow_sig_min = cfg_get(cfg, "flow_sig_min", 0.001)
        self.action_expert_adaptive_mode = cfg_get(cfg, "action_expert_adaptive_mode", None)
        if self.action_expert_adaptive_mode not in (None, "adaLN", "adaLN-Zero"):
            raise ValueError("action_expert_adaptive_mode must be adaLN, adaLN-Zero or null, got "
                             f"{self.action_expert_adaptive_mode!r}")
        for mix in ("proprio", "action"):  # pizero.py:76-84 conditions both expert mixtures or neither
            if (cfg_get(cfg, f"mixture.{mix}.adaptive_mode", None) or None) != self.action_expert_adaptive_mode:
                raise ValueError(f"mixture.{mix}.adaptive_mode must equal action_expert_adaptive_mode "
                                 f"({self.action_expert_adaptive_mode!r})")
        ada = bool(self.action_expert_adaptive_mode)
        self._q4_type = self._quantize_type(cfg)  # None: bf16 base weights
        self._q4 = None  # pizero_native.quant4.Q4Store once quantize_base_() packed them
        with torch.device("meta"):
            self.embed_tokens = nn.Embedding(self.vocab_size, self.image_text_hidden_size, self.pad_token_id)
            self.vision_tower = instantiate(cfg_get(cfg, "vision"))
            self.multi_modal_projector = instantiate(cfg_get(cfg, "vision_projector"))
            self.joint_model = instantiate(cfg_get(cfg, "joint"))
            # adaLN: the time embedding conditions the expert's norms instead of the action encoder (pizero.py:76-84)
            self.action_encoder = ActionEncoder(self.action_dim, self.action_hidden_size, time_cond=not ada)
            self.time_hidden_size = cfg_get(cfg, "time_hidden_size") if ada else self.action_hidden_size
            self.time_embedding = SinusoidalPosEmb(self.time_hidden_size, cfg_get(cfg, "time_max_period"))
            self.proprio_encoder = nn.Linear(self.proprio_dim, self.proprio_hidden_size)
            self.action_decoder = nn.Linear(self.action_hidden_size, self.action_dim)
            if self.use_lm_head:  # optional text output (pizero.py:106-112), tied to embed_tokens
                self.lm_head = nn.Linear(self.image_text_hidden_size, self.vocab_size, bias=False)
        self._tied = False
        self._eng = None
        self._kv = None
        self._build_arena(torch.device(device or "cpu"), dtype or torch.float32, init=init)
        if self._q4_type and not self.has_lora:  # the reference's warning (train.py:90-93)
            log.warning("Quantizing VLM but not adding Lora weights, which means the VLM will be fully frozen!")
            for part in (self.vision_tower, self.multi_modal_projector, self.joint_model.mixtures["vlm"]):
                for p in part.parameters():
                    p.requires_grad = False

    @staticmethod
    def _quantize_type(cfg):
        """quantize: True -> "fp4" | "nf4" (``quantize_type``, default fp4), else None.  The 4-bit set is
        every Linear of SigLIP, the projector and the vlm mixture, so the three ``use_quantize`` copies the reference's
        config derives from ``quantize`` must agree, and the expert mixtures stay bf16."""
        keys = ("vision.use_quantize", "vision_projector.use_quantize", "joint.config.mixture.vlm.use_quantize")
        flags = [bool(cfg_get(cfg, k, False)) for k in keys]
        if any(flags) and not all(flags):
            raise NotImplementedError("use_quantize is set for " + ", ".join(k for k, f in zip(keys, flags) if f)
                                      + " but not for " + ", ".join(k for k, f in zip(keys, flags) if not f)
                                      + ": a partly quantised VLM is not supported, set quantize for all three")
        for mix in ("proprio", "action"):
            if cfg_get(cfg, f"joint.config.mixture.{mix}.use_quantize", False):
                raise NotImplementedError(f"mixture.{mix}.use_quantize: the action expert stays bf16; quantize covers "
                                          "SigLIP, the projector and the vlm mixture")
        if not all(flags):
            return None
        from pizero_native.quant4 import check_qtype

        return check_qtype(cfg_get(cfg, "quantize_type", "fp4") or "fp4")

    # ================================================================ arena ==
    def _layout(self):
        """(name, region) in backward-completion order (see pizero_native/arena.py)."""
        nL = self.joint_model.num_hidden_layers
        vL = len(self.vision_tower.vision_model.encoder.layers)
        mp = "joint_model.mixtures."
        out = []
        ada = self.action_expert_adaptive_mode

        def gemma(mix, l, region):
            p = f"{mp}{mix}.layers.{l}."
            for n in ("mlp.down_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
                      "post_attention_layernorm.weight", "self_attn.o_proj.weight", "self_attn.q_proj.weight",
                      "self_attn.k_proj.weight", "self_attn.v_proj.weight", "input_layernorm.weight"):
                if ada and mix != "vlm" and "layernorm" in n:
                    continue  # AdaptiveRMSNorm has no weight vector: its Linears sit in the modulation block
                out.append((p + n, region))

        out += [("action_decoder.weight", "action"), ("action_decoder.bias", "action")]
        if not ada:
            out.append((mp + "action.norm.weight", "action"))
            if not self._tied:
                out.append((mp + "proprio.norm.weight", "action"))
        for l in reversed(range(nL)):
            gemma("action", l, "action")
            if not self._tied:
                gemma("proprio", l, "action")
        if ada:
            # the time-conditioning Linears of a mixture, adjacent (adaln_slots): their gradients come from one wgrad
            # GEMM and one column sum issued when the expert's layer-0 backward completes, hence this position
            for mix in ("action",) if self._tied else ("action", "proprio"):
                sl = adaln_slots(f"{mp}{mix}.", nL, ada)
                out += [(n, "action") for n in sl["w"] + sl["b"]]
        for n in ("action_encoder.linear_3", "action_encoder.linear_2", "action_encoder.linear_1", "proprio_encoder"):
            out += [(n + ".weight", "action"), (n + ".bias", "action")]
        if hasattr(self.joint_model.mixtures["vlm"], "norm"):  # use_final_norm (text generation config)
            out.append((mp + "vlm.norm.weight", "vlm"))
        for l in reversed(range(nL)):
            gemma("vlm", l, "vlm")
        out += [("multi_modal_projector.linear.weight", "vlm"), ("multi_modal_projector.linear.bias", "vlm")]
        vt = "vision_tower.vision_model."
        out += [(vt + "post_layernorm.weight", "vlm"), (vt + "post_layernorm.bias", "vlm")]
        for i in reversed(range(vL)):
            p = f"{vt}encoder.layers.{i}."
            for n in ("mlp.fc2.weight", "mlp.fc2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "layer_norm2.weight",
                      "layer_norm2.bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                      "self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                      "self_attn.q_proj.bias", "self_attn.k_proj.bias", "self_attn.v_proj.bias",
                      "layer_norm1.weight", "layer_norm1.bias"):
                out.append((p + n, "vlm"))
        out += [(vt + "embeddings.position_embedding.weight", "vlm"),
                (vt + "embeddings.patch_embedding.weight", "vlm"), (vt + "embeddings.patch_embedding.bias", "vlm")]
        out += self._lora_layout()
        out += [("embed_tokens.weight", "frozen")]
        return out

    def _lora_layout(self):
        """The LoRA adapters, all in one arena region ("lora") behind the VLM weights, in backward-completion order.
        A (possibly fused) site's lora_A tensors are adjacent, then its lora_B tensors: the q|k|v (gate|up) A span
        is the stacked [S r, in] operand of one u = x A^T GEMM and of the input-gradient extension, the B span the
        stacked [N, r] rows the engine packs block-diagonally.  The base weights keep their places, so the fused
        q|k|v and gate|up weight spans are unchanged; the trainable parameters of a LoRA run form one contiguous
        run per optimizer group (minus the last vlm layer's frozen adapters) and one data-parallel bucket."""
        from src.model.lora import LoRALinear

        out = []
        for prefix, projs in self._vlm_linear_sites():
            mod, _ = _resolve(self, prefix + projs[0] + ".weight")
            if isinstance(mod, LoRALinear):
                out.extend((f"{prefix}{pr}.lora_A", "lora") for pr in projs)
                out.extend((f"{prefix}{pr}.lora_B", "lora") for pr in projs)
        return out

    def _vlm_linear_sites(self):
        """(prefix, projections) of every Linear site of SigLIP, the projector and the vlm mixture, fused sites as
        one entry, in backward-completion order: the sites that take LoRA adapters and (quantize: True) 4-bit weights"""
        nL = self.joint_model.num_hidden_layers
        for l in reversed(range(nL)):
            p = f"joint_model.mixtures.vlm.layers.{l}."
            yield p + "mlp.", ["down_proj"]
            yield p + "mlp.", ["gate_proj", "up_proj"]
            yield p + "self_attn.", ["o_proj"]
            yield p + "self_attn.", ["q_proj", "k_proj", "v_proj"]
        yield "multi_modal_projector.", ["linear"]
        vt = "vision_tower.vision_model.encoder.layers."
        for i in reversed(range(len(self.vision_tower.vision_model.encoder.layers))):
            yield f"{vt}{i}.mlp.", ["fc2"]
            yield f"{vt}{i}.mlp.", ["fc1"]
            yield f"{vt}{i}.self_attn.", ["out_proj"]
            yield f"{vt}{i}.self_attn.", ["q_proj", "k_proj", "v_proj"]

    def _q4_names(self):
        """names of the base weights that quantize: True packs to 4 bits, in arena order"""
        if not self._q4_type:
            return []
        return [f"{prefix}{pr}.weight" for prefix, projs in self._vlm_linear_sites() for pr in projs]

    @property
    def has_lora(self):
        return "lora" in self._arena.region_range

    def _build_arena(self, device, dtype, init="keep"):
        from pizero_native.arena import Arena

        entries, binds = [], {}
        for name, region in self._layout():
            mod, attr = _resolve(self, name)
            p = mod._parameters[attr]
            packed = self._q4 is not None and name in self._q4.w  # the module holds uint8 [n / 2, 1]
            entries.append((name, self._q4.w[name].shape if packed else tuple(p.shape), region, p))
            binds[name] = (mod, attr, p.requires_grad)
        self._arena = Arena(entries, device, dtype, side=frozenset(self._q4_names()), alloc_side=self._q4 is None)
        self._arena.bind(binds)
        self._tie_lm_head()
        self._pmap = {name: _resolve(self, name) for name, _ in self._layout()}
        if init == "default":
            self._init_weights()
        self._eng = None

    @torch.no_grad()
    def _init_weights(self):
        """Default init: U(+-1/sqrt(fan_in)) for Linear/Conv, N(0,1)->U for embeddings,
        LayerNorm (1, 0), Gemma RMSNorm 0 (modules.py:11)."""
        import zlib

        g = torch.Generator(device="cpu").manual_seed(0)
        for name in self._arena.order:
            v = self._arena.view(name)
            if name.endswith(".lora_B"):  # lora.py:176-179: B = 0, A = kaiming_uniform(a=sqrt(5)) = U(+-1/sqrt(in)) (below)
                v.zero_()
                continue
            if "to_adaln_zero_gamma" in name:  # AdaptiveLayerscale: weight 0, bias -2 (vla/modules.py:107-109)
                v.fill_(0.0 if name.endswith("weight") else -2.0)
                continue
            if "layer_norm" in name or "post_layernorm" in name:
                v.fill_(1.0 if name.endswith("weight") else 0.0)
                continue
            if (name.endswith("norm.weight") or "layernorm" in name) and "to_gamma" not in name and "to_beta" not in name:
                v.zero_()
                continue
            if name in ("embed_tokens.weight", "vision_tower.vision_model.embeddings.position_embedding.weight"):
                bound = 1.0
            else:
                owner = name.rsplit(".", 1)[0] + ".weight" if name.endswith(".bias") else name
                w = self._arena.view(owner)
                bound = 1.0 / math.sqrt(max(1, w[0].numel() if w.dim() > 1 else w.numel()))
            if v.device.type == "cuda":
                from pizero_native import ops

                ops.fill_uniform(v, zlib.crc32(name.encode()), 0.0, bound)
            else:
                v.copy_(torch.empty(v.shape, dtype=torch.float32).uniform_(-bound, bound, generator=g))

    def _apply(self, fn, recurse=True):
        """.to(device/dtype) converts the whole arena at once and rebinds the views."""
        if getattr(self, "_arena", None) is None:
            return super()._apply(fn, recurse)
        rg = {n: self._pmap[n][0]._parameters[self._pmap[n][1]].requires_grad for n in self._pmap}
        self._arena.apply(fn)
        if self._q4 is not None:
            self._q4.apply(fn)
            self._bind_packed()
        self._arena.bind({n: (m, a, rg[n]) for n, (m, a) in self._pmap.items()})
        self._tie_lm_head()
        self._eng = None
        self._kv = None
        return self

    def _tie_lm_head(self):
        """pizero.py:112: lm_head.weight IS embed_tokens.weight (one arena tensor, two state_dict keys)"""
        if getattr(self, "use_lm_head", False) and hasattr(self, "lm_head"):
            self.lm_head._parameters["weight"] = self.embed_tokens._parameters["weight"]

    def _param(self, name):
        m, a = self._pmap[name]
        return m._parameters[a]

    def _requires_grad(self, name):
        return self._param(name).requires_grad

    def _vlm_needs_grad(self):
        return any(self._param(n).requires_grad for n in self._arena.order
                   if self._arena.slots[n].region in ("vlm", "lora"))

    def _trainable_names(self):
        return [n for n in self._arena.order if self._param(n).requires_grad]

    def _grads_live(self):
        g = self._arena.grad
        for n in self._trainable_names():
            p = self._param(n)
            if p.grad is not None and g is not None and p.grad.data_ptr() == self._arena.view(n, g).data_ptr():
                return True
        return False

    def _attach_grads(self):
        g = self._arena.ensure_grad()
        for n in self._trainable_names():
            p = self._param(n)
            v = self._arena.view(n, g)
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                p.grad = v

    def _engine(self):
        if self._eng is None:
            from pizero_native.engine import Engine

            if self._arena.data.device.type != "cuda":
                raise RuntimeError("PiZero runs on the MI355X HIP path only: move the model to a GPU (.to('cuda'))")
            self.quantize_base_()
            self._eng = Engine(self)
            if getattr(self, "_fp8_infer", False):
                self._eng.prepare_fp8()
        return self._eng

    # ============================================================ 4-bit base ==
    @property
    def quantized(self):
        return bool(self._q4_type)

    @torch.no_grad()
    def quantize_base_(self):
        """quantize: True: pack every Linear weight of SigLIP, the projector and the vlm mixture to 4 bits
        (pz_q4_quantize + the nested step) and release their bf16 storage.  Called by TrainAgent / EvalAgent after the
        weights are loaded and by the first forward otherwise; a no-op without ``quantize`` and when already packed.
        Afterwards ``module.weight`` is the packed uint8 [n / 2, 1] tensor (bitsandbytes' Params4bit layout) and
        state_dict() carries the packed state; loading a bf16 ``weight`` quantises it."""
        if not self._q4_type or self._q4 is not None:
            return self
        ar = self._arena
        if ar.data.device.type != "cuda":
            raise RuntimeError("quantize_base_ runs the HIP quantiser: move the model to a GPU first (.to('cuda'))")
        if ar.data.dtype != torch.bfloat16:
            raise RuntimeError("quantize_base_ packs bf16 weights: call model.to(torch.bfloat16) first")
        from pizero_native.quant4 import Q4Store

        store = Q4Store(self._q4_type, ar.data.device)
        for n in self._q4_names():
            store.quantize(n, ar.view(n))
        self._q4 = store
        self._bind_packed()
        ar.drop_side()
        self._q4_changed()
        return self

    def _bind_packed(self):
        for n, q in self._q4.w.items():
            mod, attr = self._pmap[n]
            mod._parameters[attr] = nn.Parameter(q.packed.view(-1, 1), requires_grad=False)

    def _q4_changed(self):
        """the packed weights changed: everything keyed on the weight version (merged shadow, fp8 codes) is stale"""
        from torch.autograd.graph import increment_version

        increment_version(self._arena.data)
        if self._eng is not None and self._eng._q4 is not self._q4:
            self._eng = None

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        """nn.Module.state_dict; a packed Linear emits ``weight`` (uint8 [n / 2, 1]) followed by weight.absmax,
        weight.quant_map, weight.nested_absmax, weight.nested_quant_map and the weight.quant_state.bitsandbytes__*
        JSON blob -- the packed layout of bitsandbytes 0.45 as far as it can be restated without the package"""
        sd = super().state_dict(*args, destination=destination, prefix=prefix, keep_vars=keep_vars)
        if self._q4 is None:
            return sd
        items = list(sd.items())
        sd.clear()
        for k, v in items:
            sd[k] = v
            n = k[len(prefix):]
            if n in self._q4.w:
                for suf, t in self._q4.entries(n).items():
                    if suf:
                        sd[k + suf] = t if keep_vars else t.detach()
        return sd

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """nn.Module.load_state_dict.  With quantize: True a packed ``weight`` (uint8, with its weight.* tensors) is
        installed without requantising and a floating-point ``weight`` is quantised on load (before quantize_base_()
        it is simply copied, like every other tensor)."""
        if not self._q4_type:
            return super().load_state_dict(state_dict, strict=strict, assign=assign)
        qn = set(self._q4_names())
        sd, packed_in, float_in = {}, {}, {}
        for k, v in state_dict.items():
            base = k.split(".weight", 1)[0] + ".weight" if ".weight." in k else k
            if base in qn and (k != base or v.dtype == torch.uint8):
                packed_in.setdefault(base, {})[k[len(base):]] = v
            elif base in qn and self._q4 is not None:
                float_in[base] = v
            else:
                sd[k] = v
        if packed_in:
            self.quantize_base_()
            # quantize_base_ packed whatever the arena held; floating-point weights of this load are packed below
            float_in.update({k: sd.pop(k) for k in list(sd) if k in qn})
        handled = set(packed_in) | set(float_in)
        if handled:
            dev = self._arena.data.device
            for n, ent in packed_in.items():
                self._q4.install(n, self._arena.slots[n].shape, ent, dev)
            for n, v in float_in.items():
                shape = self._arena.slots[n].shape
                if tuple(v.shape) != tuple(shape):
                    raise RuntimeError(f"size mismatch for {n}: copying a param with shape {tuple(v.shape)} from "
                                       f"checkpoint, the shape in current model is {tuple(shape)}")
                self._q4.quantize(n, v.to(device=dev, dtype=torch.bfloat16).contiguous())
            self._bind_packed()
            self._q4_changed()
        res = super().load_state_dict(sd, strict=False, assign=assign)
        missing = [k for k in res.missing_keys if k not in handled]
        if strict and (missing or res.unexpected_keys):
            raise RuntimeError("Error(s) in loading state_dict for PiZero: missing keys "
                               f"{missing}, unexpected keys {list(res.unexpected_keys)}")
        res.missing_keys[:] = missing
        return res

    def use_fp8_inference(self, enabled: bool = True):
        """Config C5 (BASELINE.json configs[4], "fp8 MFMA attention/MLP"): run inference (infer_action,
        infer_text) with OCP e4m3 weights -- per-tensor scales -- for every Linear of SigLIP, the vlm
        mixture and the action expert: prefill MLP GEMMs W8A8 on the fp8 MFMA (per-row activation scales),
        prefill q|k|v / o projections and denoise rows W8A16.  Training never uses them.  The codes are a snapshot of the current weights:
        call again after the weights change.  An extension: the reference has no fp8 path."""
        if enabled and self.action_expert_adaptive_mode:
            from pizero_native.engine import FP8_ADAPTIVE_MSG

            raise NotImplementedError(FP8_ADAPTIVE_MSG)
        self._fp8_infer = bool(enabled)
        eng = self._engine()
        if enabled:
            eng.prepare_fp8()
        else:
            eng.f8 = None
        return self

    # ========================================================= param groups ==
    @property
    def action_expert_parameters(self):
        return (list(self.action_encoder.parameters()) + list(self.action_decoder.parameters())
                + list(self.proprio_encoder.parameters()) + list(self.joint_model.mixtures["action"].parameters()))

    @property
    def trainable_vlm_parameters(self):
        return (list(self.vision_tower.parameters()) + list(self.multi_modal_projector.parameters())
                + self.trainable_gemma_parameters)

    @property
    def lora_trainable_vlm_parameters(self):
        """pizero.py:131-142: every lora_ tensor of SigLIP and the projector, and the used ones of the vlm mixture"""
        return ([p for n, p in self.vision_tower.named_parameters() if "lora_" in n]
                + [p for n, p in self.multi_modal_projector.named_parameters() if "lora_" in n]
                + self.trainable_lora_gemma_parameters)

    @property
    def trainable_lora_gemma_parameters(self):
        return [p for n, p in self.joint_model.mixtures["vlm"].named_parameters()
                if not self._check_gemma_unused_parameter_by_name(n) and "lora_" in n]

    @property
    def trainable_gemma_parameters(self):
        return [p for n, p in self.joint_model.mixtures["vlm"].named_parameters()
                if not self._check_gemma_unused_parameter_by_name(n)]

    def _check_gemma_unused_parameter_by_name(self, name: str) -> bool:
        last = self.joint_model.num_hidden_layers - 1
        return (f"{last}.post" in name or f"{last}.mlp" in name or f"{last}.self_attn.o_proj" in name
                or f"{last}.self_attn.v_proj" in name)

    def load_pretrained_weights(self):
        """pizero.py:160-222: PaliGemma safetensors -> embed / vision / projector / Gemma."""
        import glob
        import os

        from safetensors import safe_open

        files = glob.glob(os.path.join(cfg_get(self.cfg, "pretrained_model_path"), "*.safetensors"))
        if not files:
            raise FileNotFoundError(f"no *.safetensors under {cfg_get(self.cfg, 'pretrained_model_path')}")
        sd = {}
        for f in files:
            with safe_open(f, framework="pt", device="cpu") as h:
                for k in h.keys():
                    t = h.get_tensor(k)
                    if "embed_tokens" in k:
                        sd[k.replace("language_model.model.embed_tokens.", "embed_tokens.")] = t
                    elif "vision_tower" in k:
                        sd[k] = t
                    elif "multi_modal_projector" in k:
                        sd[k] = t
                    elif "language_model.model" in k:
                        sd[k.replace("language_model.model.", "joint_model.mixtures.vlm.")] = t
        missing, _ = self.load_state_dict(sd, strict=False)
        log.info("Loaded pre-trained PaliGemma weights (%d tensors, %d keys not in checkpoint)", len(sd), len(missing))

    def freeze_non_lora_weights_in_vlm(self):
        """pizero.py:236-249: only the lora_ tensors of SigLIP, the projector and the vlm mixture stay trainable (every
        bias frozen); the last vlm layer's unused tensors are left as freeze_unused_weights set them."""
        for name, param in self.vision_tower.named_parameters():
            param.requires_grad = "lora_" in name
        for name, param in self.multi_modal_projector.named_parameters():
            param.requires_grad = "lora_" in name
        for name, param in self.joint_model.mixtures["vlm"].named_parameters():
            if not self._check_gemma_unused_parameter_by_name(name):
                param.requires_grad = "lora_" in name

    def freeze_unused_weights(self):
        self.embed_tokens.weight.requires_grad = False
        for name, param in self.joint_model.mixtures["vlm"].named_parameters():
            if self._check_gemma_unused_parameter_by_name(name):
                param.requires_grad = False

    def freeze_all_weights(self):
        for _, p in self.named_parameters():
            p.requires_grad = False

    def tie_action_proprio_weights(self):
        """pizero.py:262-264; the arena is repacked without the proprio copy."""
        self.joint_model.mixtures["proprio"] = self.joint_model.mixtures["action"]
        self._tied = True
        self._build_arena(self._arena.data.device, self._arena.data.dtype, init="keep")

    def build_text_cache(self):
        return KVCache()

    # ===================================================== input preparation ==
    def build_causal_mask_and_position_ids(self, attention_mask: torch.Tensor, dtype: torch.dtype):
        """pizero.py:271-324 (vectorised; same values)."""
        bsz = attention_mask.size(0)
        P, C, H = self.max_image_text_tokens, self.num_proprio_tokens, self.num_action_tokens
        L = self.total_num_tokens
        dev = attention_mask.device
        cnt = attention_mask.sum(1)
        i = torch.arange(L, device=dev)
        c = cnt[:, None, None]
        ii, jj = i[None, :, None], i[None, None, :]
        vlm = (ii < c) & (jj < c) & (ii < P)
        prefix = (ii >= P) & (jj < c)
        prop = (ii >= P) & (ii < P + C) & (jj >= P) & (jj < P + C)
        act = (ii >= P + C) & (jj >= P)
        allowed = vlm | prefix | prop | act
        mask = torch.where(allowed, torch.zeros((), dtype=dtype, device=dev),
                           torch.full((), torch.finfo(dtype).min, dtype=dtype, device=dev)).unsqueeze(1)
        vpos = torch.arange(1, P + 1, device=dev).repeat(bsz, 1)
        ppos = torch.arange(1, C + 1, device=dev).repeat(bsz, 1)
        apos = torch.arange(C + 1, C + H + 1, device=dev).repeat(bsz, 1)
        # built here from cnt: known block pattern (finfo.min absorbs), so forward() skips validation
        if torch.finfo(dtype).min <= -1e30:
            self._mask_remember([mask], cnt.to(torch.int32).contiguous())
        return mask, vpos, ppos, apos

    def split_full_mask_into_submasks(self, causal_mask):
        """pizero.py:326-336 (views); a validated full mask passes its prefix counts on to the pair."""
        n = self.max_image_text_tokens + self.num_proprio_tokens
        itp, am = causal_mask[..., :n, :n], causal_mask[..., -self.num_action_tokens:, :]
        spec = self._mask_lookup([causal_mask])
        if spec is not None:
            self._mask_remember([itp, am], spec)
        return itp, am

    def _prefix_counts(self, mask):
        """Per-sample image+text token count from the proprio row of the block mask."""
        P = self.max_image_text_tokens
        return (mask[:, 0, P, :P] == 0).sum(-1).to(torch.int32).contiguous()

    def _block_allowed(self, cnt, rows, ncols):
        """[B, len(rows), ncols] bool: the Pi0 block pattern of pizero.py:271-306 for prefix counts cnt."""
        P, C = self.max_image_text_tokens, self.num_proprio_tokens
        i = rows.view(1, -1, 1)
        j = torch.arange(ncols, device=cnt.device).view(1, 1, -1)
        c = cnt.view(-1, 1, 1).to(torch.int64)
        return torch.where(i < P, (i < c) & (j < c),
                           torch.where(i < P + C, (j < c) | ((j >= P) & (j < P + C)), (j < c) | (j >= P)))

    @staticmethod
    def _is_block(mask, allowed):
        """mask == 0 where allowed and <= -1e30 elsewhere (finfo.min of bf16/fp32, which absorbs any
        logit exactly like the block kernels' 'excluded' -- a fully masked row is then uniform)."""
        m = mask[:, 0]
        return bool(torch.where(allowed, m == 0, m <= -1e30).all())

    def _mask_spec(self, masks, rows_list):
        """Validate the caller's additive mask(s) once per new tensor: the Pi0 block
        pattern -> int32 per-sample prefix counts (the fused kernels regenerate the mask from them);
        anything else -> engine.GeneralMask (the GEMM+softmax path adds it like joint_model.py:271).
        The cache holds the mask tensors themselves (identity + version), so a freed-and-reused address
        can never alias a stale entry."""
        from pizero_native.engine import GeneralMask

        hit = self._mask_lookup(masks)
        if hit is not None:
            return hit
        itp = masks[0]
        P = self.max_image_text_tokens
        cnt = self._prefix_counts(itp) if itp.shape[2] > P else None
        ok = cnt is not None
        if ok:
            for m, rows in zip(masks, rows_list):
                if not self._is_block(m, self._block_allowed(cnt, rows, m.shape[-1])):
                    ok = False
                    break
        if ok:
            spec = cnt
        else:
            f = [m[:, 0].to(torch.float32).contiguous() for m in masks]
            spec = GeneralMask(full=f[0]) if len(f) == 1 else GeneralMask(itp=f[0], act=f[1])
            log.warning("attention mask is not the Pi0 block pattern: using the general additive-mask path")
        self._mask_remember(masks, spec)
        return spec

    _MASK_CACHE = 6

    def _mask_lookup(self, masks):
        for ms, vers, spec in self.__dict__.get("_mask_cache", ()):
            if len(ms) == len(masks) and all(a is b and a._version == v for a, b, v in zip(ms, masks, vers)):
                return spec
        return None

    def _mask_remember(self, masks, spec):
        cache = [e for e in self.__dict__.get("_mask_cache", []) if not all(a is b for a, b in zip(e[0], masks))]
        cache.append((tuple(masks), tuple(m._version for m in masks), spec))
        self.__dict__["_mask_cache"] = cache[-self._MASK_CACHE:]

    def block_prefix_counts(self, image_text_proprio_mask, action_mask):
        """int32 prefix counts for the static hipGraph path, which supports the Pi0 block mask only."""
        dev = self._dev()
        itp, am = image_text_proprio_mask.to(dev), action_mask.to(dev)
        L1 = itp.shape[2]
        spec = self._mask_spec([itp, am], [torch.arange(L1, device=dev), torch.arange(L1, L1 + am.shape[2], device=dev)])
        if not isinstance(spec, torch.Tensor):
            raise ValueError("the hipGraph inference path needs the Pi0 block mask (pizero.py:271-306); "
                             "call infer_action eagerly for a general mask")
        return spec

    def _dev(self):
        return self._arena.data.device

    def _cat_pos(self, *pos):
        return torch.cat([p.to(self._dev(), torch.int64) for p in pos], dim=1).contiguous()

    # ============================================================== forward ==
    def psi_t(self, x, x1, t):
        t = t[:, None, None]
        return (1 - (1 - self.flow_sig_min) * t) * x + t * x1

    def forward(self, input_ids, pixel_values, causal_mask, vlm_position_ids, proprio_position_ids,
                action_position_ids, proprios, actions, t, noise: Optional[torch.Tensor] = None,
                prefix_len: Optional[torch.Tensor] = None):
        """Flow-matching loss (pizero.py:607-661); ``noise`` = x0 (default torch.randn_like).  ``prefix_len`` (ints
        [B]): the first prefix_len[b] actions of sample b are a committed prefix -- fed clean with flow
        time 1, given no loss, attended to by the rest.  None: today's loss, with today's kernels.

        Several flow draws per observation (``flow_samples_per_observation``; frozen-VLM pass only): ``t``
        [B, S] with ``noise`` [B, S, H, A] (default randn) trains on the B * S pairs (observation b, draw s), each with
        its own t and x0, all of b sharing its images, prompt, proprio and actions; the VLM prefill runs once per
        observation.  ``prefix_len`` is then [B] (shared by the draws) or [B, S].  The loss is the mean over all pairs:
        the loss of the batch with every observation repeated S times.  ``t`` [B] is today's step."""
        dev = self._dev()
        cdt = self._arena.data.dtype
        if cdt != torch.bfloat16:
            raise RuntimeError("the native path computes in bf16: call model.to(torch.bfloat16)")
        B, H, A = actions.shape
        two = t.dim() == 2  # [B, S]: pairs, even for S == 1
        S = flow_draws(B, H, A, t.shape, None if noise is None else noise.shape,
                       prefix_len.shape if isinstance(prefix_len, torch.Tensor) else None)
        x1 = actions.to(dev, torch.float32).contiguous()
        cm = causal_mask.to(dev)
        cnt = self._mask_spec([cm], [torch.arange(cm.shape[2], device=dev)])
        if S > 1:
            from pizero_native.engine import DRAWS_FROZEN_MSG, GeneralMask

            if self._vlm_needs_grad() or isinstance(cnt, GeneralMask):
                raise ValueError(DRAWS_FROZEN_MSG)
        rep = (lambda x: x.repeat_interleave(S, dim=0)) if S > 1 else (lambda x: x)  # observation -> its S pairs
        x1 = rep(x1)
        x0 = (torch.randn_like(x1) if noise is None else noise.to(dev, torch.float32).reshape(B * S, H, A)).contiguous()
        tied = self._tied
        pos = {"vlm": vlm_position_ids.to(dev, torch.int64).contiguous()}
        if tied:
            pos["expert"] = rep(self._cat_pos(proprio_position_ids, action_position_ids))
        else:
            pos["proprio"] = rep(proprio_position_ids.to(dev, torch.int64).contiguous())
            pos["action"] = rep(action_position_ids.to(dev, torch.int64).contiguous())
        batch = dict(ids=input_ids.to(dev, torch.int64).contiguous(),
                     pix=pixel_values.to(dev, torch.bfloat16).contiguous(), cnt=cnt, pos=pos,
                     proprios=rep(proprios.to(dev, torch.float32).contiguous()), actions=x1,
                     t=t.to(dev, torch.float32).reshape(B * S).contiguous(), x0=x0)
        if prefix_len is not None:
            pl = torch.as_tensor(prefix_len)
            if two and pl.dim() == 2:
                batch["prefix_len"] = self._prefix_len(pl.reshape(B * S), B * S)
            else:
                batch["prefix_len"] = rep(self._prefix_len(pl, B))
        if S > 1:
            batch["draws"] = S
        anchor = next((self._param(n) for n in self._trainable_names()), None)
        if anchor is not None and torch.is_grad_enabled():
            self._check_ddp_wrapper()
        if anchor is None or not torch.is_grad_enabled():
            save = {}
            return self._engine().train_forward(save=save, **batch).view(())
        return _PiZeroLoss.apply(anchor, self, batch)

    def _prefix_len(self, prefix_len, B):
        """ints [B] (or one int) -> the int32 [B] device tensor the engine takes; refused with an adaLN expert, and
        outside [0, horizon_steps - 1] where the values are known on the host"""
        if self.action_expert_adaptive_mode:
            from pizero_native.engine import PREFIX_ADAPTIVE_MSG

            raise NotImplementedError(PREFIX_ADAPTIVE_MSG)
        pl = torch.as_tensor(prefix_len)
        if pl.dtype.is_floating_point or pl.dtype.is_complex or pl.dtype == torch.bool:
            raise ValueError(f"prefix_len must be integers, got {pl.dtype}")
        if pl.dim() == 0:
            pl = pl.expand(B)
        if pl.numel() != B:
            raise ValueError(f"prefix_len has {pl.numel()} entries for a batch of {B}")
        H = self.horizon_steps
        if not pl.is_cuda and pl.numel() and (int(pl.min()) < 0 or int(pl.max()) > H - 1):
            raise ValueError(f"prefix_len must lie in [0, horizon_steps - 1] = [0, {H - 1}], got {pl.tolist()}")
        return pl.reshape(B).to(self._dev(), torch.int32).contiguous()

    def _check_ddp_wrapper(self):
        """torch DDP (train.py:121-126) cannot reduce this model's gradients: the native backward writes
        them into the flat arena, so no per-parameter autograd hook ever fires and DDP would either skip
        the all-reduce or fail on the next step.  Multi-rank training must use PiZeroDDP."""
        import torch.distributed as dist

        if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
                and getattr(self, "_ddp_wrapper", None) is None):
            raise RuntimeError(
                "PiZero's native backward does not fire torch.nn.parallel.DistributedDataParallel's "
                "per-parameter hooks: wrap the model with pizero_native.ddp.PiZeroDDP (same .module / "
                "no_sync() / forward surface, bucketed RCCL all-reduce overlapped with the backward) "
                "instead of DistributedDataParallel (reference train.py:121-126)")

    # ============================================================ inference ==
    def _kv_buffers(self, B):
        e = self._engine()
        d = e.d
        if self._kv is None or self._kv[0].shape[1] != B:
            k = torch.zeros(d.nL, B, d.Lp, d.hd, device=self._dev(), dtype=torch.bfloat16)
            v = torch.zeros_like(k)
            self._kv = (k, v)
        return self._kv

    @torch.no_grad()
    def infer_action(self, input_ids, pixel_values, image_text_proprio_mask, action_mask, vlm_position_ids,
                     proprio_position_ids, action_position_ids, proprios, noise: Optional[torch.Tensor] = None,
                     clip: bool = True, prefix_actions: Optional[torch.Tensor] = None,
                     prefix_len: Optional[torch.Tensor] = None, guide=None):
        """pizero.py:416-490: prefill caches vlm+proprio K/V once, 10 Euler steps on the action expert.
        ``guide`` = (target [B, horizon, action_dim] in normalised units, w [B, horizon], coef [steps]) (DESIGN 7i;
        src/agent/chunking.py: next_guidance, soft_mask, guidance_coef): every Euler step is steered toward the rows
        of the previous chunk by the denoiser's vector-Jacobian product -- inference-time real-time chunking, for
        checkpoints trained without a prefix.  Returned in fp32.  It does not compose with a hard prefix.
        ``prefix_actions`` [B, horizon, action_dim] (normalised units) with ``prefix_len`` (ints [B]): the
        first prefix_len[b] actions of the chunk are committed -- returned bit for bit (fp32), the rest denoised
        around them; rows of ``prefix_actions`` past prefix_len[b] are ignored.
        With an adaLN expert (action_expert_adaptive_mode) the reference's cached path raises AttributeError
        ('NoneType' object has no attribute 'ndim': its prefill runs the proprio mixture without the time condition)
        and cannot work, since the proprio K/V depend on t: here it computes infer_action_naive's result -- the vlm
        K/V cached once, the proprio + action rows re-run with cond(t) every Euler step."""
        if (prefix_actions is None) != (prefix_len is None):
            raise ValueError("infer_action: prefix_actions and prefix_len go together")
        dev = self._dev()
        B = input_ids.shape[0]
        dtype = pixel_values.dtype
        if noise is None:
            noise = torch.randn(B, self.horizon_steps, self.action_dim, device=dev, dtype=torch.float32)
        k, v = self._kv_buffers(B)
        itp, am = image_text_proprio_mask.to(dev), action_mask.to(dev)
        L1 = itp.shape[2]
        spec = self._mask_spec([itp, am], [torch.arange(L1, device=dev),
                                           torch.arange(L1, L1 + am.shape[2], device=dev)])
        kw = {}
        if prefix_len is not None:
            pa = torch.as_tensor(prefix_actions).to(dev, torch.float32).contiguous()
            if tuple(pa.shape) != (B, self.horizon_steps, self.action_dim):
                raise ValueError(f"prefix_actions must be [B, horizon_steps, action_dim] = "
                                 f"{(B, self.horizon_steps, self.action_dim)}, got {tuple(pa.shape)}")
            kw = dict(prefix=pa, prefix_len=self._prefix_len(prefix_len, B))
            dtype = torch.float32  # the committed rows come back bit for bit
        if guide is not None:
            if len(guide) != 3:
                raise ValueError("infer_action: guide is (target, w, coef)")
            kw["guide"] = tuple(torch.as_tensor(x).to(dev, torch.float32).contiguous() for x in guide)
            dtype = torch.float32
        a = self._engine().infer_action(
            input_ids.to(dev, torch.int64).contiguous(), pixel_values.to(dev, torch.bfloat16).contiguous(),
            spec, vlm_position_ids.to(dev, torch.int64).contiguous(),
            proprio_position_ids.to(dev, torch.int64).contiguous(), action_position_ids.to(dev, torch.int64).contiguous(),
            proprios.to(dev, torch.float32).contiguous(), noise.to(dev, torch.float32).contiguous(), k, v,
            clip=clip and self.final_action_clip_value is not None, **kw)
        return a.to(dtype)

    @torch.no_grad()
    def infer_action_naive(self, input_ids, pixel_values, causal_mask, vlm_position_ids, proprio_position_ids,
                           action_position_ids, proprios, noise: Optional[torch.Tensor] = None, clip: bool = True,
                           prefix_actions=None, prefix_len=None, guide=None):
        """pizero.py:492-557.  Re-running the prefix every step gives identical math (the vlm/proprio rows
        never attend to actions), so the native path reuses the cached prefix (fp32-exact equivalence:
        SURVEY 8(c) measured |naive - cached| = 1.8e-7).  With an adaLN expert only the vlm rows are cached: the
        proprio rows depend on t and are re-run with the action rows in every Euler step (see infer_action)."""
        if prefix_actions is not None or prefix_len is not None:
            raise NotImplementedError("infer_action_naive takes no action prefix (prefix_actions / prefix_len, DESIGN "
                                      "7f): use infer_action")
        if guide is not None:
            raise NotImplementedError("infer_action_naive takes no action guidance (guide / action_guidance_beta, "
                                      "DESIGN 7i): use infer_action")
        itp, amask = self.split_full_mask_into_submasks(causal_mask)
        return self.infer_action(input_ids, pixel_values, itp, amask, vlm_position_ids, proprio_position_ids,
                                 action_position_ids, proprios, noise=noise, clip=clip)

    def build_causal_mask_and_position_ids_for_text(self, q_len, attention_mask, kv_cache=None):
        """pizero.py:336-365: the all-zeros text mask (no masking: prefix-LM prefill, cached decode) and the
        positions cumsum(attention_mask) (pads -> 1; a cached decode step takes the last one).  The
        reference reads an undefined global ``bsz`` here; the batch size comes from attention_mask."""
        bsz = attention_mask.shape[0]
        dtype, device = attention_mask.dtype, attention_mask.device
        if kv_cache is None or kv_cache.num_items() == 0:
            mask = torch.zeros(bsz, q_len, q_len, dtype=dtype, device=device)
        else:
            if q_len != 1:
                raise ValueError("Using KV cache so should only use one single token")
            mask = torch.zeros(bsz, q_len, kv_cache.num_items() + q_len, dtype=dtype, device=device)
        mask = mask.unsqueeze(1)
        if kv_cache is not None and kv_cache.num_items() > 0:
            pos = attention_mask.cumsum(-1)[:, -1:]
        else:
            pos = attention_mask.cumsum(-1).masked_fill_(attention_mask == 0, 1)
        return mask, pos

    @torch.no_grad()
    def infer_text(self, input_ids, pixel_values, attention_mask, kv_cache: Optional[KVCache] = None):
        """pizero.py:559-593: {"logits": [B, q_len, vocab]} (+ "kv_cache").  The prompt prefill runs the
        vlm mixture over q_len tokens (image tokens merged from SigLIP); each later call feeds ONE new
        token that attends to the cache.  ``kv_cache`` is this repo's static KVCache (rows appended in
        place, grown when full); ``None`` -> a standalone prefill, like the reference."""
        if not self.use_lm_head:
            raise RuntimeError("infer_text needs use_lm_head: true (pizero.py:106-112)")
        dev = self._dev()
        ids = input_ids.to(dev, torch.int64).contiguous()
        B, q = ids.shape
        am = attention_mask.to(dev)
        _, pos = self.build_causal_mask_and_position_ids_for_text(q, am, kv_cache)
        eng = self._engine()
        d = eng.d
        cache = kv_cache if kv_cache is not None else KVCache()
        start = cache.num_items()
        if start == 0:
            cap = (q + 256 + 7) // 8 * 8
            cache.allocate(d.nL, B, cap, d.hd, dev)
        elif start + q > cache.k.shape[2]:  # grow (amortised) keeping the cached rows
            old_k, old_v = cache.k, cache.v
            cache.k = torch.zeros(d.nL, B, (start + q + 256 + 7) // 8 * 8, d.hd, device=dev, dtype=old_k.dtype)
            cache.v = torch.zeros_like(cache.k)
            cache.k[:, :, :start].copy_(old_k[:, :, :start])
            cache.v[:, :, :start].copy_(old_v[:, :, :start])
        n_img = int((ids == self.image_token_index).sum(1).max().item()) if start == 0 else 0
        pix = None
        if n_img:
            pix = pixel_values.to(dev, torch.bfloat16).contiguous()
            n_img = d.n_img
        # positions are cumsum(attention_mask) <= its length (pizero.py:363-371): bounds the RoPE table
        logits = eng.text_forward(ids, pix, pos.to(torch.int64).contiguous(), cache.k, cache.v, start, n_img,
                                  maxpos=am.shape[1])
        cache.length = start + q
        out = {"logits": logits}
        if kv_cache is not None:
            out["kv_cache"] = kv_cache
        return out


class PiZeroInference(PiZero):
    def forward(self, input_ids, pixel_values, image_text_proprio_mask, action_mask, vlm_position_ids,
                proprio_position_ids, action_position_ids, proprios, noise=None, prefix_actions=None,
                prefix_len=None):
        return super().infer_action(input_ids, pixel_values, image_text_proprio_mask, action_mask,
                                    vlm_position_ids, proprio_position_ids, action_position_ids, proprios, noise=noise,
                                    prefix_actions=prefix_actions, prefix_len=prefix_len)
