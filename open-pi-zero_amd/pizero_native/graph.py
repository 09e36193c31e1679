"""hipGraph-captured action-chunk inference (pizero.py:416-490 as ONE graph replay).

The whole chunk -- SigLIP, prefix prefill writing the static KV cache, and the
10 Euler denoise steps through the action expert -- is recorded once into a
torch.cuda.CUDAGraph (= hipGraph on ROCm).  Every kernel of the path is a
libpizero_hip.so launch on the capture stream; all buffers come from the
graph's private pool; inputs are copied into static tensors before replay.
Replay removes the ~1.7k host launches per chunk (the reference's
eager path is launch-bound).
"""

from __future__ import annotations

import torch


def _prefix_static(static, name):
    """the two static inputs of a prefix-capable graph: the committed actions and their per-sample count.
    Both are read by the captured launches, so another delay or prefix replays the same capture."""
    static[name] = torch.zeros_like(static["noise"])
    static["prefix_len"] = torch.zeros(static["noise"].shape[0], device=static["noise"].device, dtype=torch.int32)


def _load_prefix(static, name, prefix, prefix_len, H, **kw):
    """copy a prefix into the static inputs; ``prefix_len``: an int or [B] (checked against [0, H - 1] where it lives
    on the host); neither given: no prefix (prefix_len = 0)"""
    if name not in static:
        if prefix is not None or prefix_len is not None:
            raise ValueError("this graph takes no action prefix: call enable_prefix() before capture()")
        return
    if prefix is None or prefix_len is None:
        if prefix is not None or prefix_len is not None:
            raise ValueError("the action prefix and its length go together")
        static["prefix_len"].zero_()
        return
    pl = torch.as_tensor(prefix_len)
    if pl.dtype.is_floating_point or pl.dtype.is_complex or pl.dtype == torch.bool:
        raise ValueError(f"prefix_len / delay must be integers, got {pl.dtype}")
    if not pl.is_cuda and (int(pl.min()) < 0 or int(pl.max()) > H - 1):
        raise ValueError(f"prefix_len / delay must lie in [0, horizon_steps - 1] = [0, {H - 1}], got {pl.tolist()}")
    static["prefix_len"].copy_(pl.to(torch.int32).expand_as(static["prefix_len"]) if pl.dim() == 0
                               else pl.reshape(static["prefix_len"].shape), **kw)
    static[name].copy_(torch.as_tensor(prefix).reshape(static[name].shape), **kw)


def _load_guide(static, target, w, coef, **kw):
    """copy the guidance inputs of a guidance-capable graph; none given: weights 0, the unguided chunk"""
    if "guide_w" not in static:
        if target is not None or w is not None or coef is not None:
            raise ValueError("this graph takes no action guidance: call enable_guidance() before capture()")
        return
    if target is None and w is None and coef is None:
        static["guide_w"].zero_()
        return
    if target is None or w is None or coef is None:
        raise ValueError("the guidance target, its row weights and the coefficient table go together")
    for name, x in (("guide_target", target), ("guide_w", w), ("guide_coef", coef)):
        x = torch.as_tensor(x)
        if x.numel() != static[name].numel():
            raise ValueError(f"{name} must have shape {tuple(static[name].shape)}, got {tuple(x.shape)}")
        static[name].copy_(x.reshape(static[name].shape), **kw)


class InferenceGraph:
    """After ``enable_prefix()`` the graph also takes a committed action prefix (normalised units) and its
    per-sample length as static inputs; without that call it is the graph it always was.
    After ``enable_guidance()`` it runs the guided loop on the static inputs ``guide_target`` (normalised
    units), ``guide_w`` and ``guide_coef``; a graph takes one of the two options, not both."""

    prefix = False
    guidance = False
    PREFIX_INPUT = "prefix"

    def __init__(self, model, bsz, clip=True):
        self.m = model
        self.B = bsz
        self.clip = clip
        e = model._engine()
        d = e.d
        dev = model._dev()
        self.static = dict(
            ids=torch.zeros(bsz, d.P, device=dev, dtype=torch.int64),
            pix=torch.zeros(bsz * d.n_images, 3, d.img, d.img, device=dev, dtype=torch.bfloat16),
            cnt=torch.full((bsz,), d.P, device=dev, dtype=torch.int32),
            vpos=torch.arange(1, d.P + 1, device=dev).repeat(bsz, 1),
            ppos=torch.arange(1, d.C + 1, device=dev).repeat(bsz, 1),
            apos=torch.arange(d.C + 1, d.C + d.H + 1, device=dev).repeat(bsz, 1),
            proprios=torch.zeros(bsz, d.C, d.Pd, device=dev, dtype=torch.float32),
            noise=torch.zeros(bsz, d.H, d.A, device=dev, dtype=torch.float32),
        )
        self.k, self.v = model._kv_buffers(bsz)
        self.graph = None
        self.out = None
        self._f8 = None

    def enable_prefix(self):
        """add the action prefix and its per-sample length to the static inputs (before capture(); a prefix length of
        0, the state after this call, gives the bits of the graph without the option).  Returns self."""
        if self.m._engine().d.ada:
            from .engine import PREFIX_ADAPTIVE_MSG

            raise NotImplementedError(PREFIX_ADAPTIVE_MSG)
        if self.guidance:
            from .engine import GUIDE_PREFIX_MSG

            raise NotImplementedError(GUIDE_PREFIX_MSG)
        if not self.prefix:
            if self.graph is not None:
                raise RuntimeError("enable_prefix() must precede capture()")
            _prefix_static(self.static, self.PREFIX_INPUT)
            self.prefix = True
        return self

    def enable_guidance(self):
        """add the guidance target, its row weights and the per-step coefficients to the static inputs (before
        capture()): the captured loop is the guided one, and one capture serves every target, delay, overlap and
        beta.  Weights of 0, the state after this call, give the unguided chunk (through the guided step's kernels,
        so within rounding, not bit for bit).  Returns self."""
        e = self.m._engine()
        from .engine import GUIDE_ADAPTIVE_MSG, GUIDE_FP8_MSG, GUIDE_PREFIX_MSG

        if e.d.ada:
            raise NotImplementedError(GUIDE_ADAPTIVE_MSG)
        if e.f8 is not None:
            raise NotImplementedError(GUIDE_FP8_MSG)
        if self.prefix:
            raise NotImplementedError(GUIDE_PREFIX_MSG)
        if not self.guidance:
            if self.graph is not None:
                raise RuntimeError("enable_guidance() must precede capture()")
            self._guide_static()
            self.guidance = True
        return self

    def _guide_static(self):
        s, d = self.static, self.m._engine().d
        s["guide_target"] = torch.zeros_like(s["noise"])
        s["guide_w"] = torch.zeros(s["noise"].shape[:2], device=s["noise"].device, dtype=torch.float32)
        s["guide_coef"] = torch.zeros(d.steps, device=s["noise"].device, dtype=torch.float32)

    def _guide(self, target=None):
        """the engine's guide argument from the static inputs (None without the option)"""
        s = self.static
        if not self.guidance:
            return None
        return (s["guide_target"] if target is None else target, s["guide_w"], s["guide_coef"])

    def _run(self):
        s = self.static
        return self.m._engine().infer_action(s["ids"], s["pix"], s["cnt"], s["vpos"], s["ppos"], s["apos"],
                                              s["proprios"], s["noise"], self.k, self.v, clip=self.clip,
                                              prefix=s.get("prefix"), prefix_len=s.get("prefix_len"),
                                              guide=self._guide())

    def load(self, input_ids, pixel_values, cnt, vpos, ppos, apos, proprios, noise, prefix=None, prefix_len=None,
             guide_target=None, guide_w=None, guide_coef=None):
        s = self.static
        _load_prefix(s, "prefix", prefix, prefix_len, s["noise"].shape[1])
        _load_guide(s, guide_target, guide_w, guide_coef)
        s["ids"].copy_(input_ids)
        s["pix"].copy_(pixel_values.reshape(s["pix"].shape))
        s["cnt"].copy_(cnt)
        s["vpos"].copy_(vpos)
        s["ppos"].copy_(ppos)
        s["apos"].copy_(apos)
        s["proprios"].copy_(proprios.reshape(s["proprios"].shape))
        s["noise"].copy_(noise.reshape(s["noise"].shape))

    def capture(self):
        # re-quantise stale fp8 codes first, so the codes recorded here are the ones the captured launches read
        # (the warm-up's infer_action would otherwise replace them and force a needless re-capture)
        e = self.m._engine()
        e.lora_refresh()  # LoRA: the merged shadow weights the captured launches read (never rebuilt inside a capture)
        e.fp8_refresh()
        self._f8 = e.f8
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # warm-up: kernel attributes, rope tables, allocator
                self._run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._run()
        torch.cuda.synchronize()
        return self

    def replay(self):
        # bf16 weights are read in place (an optimizer step / checkpoint load is seen by the next replay);
        # fp8 codes and their per-tensor scales are baked into the captured launches, so a weight change
        # since the capture re-quantises them (Engine.fp8_refresh) and re-captures the graph
        e = self.m._engine()
        e.derived_refresh()  # in place: the captured launches keep their pointers
        e.lora_refresh()  # LoRA: merged weights rebuilt in place after an optimizer step / checkpoint load
        if e.f8 is not self._f8 or e.fp8_refresh():
            self.capture()
        self.graph.replay()
        return self.out


class ObservationGraph(InferenceGraph):
    """The action chunk from RAW observations as one graph replay: uint8 camera frames of any size, raw
    proprio and token ids in, actions in robot units out.  Captured, in order, on one linear stream:

      1. ``pz_image_resize_norm`` (Lanczos-3 resize + pixel normalisation; its fp32 scratch comes from the graph's
         pool) and ``pz_proprio_normalize``,
      2. ``Engine.infer_action``,
      3. ``pz_action_denormalize`` (the last action dimension, the gripper, passes through).

    ``enable_prefix()`` adds the static inputs ``prev_actions`` (robot units) and ``prefix_len`` and two
    launches outside the denoise loop, ``pz_action_normalize`` of the previous chunk and the prefix rows written over
    the noise; the clamp and the denormalisation are replaced by their prefix forms, the latter copying rows
    ``h < prefix_len[b]`` from ``prev_actions`` bit for bit.

    ``enable_guidance()`` adds ``guide_target`` (what is left of the previous chunk, ROBOT units,
    normalised inside the graph by ``pz_action_normalize``), ``guide_w``, ``guide_coef`` and ``prefix_len`` (the
    delay): the loop is the guided one, the clamp skips rows ``h < prefix_len[b]`` and the denormalisation copies them
    from ``guide_target`` bit for bit -- the robot executes those rows from the old chunk anyway.

    The static inputs are the raw ones; the prefix counts are ``attention_mask.sum(1)``, computed by the caller where
    the mask is born, so no [L, L] mask exists on this path, and the position ids are constants.  ``stats`` is the
    dataset-statistics dict (``proprio`` / ``action`` -> ``p01``, ``p99``, ``mean``, ``std``) with the optional keys
    ``proprio_normalization_type`` / ``action_normalization_type`` (``bound`` by default, as in simpler.py:25-26).
    capture() and replay() are InferenceGraph's: the weight-refresh and re-capture rules are the same.
    ``run_eager()`` enqueues the same launches without a graph.  ``out`` holds the robot-unit actions and
    ``out_norm`` the model's normalised chunk they were computed from (both fp32 [B, H, A])."""

    PREFIX_INPUT = "prev_actions"  # the previous chunk in ROBOT units: normalised inside the graph, passed through

    def __init__(self, model, bsz, frame_hw, stats, channels_last=True, clip=True):
        from . import ops

        self.m = model
        self.B = bsz
        self.clip = clip
        self.channels_last = bool(channels_last)
        e = model._engine()
        d = e.d
        dev = model._dev()
        h, w = (int(x) for x in frame_hw)
        ops.lanczos3_taps(h, d.img), ops.lanczos3_taps(w, d.img)  # refuse an unsupported geometry here, not at capture
        n = bsz * d.n_images
        self.static = dict(
            frames=torch.zeros((n, h, w, 3) if self.channels_last else (n, 3, h, w), device=dev, dtype=torch.uint8),
            ids=torch.zeros(bsz, d.P, device=dev, dtype=torch.int64),
            cnt=torch.full((bsz,), d.P, device=dev, dtype=torch.int32),
            vpos=torch.arange(1, d.P + 1, device=dev).repeat(bsz, 1),
            ppos=torch.arange(1, d.C + 1, device=dev).repeat(bsz, 1),
            apos=torch.arange(d.C + 1, d.C + d.H + 1, device=dev).repeat(bsz, 1),
            raw_proprio=torch.zeros(bsz, d.C, d.Pd, device=dev, dtype=torch.float32),
            noise=torch.zeros(bsz, d.H, d.A, device=dev, dtype=torch.float32),
        )
        self.modes = {}
        self.stat = {}
        for key, dim in (("proprio", d.Pd), ("action", d.A)):
            mode = stats.get(f"{key}_normalization_type", "bound")
            if mode not in ops.NORM_MODES:
                raise ValueError(f"{key}_normalization_type must be one of {sorted(ops.NORM_MODES)}, got {mode!r}")
            names = ("p01", "p99") if mode == "bound" else ("mean", "std")
            ab = [torch.as_tensor(stats[key][nm], dtype=torch.float64).to(torch.float32).to(dev).contiguous()
                  for nm in names]
            if any(t.numel() != dim for t in ab):
                raise ValueError(f"dataset statistics: {key} has {ab[0].numel()} dimensions, the model {dim}")
            self.modes[key], self.stat[key] = mode, ab
        self.k, self.v = model._kv_buffers(bsz)
        self.graph = None
        self.out = None
        self.out_norm = None
        self._f8 = None

    def _guide_static(self):
        InferenceGraph._guide_static(self)
        s = self.static
        s["prefix_len"] = torch.zeros(s["noise"].shape[0], device=s["noise"].device, dtype=torch.int32)

    def _run_guided(self, pix, proprios):
        from . import ops

        s = self.static
        d = self.m._engine().d
        target = ops.action_normalize(s["guide_target"], *self.stat["action"], self.modes["action"], n_pass=1)
        self.out_norm = self.m._engine().infer_action(s["ids"], pix, s["cnt"], s["vpos"], s["ppos"], s["apos"],
                                                      proprios, s["noise"], self.k, self.v, clip=False,
                                                      guide=self._guide(target))
        if self.clip and d.clip is not None:
            ops.clamp_(self.out_norm, -d.clip, d.clip, prefix_len=s["prefix_len"])
        return ops.action_denormalize(self.out_norm, *self.stat["action"], self.modes["action"], n_pass=1,
                                      prev=s["guide_target"], prefix_len=s["prefix_len"])

    def _run(self):
        from . import ops

        s = self.static
        d = self.m._engine().d
        pix = ops.image_resize_norm(s["frames"], d.img, channels_last=self.channels_last)
        proprios = ops.proprio_normalize(s["raw_proprio"], *self.stat["proprio"], self.modes["proprio"])
        if self.guidance:
            return self._run_guided(pix, proprios)
        prefix = None
        if self.prefix:
            prefix = ops.action_normalize(s["prev_actions"], *self.stat["action"], self.modes["action"], n_pass=1)
        self.out_norm = self.m._engine().infer_action(s["ids"], pix, s["cnt"], s["vpos"], s["ppos"], s["apos"],
                                                      proprios, s["noise"], self.k, self.v, clip=self.clip,
                                                      prefix=prefix, prefix_len=s.get("prefix_len"))
        return ops.action_denormalize(self.out_norm, *self.stat["action"], self.modes["action"], n_pass=1,
                                      prev=s.get("prev_actions"), prefix_len=s.get("prefix_len"))

    def load(self, frames, input_ids, cnt, raw_proprio, noise, prev_actions=None, delay=None, guide_w=None,
             guide_coef=None):
        """``guide_w`` / ``guide_coef`` (a guidance graph): ``prev_actions`` is then the guidance target in robot units
        and ``delay`` the number of leading rows passed through from it"""
        s = self.static
        nb = dict(non_blocking=True)
        if self.guidance:
            _load_guide(s, prev_actions, guide_w, guide_coef, **nb)
            if delay is None:
                s["prefix_len"].zero_()
            else:
                _load_prefix(s, "guide_target", s["guide_target"], delay, s["noise"].shape[1], **nb)
        else:
            _load_guide(s, None, guide_w, guide_coef)
            _load_prefix(s, "prev_actions", prev_actions, delay, s["noise"].shape[1], **nb)
        s["frames"].copy_(frames.reshape(s["frames"].shape), **nb)
        s["ids"].copy_(input_ids, **nb)
        s["cnt"].copy_(cnt.reshape(s["cnt"].shape), **nb)
        s["raw_proprio"].copy_(raw_proprio.reshape(s["raw_proprio"].shape), **nb)
        s["noise"].copy_(noise.reshape(s["noise"].shape), **nb)

    def run_eager(self):
        """the captured launches, enqueued directly on the current stream (``EvalAgent(use_graph=False)``).  ``out`` /
        ``out_norm`` then name the eager results, so a graph captured earlier is dropped (re-captured on next use)."""
        self.graph = None
        self.m._engine().derived_refresh()
        self.out = self._run()
        return self.out
