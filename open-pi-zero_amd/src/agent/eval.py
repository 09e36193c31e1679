"""EvalAgent: the reference's inference call site (eval.py:21-189) on the native path.

Construction mirrors the reference: ``PiZeroInference(cfg)``, checkpoint load
(``_orig_mod.`` stripped, strict=True), ``freeze_all_weights``, dtype/device
moves.  The action chunk for one observation is ``infer_chunk`` (mask/position
building + ``model(**inputs)`` = PiZeroInference.forward, eval.py:99-125); with
``use_graph`` the whole chunk replays as one hipGraph (pizero_native/graph.py).
``act`` is the same chunk from RAW observations (camera frames of any size, raw proprio) to actions in robot
units: the env adapter's resize and normalisation (env_adapter/{base,simpler}.py) run as kernels inside the graph.
The SimplerEnv rollout loop, the tokenizer and the robot-specific post-processing are out of scope:
``run()`` needs ``simpler_env`` and raises without it.
"""

from __future__ import annotations

import torch

from src.utils.config import cfg_get


class EvalAgent:
    def __init__(self, cfg, use_graph: bool = True):
        from src.model.vla.pizero import PiZeroInference

        self.cfg = cfg
        self.device = torch.device(f"cuda:{cfg_get(cfg, 'gpu_id', 0)}")
        self.dtype = torch.bfloat16 if cfg_get(cfg, "use_bf16", True) else torch.float32
        self.model = PiZeroInference(cfg, use_ddp=False, device=self.device, dtype=torch.bfloat16, init="none")
        if cfg_get(cfg, "checkpoint_path"):
            self.load_checkpoint(cfg_get(cfg, "checkpoint_path"))
        self.model.tie_action_proprio_weights()
        self.model.freeze_all_weights()
        self.model.quantize_base_()  # quantize: True packs the VLM's Linears (no-op otherwise, or if loaded packed)
        self.model.eval()
        self.use_graph = use_graph
        self._graphs = {}
        self._obs_graphs = {}
        self._stats = None
        self.act_steps = cfg_get(cfg, "act_steps", cfg_get(cfg, "horizon_steps"))

    def load_checkpoint(self, path):
        data = torch.load(path, weights_only=True, map_location="cpu")
        sd = {k.replace("_orig_mod.", ""): v for k, v in data["model"].items()}
        self.model.load_state_dict(sd, strict=True)

    @torch.no_grad()
    def infer_chunk(self, input_ids, attention_mask, pixel_values, proprios, noise=None):
        """Tokenized observation -> [B, horizon, action_dim] normalised actions (eval.py:99-125)."""
        m = self.model
        dev = self.device
        # masks are built on the device once per call: the block pattern built from the attention mask is
        # known (its prefix counts are remembered), so no per-call validation or host sync follows
        mask, vpos, ppos, apos = m.build_causal_mask_and_position_ids(attention_mask.to(dev), self.dtype)
        itp, amask = m.split_full_mask_into_submasks(mask)
        B = input_ids.shape[0]
        if noise is None:
            noise = torch.randn(B, m.horizon_steps, m.action_dim, device=dev)
        if not self.use_graph:
            return m(input_ids.to(dev), pixel_values.to(dev, self.dtype), itp, amask, vpos, ppos, apos,
                     proprios.to(dev, self.dtype), noise=noise)
        from pizero_native.graph import InferenceGraph

        cnt = m.block_prefix_counts(itp, amask)
        args = (input_ids.to(dev), pixel_values.to(dev, torch.bfloat16), cnt, vpos, ppos, apos,
                proprios.to(dev, torch.float32), noise)
        g = self._graphs.get(B)
        if g is None:
            g = self._graphs[B] = InferenceGraph(m, B)
            g.load(*args)
            g.capture()
        g.load(*args)
        return g.replay().to(self.dtype)

    STATS_KEY = "env.adapter.dataset_statistics_path"

    def _dataset_statistics(self):
        """The env adapter's settings under the reference's names (config/eval/bridge.yaml:19-28, simpler.py:19-37):
        the statistics JSON and the two normalisation types, as the dict ObservationGraph takes."""
        if self._stats is None:
            from src.agent.env_adapter.base import load_dataset_statistics

            path = cfg_get(self.cfg, self.STATS_KEY)
            if not path:
                raise ValueError(f"EvalAgent.act needs the dataset statistics: set {self.STATS_KEY} (a JSON file with "
                                 "proprio / action -> p01, p99, mean, std)")
            stats = dict(load_dataset_statistics(path))
            for k in ("proprio_normalization_type", "action_normalization_type"):
                stats[k] = cfg_get(self.cfg, f"env.adapter.{k}", "bound")
            self._stats = stats
        return self._stats

    def observation_graph(self, bsz, frame_hw, channels_last=True, prefix=False, guidance=False):
        """the ObservationGraph of one (batch size, frame geometry, layout, with / without an action prefix, with /
        without guidance); built on first use, not yet captured"""
        from pizero_native.graph import ObservationGraph

        key = (bsz, tuple(int(x) for x in frame_hw), bool(channels_last)) + ((True,) if prefix else ()) + \
            (("guide",) if guidance else ())
        g = self._obs_graphs.get(key)
        if g is None:
            g = self._obs_graphs[key] = ObservationGraph(self.model, bsz, key[1], self._dataset_statistics(),
                                                         channels_last=channels_last)
            if prefix:
                g.enable_prefix()
            if guidance:
                g.enable_guidance()
        return g

    @torch.no_grad()
    def act(self, frames, input_ids, attention_mask, raw_proprio, noise=None, channels_last=True, prev_actions=None,
            delay=None, overlap=None, guidance_beta=None):
        """Raw observation -> fp32 [B, horizon, action_dim] actions in ROBOT units, one graph replay.

        ``frames``: uint8 camera frames of any size, [B (* n_images), H, W, 3] (or [.., 3, H, W] with
        ``channels_last=False``), torch or numpy, host or device; ``raw_proprio``: [B, cond_steps, proprio_dim] in
        robot units; ``input_ids`` / ``attention_mask``: the tokenised prompt.  The Lanczos-3 resize to the model's
        image size, the pixel and proprio normalisation and the action denormalisation run as HIP kernels inside the
        captured graph (``use_graph=False``: the same kernels, enqueued eagerly).  The prefix counts are the
        attention mask's row sums, taken where the mask lives; no [L, L] mask is built.  The returned tensor is the
        graph's static output: copy it before the next call if it must survive it.

        ``prev_actions`` (robot units, [B, horizon, action_dim]) with ``delay`` (an int or [B], 0 <= delay <
        horizon): the first ``delay`` actions of the new chunk are the ones the robot executes while this
        call runs -- ``prev_actions[:, :delay]``, e.g. from ``src.agent.chunking.next_prefix`` -- and the chunk is
        denoised around them.  Rows >= delay of ``prev_actions`` are ignored.  The returned rows < delay are
        ``prev_actions``' bits.  One capture serves every delay and prefix; calls without ``prev_actions`` keep
        using the graph without the option.

        ``overlap`` (an int, ``delay <= overlap <= horizon``, ``delay < horizon``) turns the hard prefix
        into guidance, for checkpoints trained without prefixes: ``prev_actions`` is what is left of the previous
        chunk (``src.agent.chunking.next_guidance``), its first ``overlap`` rows meaningful, and every Euler step is
        steered toward them with the weights ``soft_mask(horizon, delay, overlap)`` and the coefficients
        ``guidance_coef(steps, guidance_beta)`` (``guidance_beta`` defaults to the config key
        ``action_guidance_beta``, default 5.0).  The returned rows < delay are still ``prev_actions``' bits and the
        clamp covers the other rows only.  ``overlap=None`` is the hard prefix above, launch for launch; guided calls
        use a graph of their own, so calls without ``overlap`` keep the graph and the bits they had."""
        self._dataset_statistics()  # without statistics: the ValueError that names the key, before anything else
        m = self.model
        frames, input_ids, attention_mask, raw_proprio = (torch.as_tensor(x) for x in
                                                          (frames, input_ids, attention_mask, raw_proprio))
        if frames.dtype != torch.uint8 or frames.dim() != 4:
            raise ValueError(f"act: frames must be uint8 [n, H, W, 3] or [n, 3, H, W], got {frames.dtype} "
                             f"{tuple(frames.shape)}")
        B = input_ids.shape[0]
        hw = frames.shape[1:3] if channels_last else frames.shape[2:4]
        cnt = attention_mask.sum(1)
        if noise is None:
            noise = torch.randn(B, m.horizon_steps, m.action_dim, device=self.device)
        if (prev_actions is None) != (delay is None):
            raise ValueError("act: prev_actions and delay go together")
        kw = {}
        if prev_actions is not None:
            if m.action_expert_adaptive_mode:
                from pizero_native.engine import PREFIX_ADAPTIVE_MSG

                raise NotImplementedError(PREFIX_ADAPTIVE_MSG)
            prev = torch.as_tensor(prev_actions).to(torch.float32)
            if tuple(prev.shape) != (B, m.horizon_steps, m.action_dim):
                raise ValueError(f"act: prev_actions must be [B, horizon_steps, action_dim] = "
                                 f"{(B, m.horizon_steps, m.action_dim)}, got {tuple(prev.shape)}")
            kw = dict(prev_actions=prev, delay=delay)
        if overlap is None and guidance_beta is not None:
            raise ValueError("act: guidance_beta needs overlap")
        if overlap is not None:
            kw.update(self._guidance_tables(kw, B, delay, overlap, guidance_beta))
        g = self.observation_graph(B, hw, channels_last, prefix=bool(kw) and overlap is None,
                                   guidance=overlap is not None)
        g.load(frames.contiguous(), input_ids, cnt, raw_proprio.to(torch.float32), noise, **kw)
        if not self.use_graph:
            return g.run_eager()
        if g.graph is None:
            g.capture()
        return g.replay()

    def _guidance_tables(self, kw, B, delay, overlap, beta):
        """the host-made inputs of a guided call: row weights [B, H] and step coefficients [steps]"""
        import numpy as np

        from src.agent.chunking import guidance_coef, soft_mask

        m = self.model
        H = m.horizon_steps
        if not kw:
            raise ValueError("act: overlap needs prev_actions and delay")
        if m.action_expert_adaptive_mode:
            from pizero_native.engine import GUIDE_ADAPTIVE_MSG

            raise NotImplementedError(GUIDE_ADAPTIVE_MSG)
        dl = torch.as_tensor(delay)
        if dl.dtype.is_floating_point or dl.dtype == torch.bool or dl.is_cuda:
            raise ValueError("act: with overlap, delay must be host integers (an int or [B])")
        dl = [int(x) for x in (dl.expand(B) if dl.dim() == 0 else dl.reshape(B)).tolist()]
        overlap = int(overlap)
        if not all(0 <= x <= overlap <= H and x < H for x in dl):
            raise ValueError(f"act: need 0 <= delay <= overlap <= horizon_steps = {H} and delay < horizon_steps, got "
                             f"delay {dl}, overlap {overlap}")
        if beta is None:
            beta = cfg_get(self.cfg, "action_guidance_beta", 5.0)
        w = np.stack([soft_mask(H, x, overlap) for x in dl])
        return dict(guide_w=torch.from_numpy(w), guide_coef=torch.from_numpy(guidance_coef(m.num_inference_steps, beta)))

    def run(self):
        try:
            import simpler_env  # noqa: F401
        except ImportError as e:
            raise RuntimeError("SimplerEnv rollouts need simpler_env (not installed; out of scope, SURVEY 2.1)") from e
        raise NotImplementedError("SimplerEnv adapters are out of scope this round (SURVEY 2.1)")
