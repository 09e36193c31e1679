"""TrainAgent: the reference's training loop (train.py:36-560) on the native MI355X path.

Same structure and semantics as shroglck/open-pi-zero's TrainAgent:
  * one process per GPU (torchrun), ``PiZero(cfg, use_ddp)``, tie + freeze,
    bf16 weights, data-parallel wrapper with ``no_sync`` for accumulation;
  * two optimizers (action expert / VLM) with CosineAnnealingWarmupRestarts,
    joint grad-norm clip, ``zero_grad(set_to_none=True)``;
  * flow-matching time sampling (beta / uniform), per-batch preprocessing into
    the 9 forward kwargs (pizero.py:607-618);
  * checkpoints with the reference's keys (cnt_update, cnt_batch, model,
    action_optimizer, vlm_optimizer, *_lr_scheduler, wandb_id, n_averaged);
  * EMA / SWA weight averaging (src.agent.model_averaging.ModelAveraging, train.py:268-269,389-393), in-training
    validation on the averaged weights (train.py:413-459) and the averaged weights as the checkpoint's "model"
    (train.py:497-529).  An extension: with averaging active the checkpoint also holds the live weights
    ("model_train"), so the average can be resumed exactly (the reference cannot resume one).
MI355X-native pieces: pizero_native.ddp.PiZeroDDP (RCCL bucketed all-reduce
overlapped with backward), pizero_native.optim.FusedAdamW (flat fused AdamW; by default
with the reference's blockwise 8-bit state, ``optimizer_state_bits: 8`` -- the algorithm of
bitsandbytes' AdamW8bit restated, bitsandbytes itself absent: parity with it unpinned).
An extension: ``optimizer_rounding: compensated | stochastic`` (default ``nearest``, the reference's behaviour)
keeps steps smaller than half a bf16 ulp of a weight instead of rounding them away; its state travels in the
optimizer state dicts, so a resumed run continues bit for bit.
Data: the OXE/RLDS TensorFlow pipeline is out of scope; the
agent consumes any iterable of reference-format batches, by default
``SyntheticBridgeDataset`` (bridge-shaped random batches, already tokenized).
With ``data.train.episode_store`` (``data.val.episode_store``) set and no dataset handed in, the batches come from an
episode store instead, chunked, normalised and assembled on the device (pizero_native.episodes).
What that pipeline does to every training frame after the resize -- random crop and colour jitter
(src/agent/dataset.py:38-70) -- runs on the device with ``image_augment: True`` (off by default).
An extension: ``action_prefix_max_delay: D`` > 0 (off by default) trains every sample with its own first
d ~ U{0..D} actions as a committed, loss-free prefix ("real-time chunking"), so that a chunk can be inferred around
the actions a robot executes while the inference runs (``EvalAgent.act(prev_actions=, delay=)``).
"""

from __future__ import annotations

import logging
import os
from collections import deque

import numpy as np
import torch

from src.utils.config import cfg_get

log = logging.getLogger(__name__)


def sample_fm_time(bsz, flow_sampling="beta", beta_dist=None, t_max=1 - 0.001):
    """train.py:239-247: beta -> t = t_max * (1 - Beta(alpha, beta)); uniform -> stratified
    (U + arange(B)/B) mod (1 - 1e-5).  Same torch RNG calls as the reference (seeded parity)."""
    if flow_sampling == "uniform":
        return (torch.rand(1) + torch.arange(bsz) / bsz) % (1 - 1e-5)
    if flow_sampling != "beta":
        raise ValueError(f"Invalid flow matching timestep sampling mode: {flow_sampling}")
    return t_max * (1 - beta_dist.sample((bsz,)))


class SyntheticBridgeDataset(torch.utils.data.IterableDataset):
    """Reference batch format (train.py:319-327) with tokenized text (no tokenizer offline)."""

    def __init__(self, cfg, batch_size, seed=0):
        self.cfg, self.B, self.seed = cfg, batch_size, seed

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        c = self.cfg
        P = cfg_get(c, "max_seq_len")
        n_img = cfg_get(c, "vision.config.num_image_tokens")
        H = cfg_get(c, "horizon_steps")
        img = cfg_get(c, "vision.config.image_size")
        vmax = min(int(cfg_get(c, "vocab_size")), int(cfg_get(c, "image_token_index")))
        nl = min(108, vmax - 1)
        while True:
            ids = torch.zeros(self.B, P, dtype=torch.int64)
            ids[:, :n_img] = cfg_get(c, "image_token_index")
            ids[:, n_img] = 2
            for b in range(self.B):
                n = int(torch.randint(4, P - n_img, (1,), generator=g))
                ids[b, n_img + 1 : n_img + n - 1] = torch.randint(3, vmax, (n - 2,), generator=g)
                ids[b, n_img + n - 1] = nl
            yield {
                "input_ids": ids,
                "attention_mask": (ids != 0).long(),
                "pixel_values": torch.randint(0, 256, (self.B, 3, img, img), generator=g, dtype=torch.uint8),
                "proprio": torch.rand(self.B, cfg_get(c, "cond_steps"), cfg_get(c, "proprio_dim"), generator=g) * 2 - 1,
                "action": torch.rand(self.B, H, cfg_get(c, "action_dim"), generator=g) * 2 - 1,
            }


class TrainAgent:
    def __init__(self, cfg, dataset=None, val_dataset=None):
        from pizero_native.ddp import PiZeroDDP
        from pizero_native.optim import FusedAdamW
        from src.agent.model_averaging import ModelAveraging
        from src.model.vla.pizero import PiZero
        from src.utils.optim import CosineAnnealingWarmupRestarts

        self.cfg = cfg
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.multi_gpu = self.world > 1
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", cfg_get(cfg, "gpu_id", 0)))
        self.device = torch.device(f"cuda:{self.local_rank}")
        torch.cuda.set_device(self.device)
        if self.multi_gpu and not torch.distributed.is_initialized():
            torch.distributed.init_process_group("nccl", device_id=self.device)
        self.main_rank = self.rank == 0
        self.dtype = torch.bfloat16 if cfg_get(cfg, "use_bf16", True) else torch.float32
        self.n_updates = int(cfg_get(cfg, "n_updates", 1))
        self.max_grad_norm = float(cfg_get(cfg, "max_grad_norm", 1.0))
        self.log_freq = int(cfg_get(cfg, "log_freq", 16))
        self.save_model_freq = int(cfg_get(cfg, "save_model_freq", 10 ** 9))
        self.save_model_start = int(cfg_get(cfg, "save_model_start", 0))
        self.log_dir = cfg_get(cfg, "log_dir", "") or "."
        self.checkpoint_dir = os.path.join(self.log_dir, "checkpoint")

        self.cnt_update = 0
        self.cnt_batch = 0
        # micro-batches consumed so far: cnt_batch in an uninterrupted run.  A checkpoint stores the index of its LAST
        # micro-batch (the reference's bookkeeping, kept), so load_checkpoint restores cnt_batch + 1 here: what is keyed
        # on this count (the action-prefix draws) continues across a resume where cnt_batch repeats one index
        self.micro_batches_seen = 0
        self.wandb_id = None
        self.lora = bool(cfg_get(cfg, "lora", False))
        # quantize: True (QLoRA): the frozen base Linears of the VLM are packed to 4 bits after loading
        self.quantize = bool(cfg_get(cfg, "quantize", False))
        if self.lora and not cfg_get(cfg, "load_pretrained_weights", False):  # train.py:87-89
            raise AssertionError("lora: True must be used with load_pretrained_weights: True")
        if self.quantize and not cfg_get(cfg, "load_pretrained_weights", False):  # train.py:87-89
            raise AssertionError("quantize: True must be used with load_pretrained_weights: True")
        if self.quantize and (cfg_get(cfg, "use_ema", False) or cfg_get(cfg, "use_swa", False)):
            raise NotImplementedError("quantize: True with use_ema / use_swa is not supported: the average would need "
                                      "a second copy of the packed base weights")
        model = PiZero(cfg, use_ddp=self.multi_gpu, device=self.device, dtype=self.dtype, init="default")
        self.model = model
        self._averaging_enabled = bool(cfg_get(cfg, "use_ema", False) or cfg_get(cfg, "use_swa", False))
        self._resume_average = None
        resume = cfg_get(cfg, "resume_checkpoint_path")
        if resume:
            self.load_checkpoint(resume)
        elif cfg_get(cfg, "load_pretrained_weights", False):
            model.load_pretrained_weights()
        model.tie_action_proprio_weights()
        model.freeze_unused_weights()
        if self.lora:  # train.py:101-102
            model.freeze_non_lora_weights_in_vlm()
        model.quantize_base_()  # no-op without quantize: True
        self.model_meta = PiZeroDDP(model) if self.multi_gpu else model
        # every rank keeps its own average: the weights are identical across ranks, so nothing is communicated
        self.model_averaging = ModelAveraging(model, cfg, self.device)
        if self._resume_average is not None:
            self.model_averaging.load_average(*self._resume_average)
            self._resume_average = None

        per_dev = int(cfg_get(cfg, "per_device_batch_size"))
        self.grad_accumulation_steps = max(int(cfg_get(cfg, "global_batch_size")) // per_dev // self.world, 1)
        # batches assembled on the device from an episode store (``data.train.episode_store``), when no
        # dataset is handed in; without the key, the synthetic batches as before
        if dataset is None:
            dataset = self._episode_batches("train", per_dev)
        self.train_dataloader = dataset if dataset is not None else SyntheticBridgeDataset(cfg, per_dev, seed=self.rank)

        # quantize without lora: the VLM is fully frozen (the model logged the reference's warning, train.py:90-93)
        self.train_vlm = bool(cfg_get(cfg, "train_vlm", True)) and not (self.quantize and not self.lora)
        # the reference's bnb AdamW8bit (train.py:171-175): blockwise 8-bit state by default
        self.state_bits = int(cfg_get(cfg, "optimizer_state_bits", 8))
        # how the fp32 update becomes the bf16 weight (FusedAdamW): nearest | compensated | stochastic
        rounding = dict(rounding=cfg_get(cfg, "optimizer_rounding", "nearest"),
                        seed=int(cfg_get(cfg, "optimizer_rounding_seed", cfg_get(cfg, "seed", 0))))
        self.action_optimizer = FusedAdamW(model.action_expert_parameters, lr=cfg_get(cfg, "action_lr"),
                                           weight_decay=cfg_get(cfg, "action_weight_decay", 0.0),
                                           state_bits=self.state_bits, **rounding)
        sch = lambda opt, key, lr: CosineAnnealingWarmupRestarts(  # noqa: E731
            opt, first_cycle_steps=cfg_get(cfg, f"{key}.first_cycle_steps"), cycle_mult=1.0, max_lr=lr,
            min_lr=cfg_get(cfg, f"{key}.min_lr"), warmup_steps=cfg_get(cfg, f"{key}.warmup_steps"), gamma=1.0)
        self.action_lr_scheduler = sch(self.action_optimizer, "action_lr_scheduler", cfg_get(cfg, "action_lr"))
        self.optimizers = [self.action_optimizer]
        if self.train_vlm:
            vlm_params = model.lora_trainable_vlm_parameters if self.lora else model.trainable_vlm_parameters
            self.vlm_optimizer = FusedAdamW(vlm_params, lr=cfg_get(cfg, "vlm_lr"),
                                            weight_decay=cfg_get(cfg, "vlm_weight_decay", 0.0),
                                            state_bits=self.state_bits, **rounding)
            self.vlm_lr_scheduler = sch(self.vlm_optimizer, "vlm_lr_scheduler", cfg_get(cfg, "vlm_lr"))
            self.optimizers.append(self.vlm_optimizer)
        else:
            for p in model.trainable_vlm_parameters:
                p.requires_grad = False
            if self.main_rank and not model._vlm_needs_grad():
                log.info("train_vlm False: frozen-VLM pass active (VLM forward-only, expert-only backward%s)",
                         "; the frozen VLM region is left out of the all-reduce" if self.multi_gpu else "")
        # several flow draws per observation: S pairs (t, x0) per sample of a micro-batch share its one
        # forward-only VLM prefill.  1 (default): the step as it always was
        fs = cfg_get(cfg, "flow_samples_per_observation", 1)
        self.flow_samples = 1 if fs is None else int(fs)
        if self.flow_samples < 1:
            raise ValueError(f"flow_samples_per_observation must be >= 1, got {self.flow_samples}")
        if self.flow_samples > 1:
            if self.train_vlm or model._vlm_needs_grad():
                from pizero_native.engine import DRAWS_FROZEN_MSG

                raise ValueError(DRAWS_FROZEN_MSG + f" (got train_vlm: {self.train_vlm}, lora: {self.lora})")
            if self.main_rank:
                log.info("flow_samples_per_observation %d: every observation trains on %d flow draws (t, x0) that share "
                         "its one VLM prefill; %d pairs per micro-batch", self.flow_samples, self.flow_samples,
                         per_dev * self.flow_samples)
        self.flow_sampling = cfg_get(cfg, "flow_sampling", "beta")
        self.flow_t_max = 1 - float(cfg_get(cfg, "flow_sig_min", 0.001))
        self.flow_beta_dist = torch.distributions.Beta(float(cfg_get(cfg, "flow_alpha", 1.5)),
                                                       float(cfg_get(cfg, "flow_beta", 1)))
        if resume:
            self.load_optimizer(resume)

        # training-image augmentation on the device: off by default; the parameters of micro-batch
        # cnt_batch are drawn on the host from (image_augment_seed, cnt_batch, rank) alone, so a resumed run draws at a
        # given cnt_batch what the uninterrupted run drew there, and torch's generator (the flow-matching times) is
        # not touched
        self.image_augment = bool(cfg_get(cfg, "image_augment", False))
        if self.image_augment:
            from pizero_native import augment as A

            kw = cfg_get(cfg, "image_augment_kwargs")
            self.image_augment_specs = A.parse_kwargs(kw if kw is not None else A.REFERENCE_PRIMARY)
            self.image_augment_seed = int(cfg_get(cfg, "image_augment_seed", cfg_get(cfg, "seed", 0)))
            self.image_augment_crop_draws = cfg_get(cfg, "image_augment_crop_draws", "shared")
            if self.image_augment_crop_draws not in A.CROP_DRAWS:
                raise ValueError(f"image_augment_crop_draws must be one of {list(A.CROP_DRAWS)}, got "
                                 f"{self.image_augment_crop_draws!r}")

        # action-prefix conditioning: off by default (0: nothing is drawn, the step is the one it always
        # was).  With D > 0 every sample of micro-batch cnt_batch trains with its own first d ~ U{0..D} ground-truth
        # actions as a committed prefix, d drawn on the host from (action_prefix_seed, micro_batches_seen, rank) alone
        self.action_prefix_max_delay = int(cfg_get(cfg, "action_prefix_max_delay", 0) or 0)
        horizon = int(cfg_get(cfg, "horizon_steps"))
        if not 0 <= self.action_prefix_max_delay < horizon:
            raise ValueError(f"action_prefix_max_delay must lie in [0, horizon_steps - 1] = [0, {horizon - 1}], got "
                             f"{self.action_prefix_max_delay}")
        if self.action_prefix_max_delay and cfg_get(cfg, "action_expert_adaptive_mode", None):
            from pizero_native.engine import PREFIX_ADAPTIVE_MSG

            raise NotImplementedError(PREFIX_ADAPTIVE_MSG)
        self.action_prefix_seed = int(cfg_get(cfg, "action_prefix_seed", cfg_get(cfg, "seed", 0)))

        # in-training validation (train.py:132-160,413-459): on with a val_dataset or a ``data.val`` config node
        self.run_eval = val_dataset is not None or cfg_get(cfg, "data.val") is not None
        self.last_eval = None
        if self.run_eval:
            self.eval_freq = int(cfg_get(cfg, "eval_freq", 2000))
            self.eval_thresholds = [float(x) for x in cfg_get(cfg, "eval_thresholds", [0.05, 0.1, 0.2, 0.3, 0.5])]
            self.per_device_num_eval_batch = int(cfg_get(cfg, "eval_size", 1024)) // per_dev // self.world
            if self.per_device_num_eval_batch < 1:
                raise ValueError("eval_size is smaller than one batch per rank (per_device_batch_size x world size)")
            if val_dataset is None:
                val_dataset = self._episode_batches("val", per_dev)
            self.val_dataloader = (val_dataset if val_dataset is not None
                                   else SyntheticBridgeDataset(cfg, per_dev, seed=10_000 + self.rank))
            self.val_dataiterator = None

    def _episode_batches(self, split, per_dev):
        """``data.<split>.episode_store`` -> pizero_native.episodes.EpisodeBatches (None without the key)"""
        if not cfg_get(self.cfg, f"data.{split}.episode_store"):
            return None
        from pizero_native.episodes import from_config

        return from_config(self.cfg, split, per_dev, self.rank, self.world, self.device)

    def sample_fm_time(self, bsz):
        """train.py:239-247."""
        return sample_fm_time(bsz, self.flow_sampling, self.flow_beta_dist, self.flow_t_max)

    def preprocess_batch(self, batch, split_mask=False, sample_fm_time=True, augment=False):
        """train.py:271-314 with the per-batch work on the device: the raw batch
        (int64 ids / attention mask, uint8 pixels, fp32 proprio / actions) is copied once, then the
        block mask + positions (vectorised builder, pizero.py:271-324) and the pixel normalisation
        (x/255 - 0.5)/0.5 (vla/processing.py:109-114) are computed on the GPU -- no per-sample host
        loop, and 1 byte per pixel crosses PCIe instead of 2.  ``augment=True`` (run() passes the config's
        ``image_augment``; evaluate() never does) puts the uint8 frames through the reference's crop and colour
        jitter with this micro-batch's (cnt_batch) parameters instead."""
        m = self.model
        dev = self.device
        nb = dict(non_blocking=True)
        am = batch["attention_mask"].to(dev, **nb)
        mask, vpos, ppos, apos = m.build_causal_mask_and_position_ids(am, self.dtype)
        pix = batch["pixel_values"].to(dev, **nb)
        img = int(cfg_get(self.cfg, "vision.config.image_size"))
        if augment:
            pix = self._augment_frames(pix, img)
        elif pix.dtype == torch.uint8 and pix.dim() == 4 and tuple(pix.shape[-2:]) != (img, img):
            # frames not yet at the model's resolution: the data pipeline's Lanczos-3 resize (dlimp/utils.py:12-17)
            # and the pixel normalisation in one native op; [B, 3, H, W] as the dataset delivers them
            from pizero_native import ops

            pix = ops.image_resize_norm(pix.contiguous(), img, channels_last=False)
        elif pix.dtype == torch.uint8:
            pix = (pix.to(torch.float32) / 255.0 - 0.5) / 0.5
        inputs = {"input_ids": batch["input_ids"].to(dev, **nb), "pixel_values": pix.to(self.dtype),
                  "vlm_position_ids": vpos, "proprio_position_ids": ppos, "action_position_ids": apos,
                  "proprios": batch["proprio"].to(dev, **nb).to(self.dtype),
                  "actions": batch["action"].to(dev, **nb).to(self.dtype)}
        if split_mask:
            inputs["image_text_proprio_mask"], inputs["action_mask"] = m.split_full_mask_into_submasks(mask)
        else:
            inputs["causal_mask"] = mask
        if sample_fm_time:
            bsz, S = len(batch["input_ids"]), self.flow_samples
            t = self.sample_fm_time(bsz * S)
            inputs["t"] = (t.view(bsz, S) if S > 1 else t).to(dev, **nb).to(self.dtype)
            pl = self._prefix_len(batch)
            if pl is not None:
                inputs["prefix_len"] = pl
        return inputs

    def _prefix_len(self, batch):
        """the training step's per-sample prefix lengths: the batch's own ``action_prefix_len`` if it
        carries one, else the draw of this micro-batch with ``action_prefix_max_delay`` > 0, else None"""
        bsz = len(batch["input_ids"])
        if batch.get("action_prefix_len") is not None:
            pl = torch.as_tensor(batch["action_prefix_len"])
        elif self.action_prefix_max_delay > 0:
            from pizero_native import augment as A

            pl = torch.from_numpy(A.draw_prefix_len(bsz, self.action_prefix_max_delay, self.action_prefix_seed,
                                                    self.micro_batches_seen, self.rank))
        else:
            return None
        horizon = int(cfg_get(self.cfg, "horizon_steps"))
        if pl.numel() != bsz or int(pl.min()) < 0 or int(pl.max()) > horizon - 1:
            raise ValueError(f"action_prefix_len: {bsz} integers in [0, horizon_steps - 1] = [0, {horizon - 1}] "
                             f"expected, got {pl.tolist()}")
        return pl.to(torch.int32)

    def _augment_frames(self, pix, img):
        """uint8 [B, 3, H, W] on the device -> bf16 [B, 3, img, img]: the resize first where the frames are not at the
        model's size, then the augmentation, as the reference's pipeline orders them (dlimp/augmentations.py works
        at the resized resolution)."""
        from pizero_native import augment as A
        from pizero_native import ops

        if not self.image_augment:
            raise ValueError("preprocess_batch(augment=True) needs image_augment: True in the config")
        if pix.dtype != torch.uint8 or pix.dim() != 4 or pix.shape[1] != 3:
            raise ValueError("image_augment works on uint8 frames [B, 3, H, W]; got pixel_values of dtype "
                             f"{pix.dtype}, shape {tuple(pix.shape)} (already normalised frames cannot be augmented)")
        pix = pix.contiguous()
        if tuple(pix.shape[-2:]) != (img, img):
            pix = ops.image_resize_u8(pix, img, channels_last=False)
        params, op_mask = A.draw_params(self.image_augment_specs, pix.shape[0], self.image_augment_seed,
                                        self.cnt_batch, self.rank, self.image_augment_crop_draws)
        return ops.image_augment(pix, params, op_mask, channels_last=False)

    def run(self):
        try:
            return self._run()
        finally:  # an episode store's prefetch worker is joined however the loop ends
            for data in (self.train_dataloader, getattr(self, "val_dataloader", None)):
                if hasattr(data, "seek") and hasattr(data, "close"):
                    data.close()

    def _run(self):
        from pizero_native.optim import clip_grad_norm_

        loss_deque = deque(maxlen=self.grad_accumulation_steps)
        self.model_meta.train()
        if hasattr(self.train_dataloader, "seek"):  # a resumed run continues the sampler's sequence
            self.train_dataloader.seek(self.micro_batches_seen)
        it = iter(self.train_dataloader)
        while self.cnt_update < self.n_updates:
            batch = next(it)
            inputs = self.preprocess_batch(batch, augment=self.image_augment)
            last = (self.cnt_batch + 1) % self.grad_accumulation_steps == 0
            ctx = self.model_meta.no_sync() if (self.multi_gpu and not last) else torch.enable_grad()
            with ctx:
                loss = self.model_meta(**inputs)
                (loss / self.grad_accumulation_steps).backward()
            if last:
                clip_grad_norm_(self.optimizers, self.max_grad_norm)
                for opt in self.optimizers:
                    opt.step()
                self.action_lr_scheduler.step()
                if self.train_vlm:
                    self.vlm_lr_scheduler.step()
                for opt in self.optimizers:
                    opt.zero_grad(set_to_none=True)
                self.cnt_update += 1
                self.model_averaging.maybe_initialize(self.cnt_update)
                self.model_averaging.maybe_update(self.cnt_update)
                if ((self.cnt_update % self.save_model_freq == 0 and self.cnt_update > self.save_model_start)
                        or self.cnt_update == self.n_updates):
                    self.save_training(self.cnt_update, self.cnt_batch)
            # every micro-batch's loss enters the window (kept on the device: no sync), as the reference's
            # deque of grad_accumulation_steps rank-mean losses (train.py:405-463); the window is all-reduced
            # ONCE, on the logged batches only (every rank has the same cnt_batch, so all enter the collective)
            loss_deque.append(loss.detach().reshape(1).float())
            if self.run_eval and (self.cnt_batch + 1) % self.eval_freq == 0:
                self.evaluate()
            if self.cnt_batch % self.log_freq == 0:
                win = torch.cat(list(loss_deque))
                if self.multi_gpu:
                    torch.distributed.all_reduce(win, op=torch.distributed.ReduceOp.SUM)
                    win = win / self.world
                if self.main_rank:
                    log.info("Batch %d Update %d: loss %.4f | action lr %.8f", self.cnt_batch, self.cnt_update,
                             float(win.mean()), self.action_optimizer.param_groups[0]["lr"])
            self.cnt_batch += 1
            self.micro_batches_seen += 1
        return self

    # ----------------------------------------------------------- validation --
    def evaluate(self):
        """train.py:413-459: ``per_device_num_eval_batch`` validation batches through ``infer_action`` on the averaged
        weights (the live ones before averaging starts), action accuracy per threshold and L1 loss, averaged over
        batches and ranks.  The live weights and train mode are restored.  Returns (and keeps as ``last_eval``)
        {"l1": float, "accuracy": [float per threshold], "cnt_batch": int}."""
        from src.utils.metric import get_action_accuracy

        n = self.per_device_num_eval_batch
        if self.main_rank:
            log.info("Running evaluation for %d batches...", n)
        if self.val_dataiterator is None:
            self.val_dataiterator = iter(self.val_dataloader)
        acc = torch.zeros(len(self.eval_thresholds), device=self.device)
        l1 = torch.tensor(0.0, device=self.device)
        D = self.action_prefix_max_delay
        l1_suffix = torch.tensor(0.0, device=self.device)
        self.model_meta.eval()
        try:
            with self.model_averaging.averaged_weights() as model_eval, torch.no_grad():
                for _ in range(n):
                    inputs = self.preprocess_batch(next(self.val_dataiterator), split_mask=True, sample_fm_time=False)
                    gt_actions = inputs.pop("actions")
                    if D > 0:  # infer_action's own draw, made here so that both chunks start from the same noise
                        inputs["noise"] = torch.randn(gt_actions.shape, device=self.device, dtype=torch.float32)
                    preds = model_eval.infer_action(**inputs)
                    acc += get_action_accuracy(gt_actions, preds, self.eval_thresholds)
                    l1 += torch.nn.functional.l1_loss(preds, gt_actions)
                    if D > 0:  # the chunk again around its ground-truth first D actions: L1 over the rows it fills in
                        cond = model_eval.infer_action(**inputs, prefix_actions=gt_actions.float(),
                                                       prefix_len=torch.full((len(gt_actions),), D))
                        l1_suffix += torch.nn.functional.l1_loss(cond[:, D:], gt_actions[:, D:].float())
        finally:
            self.model_meta.train()
        acc /= n
        l1 /= n
        l1_suffix /= n
        if self.multi_gpu:
            torch.distributed.all_reduce(acc, op=torch.distributed.ReduceOp.SUM)
            torch.distributed.all_reduce(l1, op=torch.distributed.ReduceOp.SUM)
            acc /= self.world
            l1 /= self.world
            if D > 0:
                torch.distributed.all_reduce(l1_suffix, op=torch.distributed.ReduceOp.SUM)
                l1_suffix /= self.world
        self.last_eval = {"l1": float(l1), "accuracy": [float(x) for x in acc], "cnt_batch": int(self.cnt_batch)}
        if D > 0:
            self.last_eval["l1_prefix_suffix"] = float(l1_suffix)
        if self.main_rank:
            log.info("Eval | l1 Loss: %.3f | %s", self.last_eval["l1"],
                     " | ".join(f"acc thres {t}: {a:.3f}" for t, a in zip(self.eval_thresholds,
                                                                          self.last_eval["accuracy"])))
            if D > 0:
                log.info("Eval | l1 Loss over rows >= %d around the ground-truth first %d actions: %.3f", D, D,
                         self.last_eval["l1_prefix_suffix"])
        return self.last_eval

    # ---------------------------------------------------------- checkpoints --
    def save_training(self, cnt_update, cnt_batch):
        if not self.main_rank or not cfg_get(self.cfg, "log_dir"):
            return None
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        # train.py:500-512: once averaging is active "model" holds the AVERAGED weights (read from the average buffer:
        # the same bits the model computes with inside averaged_weights()) and n_averaged their count
        avg_state = self.model_averaging.state_dict()
        weights = avg_state["state_dict"] if avg_state else self.model.state_dict()
        data = {
            "cnt_update": cnt_update, "cnt_batch": cnt_batch,
            "model": {k: v.detach().clone() for k, v in weights.items()},
            "action_optimizer": self.action_optimizer.state_dict(),
            "vlm_optimizer": self.vlm_optimizer.state_dict() if self.train_vlm else None,
            "action_lr_scheduler": self.action_lr_scheduler.state_dict(),
            "vlm_lr_scheduler": self.vlm_lr_scheduler.state_dict() if self.train_vlm else None,
            "wandb_id": None, "n_averaged": avg_state.get("n_averaged", 1),
        }
        if avg_state:  # extension: the live weights, so that a resumed run continues both exactly
            data["model_train"] = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        path = os.path.join(self.checkpoint_dir, f"step{cnt_update}.pt")
        torch.save(data, path)
        return path

    def load_checkpoint(self, path):
        """train.py:531-544: counters + weights (strict, ``_orig_mod.`` prefix of compiled saves stripped).
        With averaging enabled and a checkpoint that holds "model_train": live <- "model_train", and "model" with
        n_averaged is kept for the average (restored once ModelAveraging is built)."""
        data = torch.load(path, weights_only=True, map_location="cpu")
        self.cnt_update = int(data["cnt_update"])
        self.cnt_batch = int(data["cnt_batch"])
        self.micro_batches_seen = self.cnt_batch + 1  # the checkpoint was written after micro-batch cnt_batch
        self.wandb_id = data.get("wandb_id")
        sd = {k.replace("_orig_mod.", ""): v for k, v in data["model"].items()}
        if self._averaging_enabled and data.get("model_train") is not None:
            self._resume_average = (sd, int(data.get("n_averaged", 1)))
            sd = data["model_train"]
        self.model.load_state_dict(sd, strict=True)
        log.info("Loaded model from %s at update %d batch %d", path, self.cnt_update, self.cnt_batch)
        return data

    def load_optimizer(self, path):
        """train.py:546-560: optimizer moments/steps and scheduler states."""
        data = torch.load(path, weights_only=True, map_location="cpu")
        self.action_optimizer.load_state_dict(data["action_optimizer"])
        self.action_lr_scheduler.load_state_dict(data["action_lr_scheduler"])
        if self.train_vlm:
            self.vlm_optimizer.load_state_dict(data["vlm_optimizer"])
            self.vlm_lr_scheduler.load_state_dict(data["vlm_lr_scheduler"])
        log.info("Loaded optimizer and scheduler states from %s", path)
