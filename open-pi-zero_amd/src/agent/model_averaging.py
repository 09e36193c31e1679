"""ModelAveraging: the reference's EMA / SWA switch (src/agent/model_averaging.py) on the flat arena.

Same import path, constructor, config keys and methods as the reference's class, which drives
``torch.optim.swa_utils.AveragedModel``; the schedule is restated from that class as the reference calls it:

  * ``maybe_initialize(cnt_update)``: at ``cnt_update == ema_start`` / ``swa_start`` the average becomes a copy of
    the live weights with ``n_averaged = 0``;
  * ``maybe_update(cnt_update)``: once started, every ``ema_freq`` / ``swa_freq`` updates: a copy while
    ``n_averaged == 0``, else ``avg <- lerp(avg, live, w)`` with ``w = 1 - ema_decay`` (EMA) or
    ``w = float32(1) / float32(n_averaged + 1)`` (SWA); then ``n_averaged += 1``.

``n_averaged`` is a host int (no device sync).  The average is a ``pizero_native.averaging.FlatAverage``: one more
flat bf16 buffer on the rank's GPU (6.5 GB at bridge dims), updated by ``pz_avg_lerp`` bit-identically to torch's
bf16 lerp.  ``ema_device`` / ``swa_device`` other than that GPU (the reference defaults ``swa_device: cpu``) are
accepted and logged: there is no CPU copy.

SWA deviation: with ``swa_device: cpu`` the reference takes torch's per-tensor path ``avg + (p - avg) / (n + 1)``
(a bf16 result per op); on a GPU device it takes the foreach-lerp path.  This class implements the lerp form for
both.

Using the averaged model: the native model is bound to one arena, so there is no second module.
``averaged_weights()`` is a context manager inside which the model computes with the averaged weights (a no-op
before the start); ``get_model_module()`` returns the model for use inside it.  Unlike the reference's class, the
average can be resumed (``load_average``).
"""

from __future__ import annotations

import logging
from contextlib import contextmanager

import numpy as np
import torch

log = logging.getLogger(__name__)


class ModelAveraging:
    def __init__(self, model, cfg, device):
        self.use_ema = cfg.get("use_ema", False)
        self.use_swa = cfg.get("use_swa", False)
        assert not (self.use_ema and self.use_swa), "Cannot use both EMA and SWA at once"
        self.model = model
        self.device = device
        self.model_avg = None  # FlatAverage once started: nothing is allocated before
        self.n_averaged = 0
        if self.use_ema:
            self.ema_start = cfg["ema_start"]
            self.ema_decay = cfg.get("ema_decay", 0.99)
            self.ema_freq = cfg.get("ema_freq", 1)
            self.ema_device = self._accept_device("ema_device", cfg.get("ema_device", device))
        if self.use_swa:
            self.swa_start = cfg["swa_start"]
            self.swa_freq = cfg["swa_freq"]
            self.swa_device = self._accept_device("swa_device", cfg.get("swa_device", "cpu"))

    def _accept_device(self, key, value):
        own = torch.device(self.device)
        want = torch.device(value) if value is not None else own
        if want.type != own.type or (want.index is not None and own.index is not None and want.index != own.index):
            log.info("%s: %s is ignored: the averaged weights stay on %s (no CPU path)", key, value, own)
        return own

    @property
    def enabled(self):
        return bool(self.use_ema or self.use_swa)

    @property
    def active(self):
        return self.model_avg is not None

    def _start(self):
        from pizero_native.averaging import FlatAverage

        self.model_avg = FlatAverage.for_model(self.model)
        self.n_averaged = 0

    def maybe_initialize(self, cnt_update):
        if self.use_swa and cnt_update == self.swa_start:
            self._start()
            log.info("Starting SWA...")
        if self.use_ema and cnt_update == self.ema_start:
            self._start()
            log.info("Starting EMA with decay %s...", self.ema_decay)

    def _update(self):
        if self.n_averaged == 0:
            self.model_avg.copy_from_live()
        elif self.use_ema:
            self.model_avg.update(1.0 - self.ema_decay)
        else:
            self.model_avg.update(float(np.float32(1.0) / np.float32(self.n_averaged + 1)))
        self.n_averaged += 1

    def maybe_update(self, cnt_update):
        if self.model_avg is None:
            return
        if self.use_ema and cnt_update % self.ema_freq == 0:
            self._update()
            log.info("EMA updated")
        if self.use_swa and cnt_update % self.swa_freq == 0:
            self._update()
            log.info("SWA updated")

    def get_model_module(self):
        """the model: it computes with the averaged weights inside ``averaged_weights()``"""
        return self.model

    @contextmanager
    def averaged_weights(self):
        if self.model_avg is None:
            yield self.model
            return
        with self.model_avg.swapped():
            yield self.model

    def state_dict(self) -> dict:
        if self.model_avg is None:
            return {}
        return {"state_dict": self.model_avg.state_dict(),
                "n_averaged": torch.tensor(self.n_averaged, dtype=torch.long),
                "model_type": "ema" if self.use_ema else "swa"}

    def load_average(self, state_dict, n_averaged):
        """Resume: the average <- a saved averaged state_dict (the live weights are loaded by the caller first)."""
        self._start()
        own = self.model_avg.state_dict()
        with torch.no_grad():
            for k, v in state_dict.items():
                if k in own:
                    own[k].copy_(v.to(own[k].device, own[k].dtype))
        self.n_averaged = int(n_averaged)
