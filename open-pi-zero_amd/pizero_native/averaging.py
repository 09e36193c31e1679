"""Averaged weights (EMA / SWA) as a second flat buffer beside the parameter arena.

The reference averages with ``torch.optim.swa_utils.AveragedModel`` (src/agent/model_averaging.py): a deep copy of
the module tree updated by ``_foreach_lerp_`` over ~1,000 tensors.  Here every weight already lives in one flat
buffer (arena.py), so the averaged model is ONE more buffer with the arena's layout and an update is one
``pz_avg_lerp`` launch per contiguous run of trained parameters (a handful), bit-identical to ``torch.lerp`` on bf16.

Frozen tensors are skipped: they never move, and lerp(a, a, w) == a, so the average keeps its initial copy of them
(what matters under LoRA, where almost everything is frozen).  The one value for which skipping is not what a lerp
would compute is a frozen -0.0, which torch's lerp turns into +0.0 and the skipped copy keeps.

The native model is bound to its arena (views, captured graphs, the engine's cached pointers), so the averaged model
is not a second module: ``swapped()`` exchanges the CONTENTS of the two buffers in place (``pz_avg_swap``, no
temporary) and exchanges them back on exit.  Addresses never change, so captured inference graphs stay valid; the
arena's version counter is bumped on both edges, which is what the weight-derived caches (fp8 codes, the LoRA merged
shadow, the batch-3 scale cache) key on through ``Engine.weights_version()``.

bf16 only (as ``pz_adamw``): the reference averages in the model's dtype, bf16 in training.
"""

from __future__ import annotations

from contextlib import contextmanager

import torch
from torch.autograd.graph import increment_version

from . import ops
from .optim import contiguous_runs


class FlatAverage:
    def __init__(self, arena, parameters, state_dict_fn=None):
        """arena: the object owning the flat buffer as ``.data`` (arena.Arena); parameters: the nn.Parameters viewing
        it, or a callable returning them (read at every update: requires_grad may change); state_dict_fn: returns the
        live ``state_dict()`` whose keys / shapes ``state_dict()`` mirrors.  Copies the live weights once."""
        data = arena.data
        if data.dtype != torch.bfloat16 or data.device.type != "cuda":
            raise TypeError(f"FlatAverage needs a bf16 arena on the GPU (got {data.dtype} on {data.device}): "
                            "the averaging kernels are bf16-only, like the fused AdamW")
        self.arena = arena
        self._parameters = parameters if callable(parameters) else (lambda ps=list(parameters): ps)
        self._state_dict_fn = state_dict_fn
        self.avg = torch.empty_like(data)
        self._runs = None
        self._swapped = False
        self.copy_from_live()

    @classmethod
    def for_model(cls, model):
        """over a native PiZero (or any module with ``_arena`` whose parameters are views of it)"""
        return cls(model._arena, lambda: list(model.parameters()), model.state_dict)

    def _live(self):
        data = self.arena.data
        if data.data_ptr() != self._live_ptr or data.numel() != self.avg.numel():
            raise RuntimeError("FlatAverage: the arena was rebuilt or moved after the average was created "
                               "(tie / .to() must come before averaging starts)")
        return data

    @torch.no_grad()
    def copy_from_live(self):
        """avg <- the live weights (the whole buffer: frozen tensors and padding included)"""
        if self._swapped:
            raise RuntimeError("FlatAverage.copy_from_live inside swapped()")
        self._live_ptr = self.arena.data.data_ptr()
        self.avg.copy_(self.arena.data)

    def _trainable_runs(self):
        """[(flat live view, element offset)] of the contiguous runs of parameters with requires_grad; rebuilt only
        when the set of trained parameters changes"""
        ps = [p for p in self._parameters() if p.requires_grad]
        key = tuple(p.data_ptr() for p in ps)
        if self._runs is None or self._runs[0] != key:
            self._runs = (key, [(flat, off) for flat, _, off in contiguous_runs(ps)])
        return self._runs[1]

    @torch.no_grad()
    def update(self, w):
        """avg <- lerp(avg, live, w) over the trained parameters (one launch per contiguous run)"""
        if self._swapped:
            raise RuntimeError("FlatAverage.update inside swapped()")
        data = self._live()
        base = data.data_ptr()
        for flat, off in self._trainable_runs():
            if flat.data_ptr() != base + off * data.element_size():
                raise RuntimeError("FlatAverage: a trained parameter is not a view of the arena")
            ops.avg_lerp(self.avg[off:off + flat.numel()], flat, w)

    @contextmanager
    def swapped(self):
        """Inside, the model computes with the averaged weights (and the average buffer holds the live ones)."""
        if self._swapped:
            raise RuntimeError("FlatAverage.swapped() is not re-entrant")
        data = self._live()
        with torch.no_grad():
            ops.avg_swap(data, self.avg)
        increment_version(data)
        self._swapped = True
        try:
            yield self
        finally:
            with torch.no_grad():
                ops.avg_swap(data, self.avg)
            increment_version(data)
            self._swapped = False

    def state_dict(self):
        """The model's state_dict() keys, shapes and dtypes, as views of the average buffer (tied keys alias one
        tensor, as in the live state_dict); tensors that are not arena views (buffers) are passed through."""
        if self._state_dict_fn is None:
            raise RuntimeError("FlatAverage.state_dict needs state_dict_fn")
        data = self._live()
        buf = data if self._swapped else self.avg  # inside swapped() the average sits in the arena
        lo, es = data.data_ptr(), data.element_size()
        hi = lo + data.numel() * es
        out = {}
        for k, v in self._state_dict_fn().items():
            if isinstance(v, torch.Tensor) and v.device == data.device and lo <= v.data_ptr() < hi and v.numel() > 0:
                if v.dtype != data.dtype or not v.is_contiguous():
                    raise RuntimeError(f"FlatAverage.state_dict: {k} is not a contiguous {data.dtype} arena view")
                off = (v.data_ptr() - lo) // es
                out[k] = buf[off:off + v.numel()].view(v.shape)
            else:
                out[k] = v
        return out
