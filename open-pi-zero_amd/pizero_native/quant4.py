"""4-bit base weights of QLoRA (quantize: True): the packed state of every quantised Linear.

Format (bitsandbytes 0.45's public storage format, restated in tests/quant4_ref.py; parity with bitsandbytes' own
kernels is unpinned): codes into the 16-entry fp4 / nf4 table in blocks of 64, two per byte; the fp32 block scales
minus their mean (``offset``) quantised again in blocks of 256 through the signed 8-bit dynamic map.  pz_q4_quantize
makes the codes and the block scales; the nested step runs once per load in torch (elementwise fp32 arithmetic and
max reductions, whose results do not depend on the order; the mean is taken in fp64 on the host).  pz_q4_dequant is
the per-step kernel.
"""

from __future__ import annotations

import json
from dataclasses import dataclass

import numpy as np
import torch

from . import ops

BLOCK = 64
NESTED_BLOCK = 256
QTYPES = ("fp4", "nf4")
FP4_MAG = (0.0, 0.0052083333, 0.66666667, 1.0, 0.33333333, 0.5, 0.16666667, 0.25)
NF4 = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
       -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
       0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)
SUFFIXES = ("absmax", "quant_map", "nested_absmax", "nested_quant_map")


def check_qtype(qtype):
    if qtype not in QTYPES:
        raise ValueError(f"quantize_type must be fp4 or nf4, got {qtype!r}")
    return qtype


def table(qtype) -> torch.Tensor:
    check_qtype(qtype)
    return torch.tensor(NF4 if qtype == "nf4" else FP4_MAG + tuple(-m for m in FP4_MAG), dtype=torch.float32)


def state_keys(qtype):
    """state_dict keys of one quantised ``weight``, in the order they are emitted"""
    return ["weight"] + [f"weight.{s}" for s in SUFFIXES] + [f"weight.quant_state.bitsandbytes__{check_qtype(qtype)}"]


def quant_state_blob(qtype, shape, offset) -> torch.Tensor:
    """the non-tensor part of the state as a uint8 JSON blob (bitsandbytes' QuantState.as_dict(packed=True))"""
    d = {"quant_type": check_qtype(qtype), "blocksize": BLOCK, "dtype": "bfloat16", "shape": [int(s) for s in shape],
         "nested_blocksize": NESTED_BLOCK, "nested_dtype": "float32", "nested_offset": float(offset)}
    return torch.from_numpy(np.frombuffer(json.dumps(d).encode("utf-8"), dtype=np.uint8).copy())


def parse_quant_state(blob) -> dict:
    d = json.loads(bytes(blob.detach().cpu().to(torch.uint8).numpy()).decode("utf-8"))
    if d.get("blocksize") != BLOCK or d.get("nested_blocksize") != NESTED_BLOCK:
        raise ValueError(f"4-bit state with blocksize {d.get('blocksize')} / nested {d.get('nested_blocksize')}: "
                         f"only {BLOCK} / {NESTED_BLOCK} (compress_statistics) is supported")
    check_qtype(d.get("quant_type"))
    return d


def _dynamic_codes(x, qmap):
    """uint8 codes of fp32 x in [-1, 1]: the 7-step binary search with midpoint rounding of the 8-bit optimizer's
    signed dynamic map (oracle/adamw8bit.py quantize), elementwise"""
    pivot = torch.full_like(x, 127, dtype=torch.int64)
    upper_p, lower_p = torch.full_like(pivot, 255), torch.zeros_like(pivot)
    lower, upper = torch.full_like(x, -1.0), torch.ones_like(x)
    val = qmap[pivot]
    i = 64
    while i > 0:
        gt = x > val
        lower_p, lower = torch.where(gt, pivot, lower_p), torch.where(gt, val, lower)
        upper_p, upper = torch.where(gt, upper_p, pivot), torch.where(gt, upper, val)
        pivot = torch.where(gt, pivot + i, pivot - i)
        val = qmap[pivot]
        i >>= 1
    gt = x > val
    mid_up, mid_lo = (upper + val) * 0.5, (lower + val) * 0.5
    code = torch.where(gt, torch.where(x > mid_up, upper_p, pivot), torch.where(x < mid_lo, lower_p, pivot))
    return code.to(torch.uint8)


def nested_quantize(absmax, qmap):
    """(codes uint8 [nb], nested_absmax fp32 [ceil(nb / 256)], offset): double quantisation of the block scales"""
    offset = float(np.float32(absmax.detach().cpu().numpy().astype(np.float64).mean()))
    d = absmax - offset
    nb = d.numel()
    nn_ = (nb + NESTED_BLOCK - 1) // NESTED_BLOCK
    dp = torch.zeros(nn_ * NESTED_BLOCK, device=d.device, dtype=torch.float32)
    dp[:nb] = d
    dp = dp.view(nn_, NESTED_BLOCK)
    nam = dp.abs().amax(1)
    pos = nam > 0
    xn = torch.where(pos[:, None], dp / torch.where(pos, nam, torch.ones_like(nam))[:, None], torch.zeros_like(dp))
    return _dynamic_codes(xn, qmap).view(-1)[:nb].contiguous(), nam.contiguous(), offset


@dataclass
class Q4Weight:
    packed: torch.Tensor         # uint8 [n / 2]
    absmax: torch.Tensor         # uint8 [ceil(n / 64)]: codes of the block scales
    nested_absmax: torch.Tensor  # fp32 [ceil(nb / 256)]
    offset: float
    shape: tuple
    n: int

    def nbytes(self):
        return self.packed.numel() + self.absmax.numel() + 4 * self.nested_absmax.numel() + 4

    def seg(self, dst):
        return (self.packed, self.absmax, self.nested_absmax, self.offset, self.n, dst)


class Q4Store:
    """name -> Q4Weight of every quantised Linear weight of one model, and the shared tables"""

    def __init__(self, qtype, device):
        from .optim import create_dynamic_map

        self.qtype = check_qtype(qtype)
        self.qmap = create_dynamic_map(True).to(device)
        self.table = table(qtype).to(device)
        self.w: dict[str, Q4Weight] = {}

    def quantize(self, name, w):
        """pack the bf16 weight ``w`` (any shape, contiguous) under ``name``"""
        n = w.numel()
        if n % 2:
            raise ValueError(f"{name}: {n} elements; a 4-bit weight needs an even count (two codes per byte)")
        flat = w.detach().reshape(-1)
        packed = torch.empty(n // 2, device=w.device, dtype=torch.uint8)
        absmax = torch.empty((n + BLOCK - 1) // BLOCK, device=w.device, dtype=torch.float32)
        ops.q4_quantize(flat, packed, absmax, self.qtype)
        codes, nam, offset = nested_quantize(absmax, self.qmap)
        self.w[name] = Q4Weight(packed, codes, nam, offset, tuple(w.shape), n)
        return self.w[name]

    def dequant(self, names, dst):
        """the bf16 weights ``names`` into the flat bf16 buffer ``dst``, one after another (every size a multiple of
        8 elements, as the arena's spans are), one launch"""
        segs, off = [], 0
        for nm in names:
            q = self.w[nm]
            segs.append(q.seg(dst[off:off + q.n]))
            off += q.n
        ops.q4_dequant(segs, self.qmap, self.qtype)
        return dst[:off]

    def entries(self, name):
        """the state_dict tensors of ``name`` (a ``...weight`` key), by key suffix after ``weight``"""
        q = self.w[name]
        return {"": q.packed.view(-1, 1), ".absmax": q.absmax, ".quant_map": self.table,
                ".nested_absmax": q.nested_absmax, ".nested_quant_map": self.qmap,
                f".quant_state.bitsandbytes__{self.qtype}": quant_state_blob(self.qtype, q.shape, q.offset)}

    def install(self, name, shape, ent, device):
        """take the packed tensors of a state_dict (``entries``' keys) without requantising"""
        key = next((k for k in ent if k.startswith(".quant_state.bitsandbytes__")), None)
        missing = [k for k in ("", ".absmax", ".nested_absmax") if k not in ent]
        if key is None or missing:
            lost = [name + k for k in missing] + ([name + ".quant_state.bitsandbytes__" + self.qtype] if key is None else [])
            raise RuntimeError(f"Error(s) in loading state_dict: a packed 4-bit weight needs all of its tensors, "
                               f"missing keys {lost}")
        st = parse_quant_state(ent[key])
        if st["quant_type"] != self.qtype:
            raise ValueError(f"{name}: checkpoint holds {st['quant_type']} codes, the model is configured for "
                             f"quantize_type: {self.qtype}")
        if tuple(st["shape"]) != tuple(shape):
            raise ValueError(f"{name}: packed weight of shape {tuple(st['shape'])}, expected {tuple(shape)}")
        n = 1
        for s in shape:
            n *= int(s)
        nb = (n + BLOCK - 1) // BLOCK
        packed = ent[""].to(device=device, dtype=torch.uint8).reshape(-1).contiguous().clone()
        codes = ent[".absmax"].to(device=device, dtype=torch.uint8).reshape(-1).contiguous().clone()
        nam = ent[".nested_absmax"].to(device=device, dtype=torch.float32).reshape(-1).contiguous().clone()
        if packed.numel() != n // 2 or codes.numel() != nb or nam.numel() != (nb + NESTED_BLOCK - 1) // NESTED_BLOCK:
            raise ValueError(f"{name}: packed 4-bit tensors do not fit a weight of shape {tuple(shape)}")
        self.w[name] = Q4Weight(packed, codes, nam, float(np.float32(st["nested_offset"])), tuple(shape), n)
        return self.w[name]

    def nbytes(self):
        return sum(q.nbytes() for q in self.w.values())

    def apply(self, fn):
        """follow a Module._apply (.to / .cuda): the device only -- the scales stay fp32 whatever dtype is asked for"""
        dev = fn(torch.empty(0, device=self.qmap.device, dtype=torch.uint8)).device
        self.qmap, self.table = self.qmap.to(dev), self.table.to(dev)
        for q in self.w.values():
            q.packed, q.absmax, q.nested_absmax = q.packed.to(dev), q.absmax.to(dev), q.nested_absmax.to(dev)
