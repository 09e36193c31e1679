"""numpy restatement of the 4-bit base-weight format of QLoRA: TEST INFRASTRUCTURE, the pin of
pz_q4_quantize / pz_q4_dequant (csrc/pz_q4.hip) and of the nested step (pizero_native/quant4.py).

Sources: the public storage format of bitsandbytes 0.45 (Linear4bit / Params4bit, blocksize 64, compress_statistics)
and Dettmers et al., "QLoRA" (2023).  bitsandbytes is not installed where this project builds, so parity with its own
kernels (whose decision thresholds are hand-typed constants) is UNPINNED; the pin is this restatement.

One Linear weight, flattened row-major, n = out * in (n even):
  1. bf16 -> fp16 (RNE; Params4bit.cuda does .half())
  2. blocks of 64 consecutive elements, the last one may be short
  3. absmax = fp32 max |x| of the block; inv = float32(1) / absmax (correctly rounded; 0 for an all-zero block);
     the normalised value is float32(x) * inv
  4. code = nearest table entry: thresholds are the fp32 midpoints (a + b) * 0.5 of adjacent sorted table values,
     x > mid picks the upper one; fp4: sign bit = x < 0, the 3 magnitude bits are chosen on |x|
  5. two codes per byte, the element of even index in the high nibble
  6. double quantisation, per Linear: offset = float32(mean of absmax in fp64); absmax - offset in blocks of 256
     through the signed dynamic map of the 8-bit optimizer (oracle.adamw8bit: create_dynamic_map(True), quantize), the
     value normalised by an fp32 division by the block's nested_absmax = max |absmax - offset| (0 for a zero block)
  7. dequantisation: absmax' = float32(qmap[code] * nested_absmax) + offset; w = float32(table[nibble] * absmax'),
     rounded to fp16 (RNE), then to bf16 (RNE) -- bitsandbytes dequantises to fp16 and casts to the compute dtype.
Every product and sum is rounded by itself (no FMA).
"""

from __future__ import annotations

import json

import numpy as np

from oracle import adamw8bit as O8

BLOCK = 64
NESTED_BLOCK = 256
F = np.float32

# fp4: magnitudes of codes 0..7, bit 3 is the sign
FP4_MAG = np.array([0.0, 0.0052083333, 0.66666667, 1.0, 0.33333333, 0.5, 0.16666667, 0.25], dtype=F)
FP4 = np.concatenate([FP4_MAG, -FP4_MAG]).astype(F)
# nf4: the 16 NormalFloat values of the QLoRA paper (appendix E)
NF4 = np.array([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
                -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
                0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941,
                0.7229568362236023, 1.0], dtype=F)
TABLES = {"fp4": FP4, "nf4": NF4}


def bf16_bits_to_f32(u16: np.ndarray) -> np.ndarray:
    return (np.asarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(F)


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 -> nearest-even bf16 bit patterns (finite inputs)"""
    u = np.asarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _midpoints(sorted_vals: np.ndarray) -> np.ndarray:
    return ((sorted_vals[:-1] + sorted_vals[1:]) * F(0.5)).astype(F)


def codes_of(xn: np.ndarray, qtype: str) -> np.ndarray:
    """4-bit codes of the normalised fp32 values"""
    xn = np.asarray(xn, dtype=F)
    if qtype == "nf4":
        mids = _midpoints(NF4)
        return (xn[..., None] > mids).sum(-1).astype(np.uint8)
    if qtype == "fp4":
        order = np.argsort(FP4_MAG, kind="stable")  # magnitude rank -> code
        mids = _midpoints(FP4_MAG[order])
        rank = (np.abs(xn)[..., None] > mids).sum(-1)
        return (order[rank] | ((xn < 0).astype(np.int64) << 3)).astype(np.uint8)
    raise ValueError(f"quantize_type must be fp4 or nf4, got {qtype!r}")


def quantize_blocks(w_bf16_bits: np.ndarray, qtype: str):
    """(packed uint8 [n / 2], absmax fp32 [ceil(n / 64)]) of a flat bf16 tensor given as uint16 bit patterns"""
    n = w_bf16_bits.size
    if n % 2:
        raise ValueError("n must be even")
    with np.errstate(over="ignore"):
        x = bf16_bits_to_f32(w_bf16_bits.reshape(-1)).astype(np.float16).astype(F)
    nb = (n + BLOCK - 1) // BLOCK
    xp = np.concatenate([x, np.zeros(nb * BLOCK - n, F)]).reshape(nb, BLOCK)
    absmax = np.abs(xp).max(1).astype(F)
    with np.errstate(divide="ignore"):
        inv = np.where(absmax > 0, F(1.0) / np.where(absmax > 0, absmax, F(1)), F(0)).astype(F)
    c = codes_of((xp * inv[:, None]).astype(F), qtype).reshape(-1)[:n]
    return ((c[0::2] << 4) | c[1::2]).astype(np.uint8), absmax


def nested_quantize(absmax: np.ndarray):
    """(codes uint8 [nb], nested_absmax fp32 [ceil(nb / 256)], offset fp32 scalar, qmap fp32 [256])"""
    absmax = np.asarray(absmax, dtype=F)
    qmap = O8.create_dynamic_map(True)
    offset = F(absmax.astype(np.float64).mean())
    d = (absmax - offset).astype(F)
    nb = d.size
    nn = (nb + NESTED_BLOCK - 1) // NESTED_BLOCK
    dp = np.concatenate([d, np.zeros(nn * NESTED_BLOCK - nb, F)]).reshape(nn, NESTED_BLOCK)
    nam = np.abs(dp).max(1).astype(F)
    xn = np.where(nam[:, None] > 0, dp / np.where(nam > 0, nam, F(1))[:, None], F(0)).astype(F)
    codes = O8.quantize(xn, qmap, True).reshape(-1)[:nb]
    return codes, nam, offset, qmap


def nested_dequantize(codes, nam, offset, qmap) -> np.ndarray:
    blk = np.arange(codes.size) // NESTED_BLOCK
    return ((qmap[codes] * nam[blk]).astype(F) + F(offset)).astype(F)


def dequantize(packed, codes, nam, offset, qmap, qtype: str, n: int) -> np.ndarray:
    """bf16 bit patterns (uint16 [n]) of the dequantised weight"""
    table = TABLES[qtype]
    absmax = nested_dequantize(codes, nam, offset, qmap)
    nib = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:n]
    w = (table[nib] * absmax[np.arange(n) // BLOCK]).astype(F)
    return f32_to_bf16_bits(w.astype(np.float16).astype(F))


def quantize(w_bf16_bits: np.ndarray, qtype: str) -> dict:
    """the whole quantised state of one Linear weight"""
    packed, absmax = quantize_blocks(w_bf16_bits, qtype)
    codes, nam, offset, qmap = nested_quantize(absmax)
    return dict(packed=packed, absmax=codes, nested_absmax=nam, offset=offset, qmap=qmap, qtype=qtype,
                n=int(w_bf16_bits.size))


def roundtrip(w_bf16_bits: np.ndarray, qtype: str) -> np.ndarray:
    q = quantize(w_bf16_bits, qtype)
    return dequantize(q["packed"], q["absmax"], q["nested_absmax"], q["offset"], q["qmap"], qtype, q["n"])


# ---- state_dict layout (bitsandbytes 0.45 packed format, restated) ---------------------------------------------------
def state_keys(qtype: str):
    return ["weight", "weight.absmax", "weight.quant_map", "weight.nested_absmax", "weight.nested_quant_map",
            f"weight.quant_state.bitsandbytes__{qtype}"]


def quant_state_blob(qtype: str, shape, offset) -> np.ndarray:
    d = {"quant_type": qtype, "blocksize": BLOCK, "dtype": "bfloat16", "shape": [int(s) for s in shape],
         "nested_blocksize": NESTED_BLOCK, "nested_dtype": "float32", "nested_offset": float(offset)}
    return np.frombuffer(json.dumps(d).encode("utf-8"), dtype=np.uint8).copy()


def parse_blob(blob: np.ndarray) -> dict:
    return json.loads(bytes(np.asarray(blob, dtype=np.uint8)).decode("utf-8"))
