"""pz_q4_quantize / pz_q4_dequant (csrc/pz_q4.hip) against the numpy restatement tests/quant4_ref.py, bit for bit
(DESIGN 7j): fp4 and nf4; sizes with a short last block, a ragged nested block, rows that are no multiple of 64 and
more than one workgroup; all-zero blocks, a block whose max is negative, values on a decision threshold, bf16 values
below the fp16 normal range, +-0; NaN-filled outputs with guard elements; two runs; the refusal of an odd n."""

import numpy as np
import pytest
import torch

from tests import quant4_ref as R
from tests.qlora_helpers import bits_of, tensor_of

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [64, 72, 64 * 257 + 8, 136 * 64, 4304 * 8]
GUARD = 24


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _weights(n, qtype, seed):
    """bf16 bit patterns [n] with the edge cases planted in whole blocks where n allows"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(n) * 0.04).astype(F)
    table = R.TABLES[qtype]
    srt = np.sort(np.unique(np.abs(table) if qtype == "fp4" else table))
    mids = ((srt[:-1] + srt[1:]) * F(0.5)).astype(F)
    nb = n // 64
    if nb >= 1:  # block 0: max is negative (-1 at the front), thresholds (scale 1: exact in bf16 where the mid is), +-0
        w[:64] = 0.0
        w[0] = -1.0
        k = len(mids)  # <= 15: each midpoint rounded to bf16, and the bf16 value on its other side
        w[1:1 + k] = mids
        up = R.bf16_bits_to_f32(R.f32_to_bf16_bits(mids))
        w[17:17 + k] = np.where(up > mids, up * F(1 - 2.0 ** -7), up * F(1 + 2.0 ** -7))
        w[41], w[42], w[43] = 0.0, -0.0, 0.5
    if nb >= 3:
        w[64:128] = 0.0  # an all-zero block
        w[128:192] = (rng.standard_normal(64) * 3e-6).astype(F)  # below the fp16 normal range (6.1e-5): subnormals
        w[130] = 1e-9  # under half the smallest fp16 subnormal: 0 after the cast
    if nb >= 5:
        w[192:256] = np.tile(table, 4) * F(0.25)  # every table entry, scale exact
        w[256:320] = -np.abs(w[256:320]) - F(0.01)  # every element negative
    if nb >= 7:
        # exactly on a threshold (the lower entry must win): 5 * fl(1 / 6) is the fp32 midpoint of fp4's 2/3 and 1,
        # 5 * fl(1 / 12) that of 1/3 and 1/2.  No bf16 input lands exactly on an nf4 midpoint (searched over every bf16
        # mantissa pair); block 0 holds the bf16 neighbours of each instead
        w[320:448] = 0.0
        w[320:323] = (6.0, 5.0, -5.0)
        w[384:387] = (12.0, 5.0, -5.0)
    return R.f32_to_bf16_bits(w)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for qtype in ("fp4", "nf4"):
        for i, n in enumerate(SIZES):
            bits = _weights(n, qtype, 100 + i)
            out[qtype, n] = (bits, R.quantize(bits, qtype))
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("qtype", ["fp4", "nf4"])
def test_quantize_and_dequant_equal_the_restatement(cases, qtype, n):
    from pizero_native import ops
    from pizero_native import quant4 as Q
    from pizero_native.optim import create_dynamic_map

    bits, ref = cases[qtype, n]
    dev = "cuda"
    w = tensor_of(bits, (n,), dev)
    nb = (n + 63) // 64
    packed = torch.full((n // 2 + GUARD,), 0xA5, device=dev, dtype=torch.uint8)
    absmax = torch.full((nb + GUARD,), float("nan"), device=dev, dtype=torch.float32)
    ops.q4_quantize(w, packed, absmax, qtype)
    p1, a1 = packed.clone(), absmax.clone()
    ops.q4_quantize(w, packed, absmax, qtype)
    torch.cuda.synchronize()
    assert torch.equal(p1, packed) and torch.equal(a1.view(torch.int32), absmax.view(torch.int32))
    assert (packed[n // 2:] == 0xA5).all() and torch.isnan(absmax[nb:]).all()
    pk = packed[: n // 2].cpu().numpy()
    ref_pk, ref_am = R.quantize_blocks(bits, qtype)
    assert np.array_equal(absmax[:nb].cpu().numpy().view(np.uint32), ref_am.view(np.uint32))
    bad = np.flatnonzero(pk != ref_pk)
    assert bad.size == 0, f"{bad.size} packed bytes differ, first at {bad[:5]}: {pk[bad[:5]]} vs {ref_pk[bad[:5]]}"

    # the nested step (torch) on the kernel's absmax
    qmap = create_dynamic_map(True).to(dev)
    codes, nam, offset = Q.nested_quantize(absmax[:nb], qmap)
    assert np.array_equal(qmap.cpu().numpy().view(np.uint32), ref["qmap"].view(np.uint32))
    assert np.array_equal(codes.cpu().numpy(), ref["absmax"])
    assert np.array_equal(nam.cpu().numpy().view(np.uint32), ref["nested_absmax"].view(np.uint32))
    assert F(offset) == ref["offset"]

    # dequantisation, into NaN with guard elements past n
    want = R.dequantize(ref["packed"], ref["absmax"], ref["nested_absmax"], ref["offset"], ref["qmap"], qtype, n)
    dst = torch.full((n + GUARD,), float("nan"), device=dev, dtype=torch.bfloat16)
    seg = [(packed[: n // 2], codes, nam, offset, n, dst)]
    ops.q4_dequant(seg, qmap, qtype)
    d1 = dst.clone()
    ops.q4_dequant(seg, qmap, qtype)
    torch.cuda.synchronize()
    assert torch.equal(d1.view(torch.int16), dst.view(torch.int16))
    assert torch.isnan(dst[n:].float()).all()
    got = bits_of(dst[:n])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {n} weights differ, first at {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


@pytest.mark.parametrize("qtype", ["fp4", "nf4"])
def test_multi_segment_launch_equals_single_launches(cases, qtype):
    """q|k|v / gate|up: several weights dequantised by one launch into one buffer, each equal to its own launch"""
    from pizero_native import quant4 as Q

    dev = "cuda"
    store = Q.Q4Store(qtype, dev)
    sizes = [136 * 64, 72, 4304 * 8]
    names = [f"w{i}" for i in range(3)]
    for nm, n in zip(names, sizes):
        store.quantize(nm, tensor_of(cases[qtype, n][0], (n,), dev))
    total = sum(sizes)
    dst = torch.full((total + GUARD,), float("nan"), device=dev, dtype=torch.bfloat16)
    out = store.dequant(names, dst)
    torch.cuda.synchronize()
    assert out.numel() == total and torch.isnan(dst[total:].float()).all()
    off = 0
    for nm, n in zip(names, sizes):
        ref = cases[qtype, n][1]
        want = R.dequantize(ref["packed"], ref["absmax"], ref["nested_absmax"], ref["offset"], ref["qmap"], qtype, n)
        assert np.array_equal(bits_of(dst[off:off + n]), want), nm
        off += n


def test_odd_n_and_bad_arguments_are_refused_with_the_output_untouched():
    from pizero_native import ops
    from pizero_native._lib import NativeError
    from pizero_native.optim import create_dynamic_map

    dev = "cuda"
    n = 129
    w = torch.randn(n, device=dev).to(torch.bfloat16)
    packed = torch.full((80,), 0xA5, device=dev, dtype=torch.uint8)
    absmax = torch.full((8,), float("nan"), device=dev, dtype=torch.float32)
    with pytest.raises(NativeError, match="even"):
        ops.q4_quantize(w, packed, absmax, "fp4")
    torch.cuda.synchronize()
    assert (packed == 0xA5).all() and torch.isnan(absmax).all()
    qmap = create_dynamic_map(True).to(dev)
    dst = torch.full((n + 7,), float("nan"), device=dev, dtype=torch.bfloat16)
    codes = torch.zeros(3, device=dev, dtype=torch.uint8)
    nam = torch.ones(1, device=dev, dtype=torch.float32)
    with pytest.raises(NativeError, match="even"):
        ops.q4_dequant([(packed, codes, nam, 0.0, n, dst)], qmap, "nf4")
    with pytest.raises(NativeError, match="aligned"):
        ops.q4_dequant([(packed, codes, nam, 0.0, 128, dst[1:])], qmap, "nf4")
    with pytest.raises(ValueError, match="quantize_type"):
        ops.q4_quantize(w[:128], packed, absmax, "int4")
    torch.cuda.synchronize()
    assert torch.isnan(dst.float()).all()
