"""The 4-bit base-weight format of QLoRA on the host: properties of the numpy restatement
(tests/quant4_ref.py) that pins pz_q4_quantize / pz_q4_dequant, and the state_dict layout of a packed Linear."""

import numpy as np
import pytest
import torch

from tests import quant4_ref as R

F = np.float32


def _bf16(x):
    return R.f32_to_bf16_bits(np.asarray(x, dtype=F))


@pytest.mark.parametrize("qtype", ["fp4", "nf4"])
def test_table_entries_times_absmax_come_back(qtype):
    """a block that holds every table entry times its absmax quantises to those entries: dequantisation returns
    bf16(fp16(entry * absmax')), absmax' the double-quantised scale"""
    table = R.TABLES[qtype]
    for am in (1.0, 0.03125, 3.0):  # exactly representable in bf16 / fp16
        vals = np.tile(table * F(am), 4).astype(F)  # one block of 64: each entry 4 times
        bits = _bf16(vals)
        q = R.quantize(bits, qtype)
        nib = np.stack([q["packed"] >> 4, q["packed"] & 15], 1).reshape(-1)
        assert np.array_equal(table[nib], np.tile(table, 4))  # every entry's own code (-0 quantises to +0's)
        am2 = R.nested_dequantize(q["absmax"], q["nested_absmax"], q["offset"], q["qmap"])
        want = R.f32_to_bf16_bits((table[nib] * am2[0]).astype(F).astype(np.float16).astype(F))
        got = R.roundtrip(bits, qtype)
        assert np.array_equal(got, want)
        # one block: absmax - offset = 0 exactly, so the scale itself comes back, and every entry does up to the two
        # roundings of the output (half an ulp each: fp16 2^-11, then bf16 2^-8, relative)
        assert am2[0] == F(am)
        exact = table[nib].astype(np.float64) * am
        assert (np.abs(R.bf16_bits_to_f32(got) - exact) <= (2.0 ** -11 + 2.0 ** -8) * np.abs(exact)).all()


@pytest.mark.parametrize("qtype", ["fp4", "nf4"])
def test_round_trip_error_is_within_half_the_largest_gap(qtype):
    rng = np.random.default_rng(0)
    n = 64 * 300 + 8  # crosses a nested block, ragged end
    w = (rng.standard_normal(n) * 0.05).astype(F)
    bits = _bf16(w)
    x = R.bf16_bits_to_f32(bits).astype(np.float16).astype(F)
    packed, absmax = R.quantize_blocks(bits, qtype)
    nib = np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:n]
    blk = np.arange(n) // 64
    gap = np.diff(np.sort(R.TABLES[qtype])).max()
    # against the exact block scale: nearest entry, so half the largest gap of the table, per block
    err = np.abs(R.TABLES[qtype][nib].astype(np.float64) * absmax[blk] - x)
    assert (err <= 0.5 * gap * absmax[blk] * (1 + 1e-6)).all()
    # the whole round trip adds the error of the 8-bit scale (relative to the nested block's absmax) and two
    # roundings (fp16 2^-11, bf16 2^-8, relative) of a value of at most absmax
    got = R.bf16_bits_to_f32(R.roundtrip(bits, qtype))
    codes, nam, offset, qmap = R.nested_quantize(absmax)
    am2 = R.nested_dequantize(codes, nam, offset, qmap)
    bound = 0.5 * gap * absmax[blk] + np.abs(am2 - absmax)[blk] + (2.0 ** -11 + 2.0 ** -8) * am2[blk]
    assert (np.abs(got.astype(np.float64) - x) <= bound * (1 + 1e-6)).all()


def test_packing_order_thresholds_and_signs():
    # nf4: element 0 = +1 (code 15), element 1 = -1 (code 0): the even element sits in the high nibble
    bits = _bf16(np.array([1.0, -1.0] + [0.0] * 62, dtype=F))
    packed, absmax = R.quantize_blocks(bits, "nf4")
    assert packed[0] == 0xF0 and absmax[0] == 1.0 and (packed[1:] == 0x77).all()  # 0.0 is code 7
    # fp4: +1 is code 3, -1 is code 3 | 8, +0 and -0 are code 0 (the sign bit is x < 0)
    bits = _bf16(np.array([1.0, -1.0, 0.0, -0.0] + [0.0] * 60, dtype=F))
    packed, _ = R.quantize_blocks(bits, "fp4")
    assert packed[0] == 0x3B and packed[1] == 0x00
    # a value exactly on a threshold takes the lower entry (x > mid picks the upper one)
    mid = (R.NF4[14] + R.NF4[15]) * F(0.5)
    assert R.codes_of(np.array([mid, np.nextafter(mid, F(2))], dtype=F), "nf4").tolist() == [14, 15]
    mid = (F(0.5) + F(0.66666667)) * F(0.5)
    assert R.codes_of(np.array([mid, -mid, np.nextafter(mid, F(2))], dtype=F), "fp4").tolist() == [5, 13, 2]
    with pytest.raises(ValueError):
        R.quantize_blocks(bits[:63], "fp4")
    with pytest.raises(ValueError, match="quantize_type"):
        R.codes_of(np.zeros(2, F), "int4")


@pytest.mark.parametrize("qtype", ["fp4", "nf4"])
def test_state_dict_keys_and_blob_round_trip(qtype):
    from pizero_native import quant4 as Q

    assert Q.state_keys(qtype) == R.state_keys(qtype)
    assert np.array_equal(Q.table(qtype).numpy(), R.TABLES[qtype])
    blob = Q.quant_state_blob(qtype, (24, 16), np.float32(0.0123))
    assert blob.dtype == torch.uint8 and np.array_equal(blob.numpy(), R.quant_state_blob(qtype, (24, 16), F(0.0123)))
    st = Q.parse_quant_state(blob)
    assert st == R.parse_blob(blob.numpy())
    assert st["quant_type"] == qtype and st["shape"] == [24, 16] and st["blocksize"] == 64
    assert st["dtype"] == "bfloat16" and st["nested_blocksize"] == 256
    assert np.float32(st["nested_offset"]) == np.float32(0.0123)  # the fp32 offset survives the JSON text
    with pytest.raises(ValueError, match="quantize_type"):
        Q.state_keys("int4")
    # the nested step of the package (torch) equals the restatement's, bit for bit
    rng = np.random.default_rng(1)
    absmax = np.abs(rng.standard_normal(300)).astype(F) * F(0.1)
    absmax[5] = 0
    codes, nam, offset, qmap = R.nested_quantize(absmax)
    from pizero_native.optim import create_dynamic_map

    c2, n2, o2 = Q.nested_quantize(torch.from_numpy(absmax), create_dynamic_map(True))
    assert np.array_equal(create_dynamic_map(True).numpy(), qmap)
    assert np.array_equal(c2.numpy(), codes) and np.array_equal(n2.numpy(), nam) and F(o2) == offset


def test_config_surface_on_the_host():
    """quantize: True constructs (bf16 weights in the arena's side buffer, no gradient slot); an unknown quantize_type,
    lora_dropout > 0 and a partly quantised VLM are refused by name"""
    from src.model.vla.pizero import PiZero
    from tests.golden.make_golden_lora import lora_cfg
    from tests.oracle_helpers import O
    from tests.qlora_helpers import qlora_cfg

    d = O.TINY_DIMS
    m = PiZero(qlora_cfg(d), init="none")
    plain = PiZero(lora_cfg(d), init="none")
    q = m._q4_names()
    assert q and all(m._arena.slots[n].side for n in q)
    assert set(q) == {n[: -len("lora_A")] + "weight" for n in plain._arena.slots if n.endswith(".lora_A")}
    packed = sum(-(-plain._arena.slots[n].numel // 8) * 8 for n in q)
    assert plain._arena.total - packed - 64 < m._arena.total <= plain._arena.total - packed + 64  # 64-element rounding
    assert m._arena.side_total >= packed and plain._arena.side is None
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys())  # bf16 until quantize_base_()
    with pytest.raises(ValueError, match="quantize_type"):
        PiZero(qlora_cfg(d, qtype="int4"), init="none")
    cfg = qlora_cfg(d)
    cfg.joint.config.lora.dropout = 0.05
    with pytest.raises(NotImplementedError, match="lora_dropout"):
        PiZero(cfg, init="none")
    cfg = qlora_cfg(d)
    cfg.vision_projector.use_quantize = False
    with pytest.raises(NotImplementedError, match="use_quantize"):
        PiZero(cfg, init="none")
