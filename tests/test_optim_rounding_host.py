"""Compensated and stochastic bf16 weight updates of the fused AdamW: the parts that need no GPU.

ABI surface of pz_adamw8bit_r / pz_adamw_r and their host-side argument checks (which fail before any launch), the
properties of the two modes on the numpy restatement (tests/optim_rounding_ref.py) in the experiment that motivates
them -- weights too large for an lr = 5e-5 step to survive round-to-nearest -- and the Python / config surface.
"""

import ctypes
import os

import numpy as np
import pytest

from tests import optim_rounding_ref as R
from tests.conftest import PKG, ROOT

NEW = ("pz_adamw8bit_r", "pz_adamw_r")


def test_abi_declares_exports_and_binds_the_entry_points():
    import pizero_native
    from pizero_native._lib import ABI_VERSION, SIGNATURES, AdamW8Args
    from tests.test_abi import declared_symbols

    syms = declared_symbols()
    L = pizero_native.lib()
    for s in NEW:
        assert s in syms, f"{s} not declared in include/pz_abi.h"
        assert hasattr(L, s), f"{s} not exported"
        assert s in SIGNATURES, f"{s} has no ctypes signature"
    i64, i32, u64, f32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p
    assert SIGNATURES["pz_adamw8bit_r"] == [ctypes.POINTER(AdamW8Args), vp, i32, u64, i64, vp]
    assert SIGNATURES["pz_adamw_r"] == [vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, f32, f32, vp, i32, u64, i64,
                                        vp]
    # the existing entry points keep their signatures
    assert SIGNATURES["pz_adamw8bit"] == [ctypes.POINTER(AdamW8Args), vp]
    assert SIGNATURES["pz_adamw"] == [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, f32, f32, vp, vp]
    assert ABI_VERSION == 22 and L.pz_abi_version() == 22  # entry points added, no signature changed
    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    assert "#define PZ_ABI_VERSION 22" in hdr


def test_ops_wrappers_exist_and_share_the_constants():
    from pizero_native import ops

    assert callable(ops.adamw_r) and callable(ops.adamw8bit_r) and callable(ops._adamw8_args)
    assert (ops.ROUND_COMPENSATED, ops.ROUND_STOCHASTIC) == (1, 2)
    for z in (0, 1, 42, 2 ** 64 - 1, 0x9E3779B97F4A7C15):  # the host hash is the restatement's
        assert ops.splitmix64(z) == R.splitmix64_int(z) == int(R.splitmix64(np.uint64(z)))


def _host_buffers():
    """host memory is enough: the checks return before anything is launched or dereferenced"""
    buf = ctypes.create_string_buffer(8192 + 64)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    return base, buf


# (label, comp as an offset from the buffer base or None, mode, rng_base); p sits at base, comp's home at base + 2048
BAD = [("null comp in mode 1", None, 1, 0), ("comp off an 8-byte boundary", 2048 + 2, 1, 0),
       ("comp off by 4 bytes", 2048 + 4, 1, 0), ("comp == p", 0, 1, 0), ("comp inside p", 64, 1, 0),
       ("mode 0", 2048, 0, 0), ("mode 3", 2048, 3, 0), ("mode -1", 2048, -1, 0),
       ("negative rng_base, compensated", 2048, 1, -1), ("negative rng_base, stochastic", 2048, 2, -4)]


@pytest.mark.parametrize("fn", NEW)
def test_error_path_without_gpu(fn):
    import pizero_native
    from pizero_native._lib import AdamW8Args

    L = pizero_native.lib()
    base, keep = _host_buffers()
    p, g, other = base, base + 4096, base + 6144
    for label, coff, mode, rbase in BAD:
        comp = None if coff is None else base + coff
        if fn == "pz_adamw8bit_r":
            a = AdamW8Args()
            a.p, a.g, a.seg, a.qmap1, a.qmap2 = p, g, other, other, other
            a.s1, a.s2, a.absmax1, a.absmax2, a.m32, a.v32 = other, other, other, other, other, other
            a.nseg, a.nblocks = 1, 4  # at least 3 * 256 + 1 elements: p covers base .. base + 1538
            rc = L.pz_adamw8bit_r(ctypes.byref(a), comp, mode, 7, rbase, None)
        else:
            rc = L.pz_adamw_r(p, comp, g, other, other, 512, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, None, mode, 7,
                              rbase, None)
        assert rc == 1, f"{fn}: {label} was not refused"
        assert L.pz_last_error().startswith(fn[3:].encode()), (label, L.pz_last_error())
    del keep


# --------------------------------------------------------------------------- the restatement's properties --
STEP_FNS = [R.step_adamw_r, R.step_32bit_r]  # adamw_kernel's expression and bnb's, both with fp32 moments


@pytest.fixture(scope="module")
def stall():
    """every mode on the same 4096 weights, lr = 5e-5, 64 steps, constant gradient +1 -- computed once"""
    return {(fn.__name__, mode): R.run_stall(fn, mode) for fn in STEP_FNS
            for mode in (R.NEAREST, R.COMPENSATED, R.STOCHASTIC)}


@pytest.mark.parametrize("fn", STEP_FNS)
def test_nearest_changes_no_element(stall, fn):
    p0, p, _, master = stall[fn.__name__, R.NEAREST]
    assert p0.size == 4096 and (np.abs(p0) >= 2.0 ** -6 + 2.0 ** -12).all() and (np.abs(p0) < 2.0 ** -4).all()
    assert np.array_equal(p.view(np.uint32), p0.view(np.uint32)), int((p != p0).sum())
    moved = (p0 - master).astype(np.float64)  # while an fp32 master moves every one of them by 64 lr
    assert np.allclose(moved, 64 * 5e-5, rtol=1e-3), (moved.min(), moved.max())
    assert (moved / R.ulp_bf16(p0)).min() > 6


@pytest.mark.parametrize("fn", STEP_FNS)
def test_compensated_moves_every_element_within_the_bound(stall, fn):
    p0, p, comp, master = stall[fn.__name__, R.COMPENSATED]
    assert (p != p0).all(), int((p == p0).sum())
    err = R.err_ulps(p, master)
    print(f"{fn.__name__}: compensated max |p - master| = {err.max():.4f} ulp (bound {R.comp_bound(64):.4f})")
    assert err.max() <= R.comp_bound(64) == 0.5 + 64 * 2.0 ** -9, err.max()
    # the pair carries more than p alone: p + c is closer to the master than half an ulp
    assert R.err_ulps(p.astype(np.float64) + comp, master).max() < 0.25
    assert (np.abs(comp) <= 0.5 * R.ulp_bf16(p)).all()


@pytest.mark.parametrize("fn", STEP_FNS)
def test_stochastic_mean_drift_is_the_masters(stall, fn):
    p0, p, _, master = stall[fn.__name__, R.STOCHASTIC]
    drift = float((p.astype(np.float64) - p0).mean())
    want = float((master.astype(np.float64) - p0).mean())
    print(f"{fn.__name__}: stochastic mean drift {drift:.6e}, master {want:.6e} ({abs(drift / want - 1) * 100:.2f} %)")
    assert want < 0 and abs(drift - want) <= 0.05 * abs(want), (drift, want)
    assert (p == R.O8.bf16_round(p)).all()  # bf16 values


@pytest.mark.parametrize("fn", STEP_FNS)
def test_stochastic_is_a_function_of_seed_step_and_arena_index(stall, fn):
    _, whole, _, _ = stall[fn.__name__, R.STOCHASTIC]
    for cut in (1, 1234, 2049):  # cuts off a multiple of 4: a hash's four draws fall on both sides
        a = R.run_stall(fn, R.STOCHASTIC, sl=slice(0, cut))[1]
        b = R.run_stall(fn, R.STOCHASTIC, sl=slice(cut, None))[1]
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32)), cut
    # ... and of nothing else: another seed or another arena base gives other bits
    assert not np.array_equal(R.run_stall(fn, R.STOCHASTIC, rng_seed=1)[1], whole)
    assert not np.array_equal(R.run_stall(fn, R.STOCHASTIC, base=8)[1], whole)


def test_store_special_values():
    pv = np.array([np.inf, -np.inf, np.nan, 3.3895314e38, 1.0, -0.0], np.float32)
    p, c = R.store(pv, R.COMPENSATED)
    assert np.isinf(p[0]) and np.isinf(p[1]) and np.isnan(p[2]) and (c[:3] == 0).all() and np.isfinite(c).all()
    s, _ = R.store(pv, R.STOCHASTIC, key=5, idx=np.arange(6))
    assert s[0] == np.inf and s[1] == -np.inf and np.isnan(s[2]) and s[4] == 1.0 and s[5] == 0.0
    assert s[3] in (np.float32(3.3895314e38), np.float32(np.inf))  # the largest bf16 or, rounded up, inf


# ------------------------------------------------------------------------------------- Python / config surface --
def test_fused_adamw_refuses_an_unknown_rounding():
    import torch

    from pizero_native.optim import ROUNDINGS, FusedAdamW

    assert ROUNDINGS == ("nearest", "compensated", "stochastic")
    w = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="rounding"):
        FusedAdamW([w], rounding="bogus")
    o = FusedAdamW([w])
    assert o.rounding == "nearest" and "rounding" not in o.param_groups[0] and "seed" not in o.param_groups[0]
    for mode in ("compensated", "stochastic"):
        o = FusedAdamW([w], rounding=mode, seed=3)
        assert o.rounding == mode and o.param_groups[0]["rounding"] == mode and o.param_groups[0]["seed"] == 3


def test_bridge_config_has_the_rounding_keys():
    from src.utils.config import load_config

    c = load_config(os.path.join(PKG, "config", "train", "bridge.yaml"))
    assert c.optimizer_rounding == "nearest"
    assert c.optimizer_rounding_seed == c.seed == 42
    c2 = load_config(os.path.join(PKG, "config", "train", "bridge.yaml"), {"seed": 7})
    assert c2.optimizer_rounding_seed == 7
