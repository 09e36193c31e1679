"""Inference-time guidance on the host: the restatement tests/rtc_ref.py against the oracle, the two host
tables and next_guidance of src/agent/chunking.py, and the new entry points' declarations."""

import os

import numpy as np
import pytest
import torch

from tests import rtc_ref as R
from tests.conftest import ROOT
from tests.oracle_helpers import O

D = O.TINY_DIMS
B = 3


def _chunking():
    from src.agent import chunking

    return chunking


@pytest.fixture(scope="module")
def fx():
    return R.fixture(D, B, ragged=True)


def test_zero_weight_is_the_oracle_bit_for_bit(fx):
    """W = 0: e = 0, the VJP of 0 is 0, and every step is a + dt * v in the oracle's order"""
    W, inp, args = fx
    H, A = D["horizon_steps"], D["action_dim"]
    target = torch.from_numpy(inp["actions"])
    coef = _chunking().guidance_coef(D["num_inference_steps"], 5.0)
    got = R.guided_infer(W, D, *args, target, torch.zeros(B, H), coef, clip=False)
    with torch.no_grad():
        want = O.pizero_infer(W, D, *args, clip=False)
    assert got.shape == (B, H, A)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_guidance_pulls_the_chunk_and_needs_the_jacobian(fx):
    """delay 1, overlap 4, beta 5: the W = 1 rows land on the target; without the Jacobian term the chunk is another"""
    W, inp, args = fx
    c = _chunking()
    H = D["horizon_steps"]
    target = torch.from_numpy(inp["actions"])
    w = torch.from_numpy(c.soft_mask(H, 1, 4))[None].repeat(B, 1)
    coef = c.guidance_coef(D["num_inference_steps"], 5.0)
    full = R.guided_infer(W, D, *args, target, w, coef, clip=False)
    nojac = R.guided_infer(W, D, *args, target, w, coef, clip=False, jacobian=False)
    with torch.no_grad():
        plain = O.pizero_infer(W, D, *args, clip=False)
    near = (full[:, :1] - target[:, :1]).abs().mean().item()
    far = (plain[:, :1] - target[:, :1]).abs().mean().item()
    print(f"mean |a - Y| on the W = 1 rows: guided {near:.4f}, unguided {far:.4f}; "
          f"max |full - no Jacobian| {(full - nojac).abs().max().item():.4f}")
    assert near < 0.25 * far
    assert (full - nojac).abs().max().item() > 0.09  # 3 x the 3e-2 parity floor of the GPU test


def test_vjp_against_central_differences(fx):
    """dA = (dv/dA)^T e of one step against fp64 central differences of <e, v(A)> on a handful of coordinates.
    Step 1e-2: the truncation error is O(h^2) ~ 1e-4 of the derivative's scale, and the fp32 rounding inside the
    oracle's RMSNorm (1e-7 of <e, v>) divided by 2h stays below 1e-5; a wrong VJP is off by its own size."""
    W, inp, args = fx
    ids, pix, itp, amask, vpos, ppos, apos, prop, noise = args
    with torch.no_grad():
        emb = O.embed_siglip_and_text(W, D, ids, pix)
        pe = O.linear(prop, W, "proprio_encoder")
        _, cache = O.joint_forward(W, D, {"vlm": emb, "proprio": pe}, {"vlm": vpos, "proprio": ppos}, itp,
                                   return_cache=True)
    H = D["horizon_steps"]
    t = torch.full((B,), 0.3)
    target = torch.from_numpy(inp["actions"])
    w = torch.from_numpy(_chunking().soft_mask(H, 1, 4))[None].repeat(B, 1)
    _, v, e, dA = R.guided_step(W, D, noise, t, cache, apos, amask, target, w, 2.0, 0.1)
    W64 = {k: x.double() for k, x in W.items()}
    c64 = {n: [(k.double(), x.double()) for k, x in kv] for n, kv in cache.items()}
    h = 1e-2
    scale = dA.abs().max().item()
    worst = 0.0
    for (b, r, c) in [(0, 0, 0), (0, 3, 6), (1, 1, 2), (1, 2, 5), (2, 0, 4), (2, 3, 1)]:
        f = []
        for s in (h, -h):
            a = noise.double().clone()
            a[b, r, c] += s
            with torch.no_grad():
                f.append((R.denoiser(W64, D, a, t.double(), c64, apos, amask.double()) * e.double()).sum().item())
        fd = (f[0] - f[1]) / (2 * h)
        worst = max(worst, abs(fd - dA[b, r, c].item()))
    print(f"max |dA - central difference| {worst:.3e}, max |dA| {scale:.3e}")
    assert scale > 1e-3 and worst <= 1e-2 * scale


def test_soft_mask():
    c = _chunking()
    np.testing.assert_allclose(c.soft_mask(4, 1, 4), [1.0, 0.488, 0.189, 0.041], atol=5e-4)
    for (H, dl, ov) in [(4, 1, 4), (4, 1, 3), (4, 2, 4), (4, 0, 4), (50, 7, 30), (4, 4, 4), (4, 0, 0)]:
        w = c.soft_mask(H, dl, ov)
        assert w.dtype == np.float32 and w.shape == (H,)
        assert np.array_equal(w, R.soft_mask_ref(H, dl, ov).astype(np.float32))
        assert (w[:dl] == 1).all() and (w[ov:] == 0).all() and (np.diff(w) <= 0).all()
        assert ((w[dl:ov] > 0) & (w[dl:ov] < 1)).all()
    for bad in [(4, 3, 2), (4, 0, 5), (4, -1, 2)]:
        with pytest.raises(ValueError, match="soft_mask"):
            c.soft_mask(*bad)


def test_guidance_coef():
    c = _chunking()
    for steps, beta in [(10, 5.0), (10, 1.5), (7, 5.0), (1, 3.0)]:
        k = c.guidance_coef(steps, beta)
        assert k.dtype == np.float32 and k.shape == (steps,) and k[0] == np.float32(beta)
        assert np.array_equal(k, R.guidance_coef_ref(steps, beta).astype(np.float32))
        half = [i for i in range(steps) if i / steps <= 0.5]
        assert (np.diff(k[half]) <= 0).all()  # non-increasing up to t = 0.5
        assert (k <= np.float32(beta)).all() and (k >= min(beta, 2.0) - 1e-6).all()  # the ratio's minimum is 2, at 0.5
    np.testing.assert_allclose(c.guidance_coef(10, 5.0)[[2, 5]], [4.25, 2.0], rtol=1e-6)
    with pytest.raises(ValueError, match="guidance_coef"):
        c.guidance_coef(0, 5.0)


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_next_guidance(kind):
    c = _chunking()
    H, A = 4, 7
    prev = np.arange(H * A, dtype=np.float32).reshape(H, A)
    if kind == "torch":
        prev = torch.from_numpy(prev)
    eq = (lambda a, b: np.array_equal(a, b)) if kind == "numpy" else torch.equal
    # offset 0: the whole previous chunk is the target
    tgt, dl, ov = c.next_guidance(prev, 0, 1)
    assert (dl, ov) == (1, H) and eq(tgt, prev) and type(tgt) is type(prev)
    # offset H - 1: one row left, repeated; a longer delay is cut to it
    tgt, dl, ov = c.next_guidance(prev, H - 1, 2)
    assert (dl, ov) == (1, 1) and all(eq(tgt[i], prev[H - 1]) for i in range(H))
    # delay = overlap: hard weights only
    tgt, dl, ov = c.next_guidance(prev, 2, 2)
    assert (dl, ov) == (2, 2) and eq(tgt[:2], prev[2:]) and eq(tgt[2], prev[3]) and eq(tgt[3], prev[3])
    assert np.array_equal(c.soft_mask(H, dl, ov), np.asarray([1, 1, 0, 0], dtype=np.float32))
    tgt[0] = 0  # a copy, not a view
    assert float(prev[2][0]) == 2 * A
    for bad in [(H, 1), (-1, 1), (0, -1)]:
        with pytest.raises(ValueError, match="next_guidance"):
            c.next_guidance(prev, *bad)


def test_kernel_restatements_follow_their_formulas():
    """the numpy statements of pz_rtc_seed / pz_rtc_euler against float64 (they differ by float32 rounding only)"""
    rng = np.random.default_rng(0)
    Bn, H, A = 3, 4, 7
    a, tg, dA = (rng.standard_normal((Bn, H, A)).astype(np.float32) for _ in range(3))
    v = R.bf16_round(rng.standard_normal((Bn, H, A)).astype(np.float32))
    w = rng.random((Bn, H)).astype(np.float32)
    t = rng.random(Bn).astype(np.float32)
    e, eb = R.seed_np(a, v, tg, w, t)
    e64 = w[:, :, None].astype(np.float64) * (tg - (a + (1.0 - t.astype(np.float64))[:, None, None] * v))
    np.testing.assert_allclose(e, e64, rtol=0, atol=1e-6)
    assert np.abs(eb - e).max() <= 2.0 ** -8 * np.abs(e).max() and np.array_equal(R.bf16_round(eb), eb)
    a2, t2 = R.euler_np(a, v, e, R.bf16_round(dA), t, 4.25, 0.1)
    g64 = e64 + (1.0 - t.astype(np.float64))[:, None, None] * R.bf16_round(dA)
    np.testing.assert_allclose(a2, a + 0.1 * (v + 4.25 * g64), rtol=0, atol=2e-6)
    np.testing.assert_allclose(t2, t + 0.1, rtol=0, atol=1e-7)


def test_abi_declares_the_entry_points():
    import pizero_native
    from pizero_native import ops
    from pizero_native._lib import SIGNATURES

    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    L = pizero_native.lib()
    for name in ("pz_dgrad_rows", "pz_dgrad_rows_ws_bytes", "pz_rtc_seed", "pz_rtc_euler"):
        assert name in SIGNATURES and f" {name}(" in hdr and hasattr(L, name), name
    for f in ("linear_dgrad_rows", "rtc_seed", "rtc_euler"):
        assert callable(getattr(ops, f))
    # host logic, no device: the workspace of a supported shape holds at least one [M, K] fp32 slab, 0 = unsupported
    assert L.pz_dgrad_rows_ws_bytes(5, 1024, 4096) >= 5 * 4096 * 4
    assert L.pz_dgrad_rows_ws_bytes(17, 1024, 4096) == 0 and L.pz_dgrad_rows_ws_bytes(5, 12, 4096) == 0


def test_refusals_name_their_key():
    """the guided loop's refusals, on an engine that is never given a device (Engine._guide_args is host logic)"""
    import types

    from pizero_native import engine as E
    from src.model.vla.pizero import PiZero
    from tests.golden.make_golden import ref_cfg
    from tests.golden.make_golden_adaln import adaptive_cfg

    for msg, keys in ((E.GUIDE_ADAPTIVE_MSG, ("action_expert_adaptive_mode", "action_guidance_beta")),
                      (E.GUIDE_FP8_MSG, ("fp8", "action_guidance_beta")), (E.GUIDE_MASK_MSG, ("GeneralMask",)),
                      (E.GUIDE_PREFIX_MSG, ("prefix_len", "overlap"))):
        assert all(k in msg for k in keys), msg
    guide = (torch.zeros(3, 4, 7), torch.zeros(3, 4), torch.zeros(10))
    ada = E.Engine(PiZero(adaptive_cfg(D, "adaLN"), init="none"))
    with pytest.raises(NotImplementedError, match="action_expert_adaptive_mode"):
        ada._guide_args(guide, 3, None, None)
    eng = E.Engine(PiZero(ref_cfg(D), init="none"))
    with pytest.raises(NotImplementedError, match="GeneralMask"):
        eng._guide_args(guide, 3, E.GeneralMask(), None)
    with pytest.raises(NotImplementedError, match="prefix_len"):
        eng._guide_args(guide, 3, None, torch.zeros(3, dtype=torch.int32))
    eng.f8 = {}
    with pytest.raises(NotImplementedError, match="fp8"):
        eng._guide_args(guide, 3, None, None)
    eng.f8 = None
    with pytest.raises(ValueError, match="fp32 device tensor"):  # host tensors are not the device inputs
        eng._guide_args(guide, 3, None, None)
    m = types.SimpleNamespace()
    with pytest.raises(NotImplementedError, match="action_guidance_beta"):
        PiZero.infer_action_naive.__wrapped__(m, *([None] * 7), guide=guide)
    # the dgrad-only switch answers for requires_grad without touching it
    name = "action_decoder.weight"
    before = eng.m._requires_grad(name)
    eng._dgrad_only = True
    assert eng.rg(name) is False and eng.m._requires_grad(name) == before
    eng._dgrad_only = False
    assert eng.rg(name) == before
