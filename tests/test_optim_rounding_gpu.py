"""Compensated and stochastic bf16 weight updates (pz_adamw8bit_r, pz_adamw_r; FusedAdamW(rounding=...)) on the GPU.

Both kernels are held BIT-EXACT to the numpy restatement (tests/optim_rounding_ref.py) on the tensors of
tests/test_adamw8bit_gpu.py: >= 4096 elements (8-bit codes, one absmax per 256, a partial last block and a partial
last lane) and < 4096 (fp32 state, a 7-element tensor) in one 8-aligned arena run.  Then the properties: the default
is untouched, the stall round-to-nearest causes is gone, the stochastic draws do not depend on how parameters are
split over optimizers, and a checkpoint round trip continues bit for bit.
"""

import io

import numpy as np
import pytest
import torch

from tests import optim_rounding_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(64, 96), (5003,), (1152,), (4304,), (7,), (256, 260)]
MODES = {"compensated": R.COMPENSATED, "stochastic": R.STOCHASTIC}
LR, WD = 2e-3, 0.01


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _offsets():
    offs, o = [], 0
    for s in SIZES:
        offs.append(o)
        o += (int(np.prod(s)) + 7) // 8 * 8
    return offs, o


def _arena(seed):
    offs, total = _offsets()
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(total, generator=g) * 2 - 1).to("cuda", torch.bfloat16)
    return [torch.nn.Parameter(w[off:off + int(np.prod(s))].view(s)) for s, off in zip(SIZES, offs)], w


@pytest.fixture(scope="module")
def grads():
    """five flat bf16 gradients over the arena, shared by every test"""
    _, total = _offsets()
    gen = torch.Generator().manual_seed(1)
    return [((torch.rand(total, generator=gen) * 2 - 1) * 0.5).to("cuda", torch.bfloat16) for _ in range(5)]


def _set_grads(ps, w, gflat):
    for p in ps:
        o = (p.data_ptr() - w.data_ptr()) // 2
        p.grad = gflat[o:o + p.numel()].view(p.shape)


def _steps(opts, ps, w, gs, clip=True):
    from pizero_native.optim import clip_grad_norm_

    scales = []
    for g in gs:
        _set_grads(ps, w, g)
        if clip:
            clip_grad_norm_(opts, 1.0)
            scales.append(float(opts[0]._gscale.item()))
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    return scales


def bits(t):
    return t.detach().contiguous().view(torch.int16)


def _param_bits(ps):
    """the parameters' bits without the arena padding between them (which only the flat fp32-state kernels touch)"""
    return torch.cat([bits(p).reshape(-1) for p in ps])


def _np(t):
    return t.detach().float().cpu().numpy().reshape(-1)


def _same_state(sa, sb):
    assert sa["param_groups"] == sb["param_groups"]
    assert list(sa["state"]) == list(sb["state"])
    for i in sa["state"]:
        assert list(sa["state"][i]) == list(sb["state"][i]), i
        for k, x in sa["state"][i].items():
            y = sb["state"][i][k]
            if isinstance(x, torch.Tensor):
                x, y = x.cpu(), y.cpu()
                assert x.dtype == y.dtype and x.shape == y.shape, (i, k)
                assert torch.equal(bits(x), bits(y)) if x.dtype == torch.bfloat16 else torch.equal(x, y), (i, k)
            else:
                assert x == y, (i, k)


# --------------------------------------------------------------------------------- 1. bit-exact vs restatement --
@pytest.mark.parametrize("state_bits", [8, 32])
@pytest.mark.parametrize("mode", list(MODES))
def test_bit_exact_vs_restatement(mode, state_bits, grads):
    from pizero_native.optim import FusedAdamW

    O8, md, seed = R.O8, MODES[mode], 11
    ps, w = _arena(0)
    offs, _ = _offsets()
    opt = FusedAdamW(ps, lr=LR, weight_decay=WD, state_bits=state_bits, rounding=mode, seed=seed)
    ref = []
    for p in ps:
        n, nb = p.numel(), (p.numel() + 255) // 256
        ref.append(dict(p=_np(p), comp=np.zeros(n, np.float32), c1=np.zeros(n, np.uint8), c2=np.zeros(n, np.uint8),
                        a1=np.zeros(nb, np.float32), a2=np.zeros(nb, np.float32), m=np.zeros(n, np.float32),
                        v=np.zeros(n, np.float32)))
    q1, q2 = O8.create_dynamic_map(True), O8.create_dynamic_map(False)
    for t in range(1, 4):
        (gs,) = _steps([opt], ps, w, grads[t - 1:t])
        key = R.step_key(seed, t)
        for r, p, off in zip(ref, ps, offs):
            gg, idx = _np(p.grad), off + np.arange(p.numel(), dtype=np.int64)
            hyper = (LR, 0.9, 0.999, 1e-8, WD, t, gs, md, key, idx)
            if state_bits == 32:
                pn, cn, r["m"], r["v"] = R.step_adamw_r(r["p"], r["comp"], gg, r["m"], r["v"], *hyper)
            elif p.numel() >= O8.MIN_8BIT_SIZE:
                pn, cn, r["c1"], r["c2"], r["a1"], r["a2"] = R.step_8bit_r(
                    r["p"], r["comp"], gg, r["c1"], r["c2"], r["a1"], r["a2"], q1, q2, *hyper)
            else:
                pn, cn, r["m"], r["v"] = R.step_32bit_r(r["p"], r["comp"], gg, r["m"], r["v"], *hyper)
            r["p"] = pn
            r["comp"] = cn if cn is not None else r["comp"]
    sd = opt.state_dict()
    any_comp = False
    for i, (p, r) in enumerate(zip(ps, ref)):
        np.testing.assert_array_equal(_np(p).view(np.uint32), r["p"].view(np.uint32), err_msg=f"param {i}")
        st = sd["state"][i]
        if mode == "compensated":
            assert st["comp"].dtype == torch.bfloat16 and st["comp"].shape == p.shape
            np.testing.assert_array_equal(_np(st["comp"]).view(np.uint32), r["comp"].view(np.uint32),
                                          err_msg=f"comp {i}")
            any_comp |= bool(r["comp"].any())
        else:
            assert "comp" not in st
        if state_bits == 32:
            np.testing.assert_array_equal(_np(st["exp_avg"]), r["m"], err_msg=f"m {i}")
            np.testing.assert_array_equal(_np(st["exp_avg_sq"]), r["v"], err_msg=f"v {i}")
        elif p.numel() >= O8.MIN_8BIT_SIZE:
            np.testing.assert_array_equal(st["state1"].cpu().numpy().reshape(-1), r["c1"], err_msg=f"codes1 {i}")
            np.testing.assert_array_equal(st["state2"].cpu().numpy().reshape(-1), r["c2"], err_msg=f"codes2 {i}")
            np.testing.assert_array_equal(st["absmax1"].cpu().numpy(), r["a1"], err_msg=f"absmax1 {i}")
            np.testing.assert_array_equal(st["absmax2"].cpu().numpy(), r["a2"], err_msg=f"absmax2 {i}")
        else:
            np.testing.assert_array_equal(_np(st["state1"]), r["m"], err_msg=f"m {i}")
            np.testing.assert_array_equal(_np(st["state2"]), r["v"], err_msg=f"v {i}")
    assert any_comp == (mode == "compensated")
    g0 = sd["param_groups"][0]
    assert g0["step"] == 3 and g0["rounding"] == mode and g0["seed"] == seed
    if state_bits == 8:  # the segment kernel never writes the arena's padding between the tensors (the fp32-state
        pad = torch.ones(w.numel(), dtype=torch.bool)  # kernels, pz_adamw too, update the run as one flat vector)
        for p, off in zip(ps, offs):
            pad[off:off + p.numel()] = False
        w0 = _arena(0)[1]
        assert torch.equal(bits(w.cpu()[pad]), bits(w0.cpu()[pad]))


# ------------------------------------------------------------------------------------ 2. the default is untouched --
@pytest.mark.parametrize("state_bits", [8, 32])
def test_nearest_is_the_optimizer_of_before(state_bits, grads):
    from pizero_native.optim import FusedAdamW

    pa, wa = _arena(2)
    pb, wb = _arena(2)
    a = FusedAdamW(pa, lr=LR, weight_decay=WD, state_bits=state_bits)
    b = FusedAdamW(pb, lr=LR, weight_decay=WD, state_bits=state_bits, rounding="nearest", seed=5)
    _steps([a], pa, wa, grads[:3])
    _steps([b], pb, wb, grads[:3])
    assert torch.equal(bits(wa), bits(wb))
    sa, sb = a.state_dict(), b.state_dict()
    _same_state(sa, sb)
    assert sorted(sb["param_groups"][0]) == ["betas", "eps", "lr", "params", "step", "weight_decay"]
    want = {"step", "exp_avg", "exp_avg_sq"} if state_bits == 32 else None
    for i, st in sb["state"].items():
        assert "comp" not in st
        if want:
            assert set(st) == want
        else:
            big = pb[i].numel() >= 4096
            assert set(st) == ({"step", "state1", "state2"} | ({"absmax1", "absmax2", "qmap1", "qmap2"} if big
                                                                 else set()))
    assert a.state_bytes() == b.state_bytes()
    c = FusedAdamW(_arena(2)[0], lr=LR, state_bits=state_bits, rounding="compensated")
    assert c.state_bytes() == a.state_bytes() + 2 * wa.numel()  # one bf16 word per element of the run


# ------------------------------------------------------------------------------------------------ 3. the stall --
def test_stall_is_gone_on_the_device():
    """4096 weights of magnitude [2^-6 + 2^-12, 2^-4), lr 5e-5, 64 steps of gradient +1, 8-bit state: nearest moves
    nothing, compensated follows an fp32 master (CPU) within 0.5 + 64 * 2^-9 ulp"""
    from pizero_native.optim import FusedAdamW

    p0 = R.stall_weights()
    g = torch.ones(R.STALL_N, device="cuda", dtype=torch.bfloat16)
    out = {}
    for mode in ("nearest", "compensated"):
        p = torch.nn.Parameter(torch.from_numpy(p0).to("cuda", torch.bfloat16))
        assert np.array_equal(_np(p), p0)
        opt = FusedAdamW([p], lr=R.STALL_LR, state_bits=8, rounding=mode)
        p.grad = g
        for _ in range(R.STALL_STEPS):
            opt.step()
        torch.cuda.synchronize()
        out[mode] = _np(p)
    master, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t in range(1, R.STALL_STEPS + 1):
        master, m, v = R.master_step(R.step_32bit_r, master, np.ones_like(p0), m, v, R.STALL_LR, t)
    assert np.allclose(p0.astype(np.float64) - master, 64 * 5e-5, rtol=1e-3)
    assert np.array_equal(out["nearest"].view(np.uint32), p0.view(np.uint32)), int((out["nearest"] != p0).sum())
    assert (out["compensated"] != p0).all(), int((out["compensated"] == p0).sum())
    err = R.err_ulps(out["compensated"], master)
    print(f"compensated on the device: max |p - master| = {err.max():.4f} ulp (bound {R.comp_bound(64):.4f})")
    assert err.max() <= R.comp_bound(R.STALL_STEPS) == 0.5 + 64 * 2.0 ** -9, err.max()


# ------------------------------------------------------------------------------- 4. stochastic partitioning --
@pytest.mark.parametrize("state_bits", [8, 32])
def test_stochastic_does_not_depend_on_the_partition(state_bits, grads):
    from pizero_native.optim import FusedAdamW

    # no clipping here: the joint norm is summed run by run, so its last bit depends on the partition by itself
    kw = dict(lr=LR, weight_decay=WD, state_bits=state_bits, rounding="stochastic")
    pa, wa = _arena(3)
    _steps([FusedAdamW(pa, seed=9, **kw)], pa, wa, grads[:3], clip=False)
    pb, wb = _arena(3)
    _steps([FusedAdamW(pb[:2] + pb[4:5], seed=9, **kw), FusedAdamW(pb[2:4] + pb[5:], seed=9, **kw)], pb, wb, grads[:3], clip=False)
    assert torch.equal(_param_bits(pa), _param_bits(pb))
    pc, wc = _arena(3)
    _steps([FusedAdamW(pc, seed=10, **kw)], pc, wc, grads[:3], clip=False)
    assert not torch.equal(_param_bits(pa), _param_bits(pc))
    pd, wd_ = _arena(3)  # and against nearest: within one bf16 ulp of it, not equal to it
    _steps([FusedAdamW(pd, lr=LR, weight_decay=WD, state_bits=state_bits)], pd, wd_, grads[:1], clip=False)
    pe, we = _arena(3)
    _steps([FusedAdamW(pe, seed=9, **kw)], pe, we, grads[:1], clip=False)
    d = (_param_bits(pe).int() - _param_bits(pd).int()).abs()
    # floor or ceiling of pv where nearest takes the closer one: at most one ulp apart, and neither never nor always
    assert 0 < int(d.max()) <= 1 and 0.05 < float((d == 1).float().mean()) < 0.95


# ------------------------------------------------------------------------------------- 5. checkpoint round trip --
def _through_file(sd):
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    return torch.load(f, weights_only=True, map_location="cpu")


@pytest.mark.parametrize("state_bits", [8, 32])
@pytest.mark.parametrize("mode", ["nearest", "compensated", "stochastic"])
def test_checkpoint_round_trip_continues_bitwise(mode, state_bits, grads):
    from pizero_native.optim import FusedAdamW

    kw = dict(lr=LR, weight_decay=WD, state_bits=state_bits, rounding=mode, seed=4)
    pa, wa = _arena(6)
    a = FusedAdamW(pa, **kw)
    _steps([a], pa, wa, grads[:2])
    ck = _through_file(a.state_dict())
    pb, wb = _arena(6)
    wb.copy_(wa)
    b = FusedAdamW(pb, **kw)
    b.load_state_dict(ck)
    _same_state(a.state_dict(), b.state_dict())
    _steps([a], pa, wa, grads[2:4])
    _steps([b], pb, wb, grads[2:4])
    # (the parameters: the padding between them has no entry in a state dict, and the flat fp32-state kernels move it)
    assert torch.equal(_param_bits(pa), _param_bits(pb))
    _same_state(a.state_dict(), b.state_dict())
    assert b.param_groups[0]["step"] == 4
    if mode == "compensated":
        assert all("comp" in st for st in ck["state"].values())
        # ... and into another mode the compensation words are dropped
        n = FusedAdamW(_arena(6)[0], lr=LR, weight_decay=WD, state_bits=state_bits)
        n.load_state_dict(ck)
        sd = n.state_dict()
        assert n.rounding == "nearest" and all("comp" not in st for st in sd["state"].values())
        assert "rounding" not in sd["param_groups"][0] and "seed" not in sd["param_groups"][0]


@pytest.mark.parametrize("state_bits", [8, 32])
def test_nearest_state_into_compensated_starts_comp_at_zero(state_bits, grads):
    from pizero_native.optim import FusedAdamW

    pa, wa = _arena(7)
    a = FusedAdamW(pa, lr=LR, state_bits=state_bits)
    _steps([a], pa, wa, grads[:2])
    ck = _through_file(a.state_dict())
    pb, wb = _arena(7)
    wb.copy_(wa)
    b = FusedAdamW(pb, lr=LR, state_bits=state_bits, rounding="compensated")
    _steps([b], pb, wb, grads[:1])  # leaves comp non-zero
    assert any(bool(st["comp"].any()) for st in b.state_dict()["state"].values())
    wb.copy_(wa)
    b.load_state_dict(ck)
    sd = b.state_dict()
    assert all(st["comp"].dtype == torch.bfloat16 and not bool(st["comp"].any()) for st in sd["state"].values())
    assert sd["param_groups"][0]["rounding"] == "compensated" and sd["param_groups"][0]["step"] == 2
    _steps([b], pb, wb, grads[2:3])
    assert any(bool(st["comp"].any()) for st in b.state_dict()["state"].values())
