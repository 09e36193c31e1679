"""pz_adaln.hip (adaLN / adaLN-Zero row passes) against an fp64 torch evaluation of the same bf16 inputs."""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
EPS = 1e-6
SENT = 1234.0  # sentinel of the padded outputs: rows beyond R and columns beyond D stay untouched


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pizero_native

    pizero_native.lib()


def bf(*shape, scale=1.0, g=None):
    return (torch.randn(*shape, device=dev, generator=g) * scale).to(torch.bfloat16)


def close(out, ref, rtol=1.6e-2, atol=1e-2):
    """tests/test_kernels_gpu.py's bf16 gate (RMSNorm forward: defaults; backward dx: atol 2e-2)"""
    out, ref = out.float(), ref.float()
    err = (out - ref).abs()
    bad = (err > atol + rtol * ref.abs()).sum().item()
    assert bad == 0, f"{bad} mismatches, max err {err.max().item():.4g}, max ref {ref.abs().max().item():.4g}"


def rel_l2(out, ref):
    return float((out.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def padded(R, D, g=None, fill=None):
    """bf16 [R, D] view of a [R + 2, D + 24] buffer (leading dimension larger than D)"""
    full = torch.full((R + 2, D + 24), SENT, device=dev, dtype=torch.bfloat16)
    if fill is not None:
        full[:R, :D] = bf(R, D, scale=fill, g=g)
    return full, full[:R, :D]


def untouched(full, R, D):
    assert bool((full[R:] == SENT).all()) and bool((full[:, D:] == SENT).all())


class Case:
    """inputs of one (D, rows_per_sample, B): a distinct modulation row per sample in three slots
    (gate | gamma | beta) of an fp32 [B, 3 D + 12] buffer, rows with leading dimension D + 24"""

    def __init__(self, D, rps, B):
        g = torch.Generator(device=dev).manual_seed(D * 1000 + rps * 10 + B)
        self.D, self.rps, self.B, self.R = D, rps, B, B * rps
        R = self.R
        self.ldmod = 3 * D + 12
        self.mod = torch.randn(B, self.ldmod, device=dev, generator=g) * 1.5
        self.dmod = torch.full((B, self.ldmod), SENT, device=dev)
        self.bz, self.bg = bf(D, scale=0.5, g=g), bf(D, scale=0.5, g=g)
        _, self.x = padded(R, D, g, 2.0)
        _, self.y = padded(R, D, g, 1.0)
        _, self.dh = padded(R, D, g, 1.0)
        _, self.dres = padded(R, D, g, 1.0)
        f64 = lambda t: t.double()  # noqa: E731
        rep = lambda m: m.double().repeat_interleave(rps, 0)  # noqa: E731  (row -> its sample's modulation row)
        self.sz = torch.sigmoid(rep(self.mod[:, :D]) + f64(self.bz))
        self.sg = torch.sigmoid(rep(self.mod[:, D:2 * D]) + f64(self.bg))
        self.beta = rep(self.mod[:, 2 * D:3 * D])
        self.gate = (0, self.bz)
        self.gamma = (D, self.bg)
        self.beta_col = 2 * D

    def norm_ref(self, xm):
        r = torch.rsqrt(xm.pow(2).mean(-1, keepdim=True) + EPS)
        return xm * r * self.sg + self.beta, r[:, 0]

    def per_sample(self, t):
        return t.view(self.B, self.rps, self.D).sum(1)


CASES = [(D, rps, B) for D in (64, 1024, 2048) for rps in (1, 5, 51) for B in (1, 3)]


@pytest.mark.parametrize("D,rps,B", CASES)
def test_forward_stage_combinations(D, rps, B):
    from pizero_native import ops

    c = Case(D, rps, B)
    R = c.R
    x64, y64 = c.x.double(), c.y.double()
    # norm only
    hf, h = padded(R, D)
    rstd = torch.full((R + 2,), SENT, device=dev)
    ops.adaln_fwd(c.x, c.mod, rps, EPS, gamma=c.gamma, beta=c.beta_col, h=h, rstd=rstd[:R])
    href, rref = c.norm_ref(x64)
    close(h, href)
    untouched(hf, R, D)
    assert rel_l2(rstd[:R], rref) <= 1e-5 and bool((rstd[R:] == SENT).all())
    # gate + residual only
    xmf, xm = padded(R, D)
    ops.adaln_fwd(c.x, c.mod, rps, EPS, y=c.y, gate=c.gate, xm=xm)
    xmref = x64 + y64 * c.sz
    close(xm, xmref)
    untouched(xmf, R, D)
    # gate + residual + norm: the norm of the row as stored (bf16)
    xmf2, xm2 = padded(R, D)
    hf2, h2 = padded(R, D)
    rstd2 = torch.empty(R, device=dev)
    ops.adaln_fwd(c.x, c.mod, rps, EPS, y=c.y, gate=c.gate, xm=xm2, gamma=c.gamma, beta=c.beta_col, h=h2, rstd=rstd2)
    assert torch.equal(xm2, xm)
    href2, rref2 = c.norm_ref(xm2.double())
    close(h2, href2)
    assert rel_l2(rstd2, rref2) <= 1e-5
    untouched(xmf2, R, D)
    untouched(hf2, R, D)
    # two launches: bitwise equal
    hf3, h3 = padded(R, D)
    ops.adaln_fwd(c.x, c.mod, rps, EPS, gamma=c.gamma, beta=c.beta_col, h=h3)
    assert torch.equal(h3, h)


@pytest.mark.parametrize("D,rps,B", CASES)
def test_norm_backward(D, rps, B):
    from pizero_native import ops

    c = Case(D, rps, B)
    R = c.R
    x = c.x.double().requires_grad_()
    mg = c.mod[:, D:2 * D].double().requires_grad_()
    mb = c.mod[:, 2 * D:3 * D].double().requires_grad_()
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
    h = x * r * torch.sigmoid(mg.repeat_interleave(rps, 0) + c.bg.double()) + mb.repeat_interleave(rps, 0)
    h.backward(c.dh.double())
    rstd = r.detach()[:, 0].float().contiguous()
    outs = []
    for _ in range(2):
        dxf, dx = padded(R, D)
        dmod = c.dmod.clone()
        ops.adaln_norm_bwd(c.dh, c.x, rstd, c.mod, c.gamma, dx, dmod, c.beta_col, rps, dres=c.dres)
        outs.append((dx.clone(), dmod))
        untouched(dxf, R, D)
    dx, dmod = outs[0]
    close(dx, x.grad + c.dres.double(), atol=2e-2)
    # fp32 per-sample sums over <= 51 rows: ~1e-6; a dropped row or a wrong sample is >= 1e-2
    assert rel_l2(dmod[:, D:2 * D], mg.grad) <= 1e-4
    assert rel_l2(dmod[:, 2 * D:3 * D], mb.grad) <= 1e-4
    assert bool((dmod[:, :D] == SENT).all()) and bool((dmod[:, 3 * D:] == SENT).all())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # no residual gradient
    dxf, dx0 = padded(R, D)
    ops.adaln_norm_bwd(c.dh, c.x, rstd, c.mod, c.gamma, dx0, None, c.beta_col, rps)
    close(dx0, x.grad, atol=2e-2)


@pytest.mark.parametrize("D,rps,B", CASES)
def test_gate_backward(D, rps, B):
    from pizero_native import ops

    c = Case(D, rps, B)
    R = c.R
    y = c.y.double().requires_grad_()
    mz = c.mod[:, :D].double().requires_grad_()
    out = c.x.double() + y * torch.sigmoid(mz.repeat_interleave(rps, 0) + c.bz.double())
    out.backward(c.dh.double())
    outs = []
    for _ in range(2):
        dyf, dy = padded(R, D)
        dmod = c.dmod.clone()
        ops.adaln_gate_bwd(c.dh, c.y, c.mod, c.gate, dy, dmod, rps)
        outs.append((dy.clone(), dmod))
        untouched(dyf, R, D)
    dy, dmod = outs[0]
    close(dy, y.grad, atol=2e-2)
    assert rel_l2(dmod[:, :D], mz.grad) <= 1e-4
    assert bool((dmod[:, D:] == SENT).all())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_invalid_arguments_do_not_launch():
    import pizero_native
    from pizero_native.ops import _st

    L = pizero_native.lib()
    D, rps, B = 64, 5, 3
    c = Case(D, rps, B)
    hf, h = padded(c.R, D)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def fwd(x=c.x, ldx=None, Dv=D, R=c.R, rows=rps, hh=h, ldmod=c.ldmod):
        return L.pz_adaln_fwd(p(x), x.stride(0) if ldx is None else ldx, None, 0, None, None, None, 0,
                              p(c.mod[:, D:]), p(c.bg), p(c.mod[:, 2 * D:]), p(hh), h.stride(0), None, ldmod, R, Dv,
                              rows, EPS, _st())

    assert fwd() == 0
    ok = h.clone()
    for kw in (dict(Dv=60), dict(Dv=2056), dict(x=c.x[:, 4:]), dict(ldx=c.x.stride(0) + 4), dict(rows=4), dict(rows=0),
               dict(ldmod=c.ldmod + 2)):
        assert fwd(**kw) == 1, kw  # PZ_ERR_INVALID_ARG
        assert L.pz_last_error()
    torch.cuda.synchronize()
    assert torch.equal(h, ok)
    untouched(hf, c.R, D)
    rstd = torch.ones(c.R, device=dev)
    dxf, dx = padded(c.R, D)

    def nbwd(Dv=D, rows=rps, dhv=c.dh):
        return L.pz_adaln_norm_bwd(p(dhv), c.dh.stride(0), p(c.x), c.x.stride(0), p(rstd), p(c.mod[:, D:]), p(c.bg), None,
                                   p(dx), dx.stride(0), p(c.dmod[:, D:]), p(c.dmod[:, 2 * D:]), c.ldmod, c.R, Dv, rows,
                                   _st())

    def gbwd(Dv=D, rows=rps, dhv=c.dh):
        return L.pz_adaln_gate_bwd(p(dhv), c.dh.stride(0), p(c.y), c.y.stride(0), p(c.mod), p(c.bz), p(dx), dx.stride(0),
                                   p(c.dmod), c.ldmod, c.R, Dv, rows, _st())

    for f in (nbwd, gbwd):
        for kw in (dict(Dv=60), dict(Dv=2056), dict(rows=4), dict(dhv=c.dh[:, 4:])):
            assert f(**kw) == 1, (f.__name__, kw)
    torch.cuda.synchronize()
    assert bool((dxf == SENT).all()) and bool((c.dmod == SENT).all())


@pytest.mark.parametrize("period", (100.0, 10000.0))
def test_time_embed_width_256(period):
    """pz_time_embed at the adaLN condition's width (time_hidden_size 256) against the reference SinusoidalPosEmb
    formula (vla/modules.py:15-22) in fp32, the way tests/golden/time_embed.npz pins width 1024.  Bound: the output
    is bf16 and |sin|, |cos| <= 1, so rounding alone is up to 2^-9; one further bf16 step is allowed for the
    kernel's fp32 sin / cos / exp against torch's (max 2^-8), and the mean error of rounding values spread over
    [-1, 1] stays below 2^-9 / 2 = 9.8e-4 (test_time_embed_modes_match_reference holds 6e-4: same bound here)."""
    import math

    from pizero_native import ops

    D = 256
    t = torch.linspace(0.0, 0.999, 37, device=dev)
    out = torch.empty(t.numel(), D, device=dev, dtype=torch.bfloat16)
    ops.time_embed(t, out, period)
    half = D // 2
    freq = torch.exp(torch.arange(half, device=dev, dtype=torch.float32) * -(math.log(period) / (half - 1)))
    arg = t[:, None] * freq[None, :]
    ref = torch.cat((arg.sin(), arg.cos()), dim=-1)
    err = (out.float() - ref).abs()
    assert err.max().item() <= 2.0 ** -8 and err.mean().item() <= 6e-4, (err.max().item(), err.mean().item())
    # mode 1 (the reference's bf16 arithmetic) at this width: half = 128 <= 256, so bf16 arange is exact
    out1 = torch.empty_like(out)
    ops.time_embed(t, out1, period, ref_bf16=True)
    tb = t.to(torch.bfloat16)
    fb = torch.exp(torch.arange(half, device=dev, dtype=torch.bfloat16) * -(math.log(period) / (half - 1)))
    ab = tb[:, None] * fb[None, :]
    refb = torch.cat((ab.sin(), ab.cos()), dim=-1).float()
    errb = (out1.float() - refb).abs()
    print(f"time_embed 256 period {period}: fp32 max {err.max().item():.2e} mean {err.mean().item():.2e}; "
          f"bf16-mode max {errb.max().item():.2e} mean {errb.mean().item():.2e}")
    assert errb.max().item() <= 8e-3 and errb.mean().item() <= 6e-4, (errb.max().item(), errb.mean().item())
