"""pz_dgrad_rows (ops.linear_dgrad_rows) on the MI355X: dx[M, K] = epi(dy[M, N] @ W[N, K]) for M <= 16.

Shapes, written N -> K: the action expert's four (down_proj with DGEGLU 1024 -> 4096, gate|up 8192 -> 1024, o_proj
1024 -> 2048, q|k|v 2560 -> 1024) and three that leave the kernel's regular geometry: 72 -> 40 (N below one 32-row
step per split, K below a wave's 512 columns), 8 -> 8 (one vector, one row group) and 520 -> 1000 (ragged last slab,
K no multiple of 512).  M in {1, 5, 8, 16}: one row, the B = 1 tied group's C + H = 5, and both ends of the 8- and
16-row accumulator forms.  Both epilogues on every shape, each with contiguous and with row-strided dy / dx.

References: the fp32 product of the same bf16 inputs (DGEGLU: torch autograd of gelu_tanh(g) * u in fp32) and
ops.linear_dgrad, with the bounds tests/test_kernels_gpu.py holds the same quantities to: rtol 1.6e-2 and atol
3e-2 * sqrt(N) / 8 for the plain product (its line 101), atol 2e-2 for DGEGLU on unit-scale inputs (its lines 304-305).
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
EXPERT = [(1024, 4096), (8192, 1024), (1024, 2048), (2560, 1024)]
ODD = [(72, 40), (8, 8), (520, 1000)]
ROWS = [1, 5, 8, 16]
PAD = 8  # extra columns of the row-strided buffers (keeps rows 16-byte aligned)


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pizero_native

    pizero_native.lib()


def _bf(*shape, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, device=dev, generator=g) * scale).to(BF16)


def _close(out, ref, rtol=1.6e-2, atol=1e-2):
    out, ref = out.float(), ref.float()
    err = (out - ref).abs()
    bad = (err > atol + rtol * ref.abs()).sum().item()
    print(f"max err {err.max().item():.4g} (atol {atol:.4g}), max ref {ref.abs().max().item():.4g}")
    assert bad == 0, f"{bad} mismatches, max err {err.max().item():.4g}, max ref {ref.abs().max().item():.4g}"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _strided(x):
    """x's values in a buffer with PAD more columns per row (NaN in the pad)"""
    buf = torch.full((x.shape[0], x.shape[1] + PAD), float("nan"), device=dev, dtype=BF16)
    buf[:, :x.shape[1]] = x
    return buf, buf[:, :x.shape[1]]


def _ws(M, N, K, fill=None):
    import pizero_native

    n = pizero_native.lib().pz_dgrad_rows_ws_bytes(M, N, K) // 4
    assert n >= M * K
    ws = torch.empty(n, device=dev, dtype=torch.float32)
    if fill is not None:
        ws.fill_(fill)
    return ws


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("N,K", EXPERT + ODD)
@pytest.mark.parametrize("M", ROWS)
def test_plain(M, N, K, strided):
    from pizero_native import ops

    dy, W = _bf(M, N, seed=1), _bf(N, K, seed=2, scale=N ** -0.5)
    ref = dy.float() @ W.float()
    atol = 3e-2 * math.sqrt(N) / 8
    dyv = _strided(dy)[1] if strided else dy
    hold, dx = _strided(torch.zeros(M, K, device=dev, dtype=BF16)) if strided else (None, torch.empty(M, K, device=dev,
                                                                                                      dtype=BF16))
    assert ops.linear_dgrad_rows(dyv, W, dx, ws=_ws(M, N, K)) is True
    _close(dx, ref, atol=atol)
    if strided:
        assert torch.isnan(hold[:, K:]).all(), "columns past K of a row-strided dx were written"
    old = torch.empty(M, K, device=dev, dtype=BF16)
    ops.linear_dgrad(dy, W, old)
    _close(dx, old, atol=atol)
    # no state: workspace and output full of NaN beforehand, the same bits afterwards
    again = torch.full_like(dx, float("nan"))
    assert ops.linear_dgrad_rows(dyv, W, again, ws=_ws(M, N, K, fill=float("nan"))) is True
    assert torch.equal(_bits(again), _bits(dx))


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("N,K", EXPERT + ODD)
@pytest.mark.parametrize("M", ROWS)
def test_dgeglu(M, N, K, strided):
    """K is the GeGLU width I: aux = saved [g | u] [M, 2K], the output [M, 2K] written over aux itself"""
    from pizero_native import ops

    dy, W, gu = _bf(M, N, seed=3, scale=0.5), _bf(N, K, seed=4, scale=N ** -0.5), _bf(M, 2 * K, seed=5)
    g, u = (t.float().requires_grad_() for t in (gu[:, :K], gu[:, K:]))
    (torch.nn.functional.gelu(g, approximate="tanh") * u).backward(dy.float() @ W.float())
    dyv = _strided(dy)[1] if strided else dy
    hold, buf = _strided(gu) if strided else (None, gu.clone())
    assert ops.linear_dgrad_rows(dyv, W, buf, epi=ops.PZ_EPI_DGEGLU, aux=buf, ws=_ws(M, N, K)) is True  # in place
    _close(buf[:, :K], g.grad, atol=2e-2)
    _close(buf[:, K:], u.grad, atol=2e-2)
    if strided:
        assert torch.isnan(hold[:, 2 * K:]).all(), "columns past 2K of a row-strided dx were written"
    old = gu.clone()
    ops.linear_dgrad(dy, W, old, epi=ops.PZ_EPI_DGEGLU, aux=old)
    _close(buf, old, atol=2e-2)
    # out of place into NaN with a NaN workspace: the bits of the in-place run
    out = torch.full((M, 2 * K), float("nan"), device=dev, dtype=BF16)
    assert ops.linear_dgrad_rows(dyv, W, out, epi=ops.PZ_EPI_DGEGLU, aux=gu, ws=_ws(M, N, K, fill=float("nan"))) is True
    assert torch.equal(_bits(out), _bits(buf))


def test_default_workspace():
    """without ws the GEMM split-K scratch of the stream slot is used: the same bits"""
    from pizero_native import ops

    M, N, K = 5, 1024, 2048
    dy, W = _bf(M, N, seed=6), _bf(N, K, seed=7, scale=N ** -0.5)
    a, b = (torch.empty(M, K, device=dev, dtype=BF16) for _ in range(2))
    assert ops.linear_dgrad_rows(dy, W, a) is True
    assert ops.linear_dgrad_rows(dy, W, b, ws=_ws(M, N, K)) is True
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("M,N,K,epi", [(17, 1024, 1024, "none"), (5, 12, 1024, "none"), (5, 1024, 12, "none"),
                                       (5, 1024, 1024, "dgelu")])
def test_unsupported_leaves_the_output_alone(M, N, K, epi):
    import ctypes

    import pizero_native
    from pizero_native import ops

    L = pizero_native.lib()
    dy, W = _bf(M, N, seed=8), _bf(N, K, seed=9)
    dx = torch.full((M, K), 3.0, device=dev, dtype=BF16)
    code = {"none": ops.PZ_EPI_NONE, "dgelu": ops.PZ_EPI_DGELU}[epi]
    aux = _bf(M, K, seed=10) if epi == "dgelu" else None
    assert ops.linear_dgrad_rows(dy, W, dx, epi=code, aux=aux) is False
    ws = torch.empty(1 << 20, device=dev, dtype=torch.float32)
    rc = L.pz_dgrad_rows(dy.data_ptr(), N, W.data_ptr(), K, dx.data_ptr(), K, M, N, K, code,
                         None if aux is None else aux.data_ptr(), K, ws.data_ptr(), ws.numel() * 4,
                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == ops.PZ_ERR_UNSUPPORTED and b"not supported" in L.pz_last_error()
    assert L.pz_dgrad_rows_ws_bytes(M, N, K) == 0 or epi == "dgelu"
    torch.cuda.synchronize()
    assert (dx == 3.0).all()
