"""ABI 22 LoRA kernels: the rank-extended pz_gemm / pz_gemm_qkv_rope (a second operand pair summed before the
epilogue) against torch fp32 on the same bf16 operands, and pz_lora_wgrad against fp64 torch.  Every case runs
twice and the two results are compared bit for bit (no atomics anywhere on these paths)."""

import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
SENT = 1234.0

# the smallest 8-phase shape of the rank-extended planner: 10 x 16 = 160 tiles of 256 x 256 (M >= 512 rows, >= 512
# columns, >= 160 workgroups), the last row tile holding 8 rows; one row tile fewer takes the 128-tile kernel
M8, N8, K8 = 2312, 4096, 256
TILE = (72, 136, 64)  # the 128-tile kernel: partial tiles in M and N, one main K-tile
# "8phase_ktail": the same 8-phase shape with K = 264, so the last MAIN K-tile is partial as well as the extension's
# (SigLIP's fc2 forward and fc1 input gradient reduce over 4304 = 67 * 64 + 16)


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pizero_native

    pizero_native.lib()
    torch.manual_seed(0)


def bf(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(torch.bfloat16)


def close(out, ref, rtol=1.6e-2, atol=1e-2):
    """tests/test_kernels_gpu.py's bf16 gate"""
    out, ref = out.float(), ref.float()
    err = (out - ref).abs()
    bad = (err > atol + rtol * ref.abs()).sum().item()
    assert bad == 0, f"{bad} mismatches, max err {err.max().item():.4g}, max ref {ref.abs().max().item():.4g}"


def gelu(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


def twice(fn):
    """run fn() -> tuple of tensors twice; the results must agree bit for bit"""
    a = [t.clone() for t in fn()]
    b = fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two runs differ"
    return a


def kname(M, N, K, K2, **kw):
    from pizero_native import ops

    return ops.gemm_kernel_name(M, N, K, K2=K2, **kw)


def test_planner_picks_a_supporting_kernel():
    """K2 > 0 routes to the two kernels that carry the extension, whatever the plain planner prefers"""
    assert kname(M8, N8, K8, 32).startswith("gemm8p_x_kernel<true, true, false>")
    assert kname(M8, N8, K8, 32, b_kc=False).startswith("gemm8p_x_kernel<true, false, false>")
    assert kname(M8 - 256, N8, K8, 32).startswith("gemm_x_kernel")  # 9 x 16 = 144 tiles: below the threshold
    assert kname(M8, N8 - 256, K8, 32).startswith("gemm_x_kernel")
    assert kname(*TILE, 8).startswith("gemm_x_kernel")
    # K2 == 0: the names of the default path are what they were
    assert kname(M8, N8, K8, 0).startswith("gemm8p_kernel") or kname(M8, N8, K8, 0).startswith("gemm_kernel")
    # a row-slab / tall shape and a few-row shape: still served, by the 128-tile kernel
    assert "rows" in kname(276, 2048, 2048, 0) or "tall" in kname(276, 2048, 2048, 0)
    assert kname(276, 2048, 2048, 16).startswith("gemm_x_kernel")
    assert kname(4, 2048, 2048, 16).startswith("gemm_x_kernel")


@pytest.mark.parametrize("K2", [8, 32, 96])
@pytest.mark.parametrize("shape", ["tile", "8phase", "8phase_ktail"])
def test_forward_nt_epilogues(shape, K2):
    """NT (forward) layout: none + resid, bias, GELU (aux), GeGLU (aux) on x W^T + u B^T"""
    from pizero_native import ops

    M, N, K = TILE if shape == "tile" else (M8, N8, K8 if shape == "8phase" else K8 + 8)
    x, W = bf(M, K), bf(N, K, scale=K ** -0.5)
    u, Bm = bf(M, K2), bf(N, K2, scale=K2 ** -0.5)
    pre = x.float() @ W.float().t() + u.float() @ Bm.float().t()
    # The 8-phase kernel's staged epilogue rounds alpha * acc (+ bias) to bf16 before the residual is added (the
    # reference's bf16 Linear followed by a bf16 add), the 128-tile kernel rounds once.  Against an fp32 reference
    # the first form may be off by 2^-9 |pre| + 2^-9 |out|, which close() (0.01 + 0.016 |out|) covers unless
    # |pre| > 5.1 + 7.2 |out|; with |r| <= 1 (|out| >= |pre| - 1) no |pre| can satisfy that.
    b, r = bf(N), bf(M, N, scale=0.25).clamp_(-1.0, 1.0)
    want ="gemm_x_kernel" if shape == "tile" else "gemm8p_x_kernel"
    assert kname(M, N, K, K2).startswith(want)

    def run_resid():
        o = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        ops.linear(x, W, o, resid=r, lora=(u, Bm))
        return (o,)

    close(twice(run_resid)[0], pre + r.float())

    def run_bias():
        o = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        ops.linear(x, W, o, bias=b, lora=(u, Bm))
        return (o,)

    close(twice(run_bias)[0], pre + b.float())

    def run_gelu():
        o = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        aux = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        ops.linear(x, W, o, bias=b, epi=ops.PZ_EPI_GELU, aux=aux, lora=(u, Bm))
        return o, aux

    o, aux = twice(run_gelu)
    close(aux, pre + b.float())
    close(o, gelu(pre + b.float()))

    I = N // 2
    assert kname(M, N, K, K2, epi=ops.PZ_EPI_GEGLU, geglu_inter=I).startswith(
        "gemm_x_kernel" if shape == "tile" else "gemm8p_x_kernel<true, true, true>")

    def run_geglu():
        h = torch.empty(M, I, device=dev, dtype=torch.bfloat16)
        gu = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        ops.linear(x, W, h, epi=ops.PZ_EPI_GEGLU, aux=gu, lora=(u, Bm))
        return h, gu

    h, gu = twice(run_geglu)
    close(gu, pre)
    close(h, gelu(pre[:, :I]) * pre[:, I:])


@pytest.mark.parametrize("K2", [8, 32, 96])
@pytest.mark.parametrize("shape", ["tile", "8phase", "8phase_ktail"])
def test_dgrad_nn_epilogues(shape, K2):
    """NN (dgrad) layout: dx = dy W + v A, plain and with the DGELU / DGEGLU epilogues"""
    from pizero_native import ops

    M, Kin, Nout = (72, 136, 64) if shape == "tile" else (M8, N8, K8 if shape == "8phase" else K8 + 8)
    dy, W = bf(M, Nout, scale=0.5), bf(Nout, Kin, scale=Nout ** -0.5)
    v, Am = bf(M, K2, scale=0.5), bf(K2, Kin, scale=K2 ** -0.5)
    d = dy.float() @ W.float() + v.float() @ Am.float()
    want = "gemm_x_kernel" if shape == "tile" else "gemm8p_x_kernel<true, false, false>"
    assert kname(M, Kin, Nout, K2, b_kc=False).startswith(want)

    def run_plain():
        o = torch.empty(M, Kin, device=dev, dtype=torch.bfloat16)
        ops.linear_dgrad(dy, W, o, lora=(v, Am))
        return (o,)

    close(twice(run_plain)[0], d)

    pre = bf(M, Kin)
    xg = pre.float().requires_grad_()
    gelu(xg).backward(d)

    def run_dgelu():
        o = torch.empty(M, Kin, device=dev, dtype=torch.bfloat16)
        ops.linear_dgrad(dy, W, o, epi=ops.PZ_EPI_DGELU, aux=pre, lora=(v, Am))
        return (o,)

    close(twice(run_dgelu)[0], xg.grad)

    gu = bf(M, 2 * Kin)
    g, up = (t.float().requires_grad_() for t in (gu[:, :Kin], gu[:, Kin:]))
    (gelu(g) * up).backward(d)

    def run_dgeglu():
        buf = gu.clone()
        ops.linear_dgrad(dy, W, buf, epi=ops.PZ_EPI_DGEGLU, aux=buf, lora=(v, Am))  # in place over the saved g|u
        return (buf,)

    buf = twice(run_dgeglu)[0]
    close(buf[:, :Kin], g.grad)
    close(buf[:, Kin:], up.grad)


@pytest.mark.parametrize("K2", [8, 32, 96])
def test_qkv_rope_entry(K2):
    """pz_gemm_qkv_rope with the extension (hd = 256, the 8-phase kernel) against the unfused pair on the
    concatenated operands [x | u] [W | B]^T, itself checked against torch fp32"""
    from pizero_native import ops

    nh, hd = 14, 256
    N = (nh + 2) * hd
    B, T = 8, 289
    M = B * T
    assert (M, N) == (M8, N8)
    L, Lp = T + 3, T + 7
    x, W = bf(M, K8), bf(N, K8, scale=K8 ** -0.5)
    u, Bm = bf(M, K2), bf(N, K2, scale=K2 ** -0.5)
    pos = (torch.arange(T, device=dev) + 1).repeat(B).contiguous()
    cs = torch.empty((L + 9) * hd, device=dev, dtype=torch.float32)
    ops.rope_table(cs, L + 8, hd, 10000.0)

    def bufs():
        return (torch.full((B, L, nh * hd), 7.0, device=dev, dtype=torch.bfloat16),
                torch.full((B, Lp, hd), 7.0, device=dev, dtype=torch.bfloat16),
                torch.full((B, Lp, hd), 7.0, device=dev, dtype=torch.bfloat16))

    def run():
        Q, Kj, Vj = bufs()
        assert ops.gemm_qkv_rope(x, W, pos, cs, Q, Kj, Vj, T, nh, hd, L, 0, Lp, 0, lora=(u, Bm))
        return Q, Kj, Vj

    got = twice(run)
    xc, Wc = torch.cat([x, u], 1).contiguous(), torch.cat([W, Bm], 1).contiguous()
    qkv = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    ops.linear(xc, Wc, qkv)
    close(qkv, x.float() @ W.float().t() + u.float() @ Bm.float().t())
    ref = bufs()
    ops.qkv_rope_split(qkv, pos, cs, *ref, B, T, nh, 1, hd, L, 0, Lp, 0)
    for a, b in zip(got, ref):
        close(a, b)
    assert (got[0][:, T:] == 7.0).all() and (got[1][:, T:] == 7.0).all() and (got[2][:, T:] == 7.0).all()


def test_rows_shape_is_served_and_fp8_is_refused():
    from pizero_native import ops
    from pizero_native._lib import NativeError

    M, N, K, K2 = 276, 2048, 2048, 16
    x, W = bf(M, K), bf(N, K, scale=K ** -0.5)
    u, Bm = bf(M, K2), bf(N, K2, scale=K2 ** -0.5)
    o = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    ops.linear(x, W, o, lora=(u, Bm))
    close(o, x.float() @ W.float().t() + u.float() @ Bm.float().t())
    # fp8 operands with K2 > 0: PZ_ERR_UNSUPPORTED (3)
    a = ops._args(M, N, K, x, K, True, W, K, True, o, N, ops.PZ_EPI_NONE, 1.0, False, None, None, 0, None, 0, 0, 1, 1,
                  (0, 0), (0, 0), (0, 0), (0, 0))
    a.fp8_mode = 2
    a.A2, a.lda2, a.B2, a.ldb2, a.K2 = u.data_ptr(), K2, Bm.data_ptr(), K2, K2
    with pytest.raises(NativeError, match=r"rc=3"):
        ops.call("pz_gemm", C.byref(a), ops._st())
    # K2 outside 8..384 or not a multiple of 8: an argument error
    a.fp8_mode = 0
    for bad in (4, 12, 392):
        a.K2 = bad
        with pytest.raises(NativeError, match=r"rc=1"):
            ops.call("pz_gemm", C.byref(a), ops._st())


@pytest.mark.parametrize("R", [8, 32, 64])
@pytest.mark.parametrize("D", [136, 256])
@pytest.mark.parametrize("M", [264, 4104])
def test_lora_wgrad(M, D, R):
    """out (+)= alpha P^T Q in both orientations, beta 0 / 1, ldq = D + 24, and a column-slice P (ldp > R)"""
    from pizero_native import ops

    Qf = torch.full((M, D + 24), SENT, device=dev, dtype=torch.bfloat16)
    Qf[:, :D] = bf(M, D)
    Q = Qf[:, :D]
    Pf = bf(M, 3 * R)  # the fused-site case: this projection's R columns of a wider u / v
    ws = torch.empty(ops.lora_wgrad_ws_bytes(M, D, R) // 4, device=dev, dtype=torch.float32)
    assert ws.numel() >= R * D * (2 if M > 256 else 1)
    alpha = 0.5
    for P in (Pf[:, :R].contiguous(), Pf[:, R:2 * R]):
        ref = alpha * (P.double().t() @ Q.double())  # [R, D]
        for transposed in (False, True):
            shape = (D, R + 8) if transposed else (R, D + 8)
            old = torch.full(shape, SENT, device=dev, dtype=torch.bfloat16)
            view = old[:, :R] if transposed else old[:, :D]
            view.copy_(bf(*view.shape, scale=4.0))
            r = ref.t() if transposed else ref
            for beta in (False, True):
                def run():
                    o = old.clone()
                    ov = o[:, :R] if transposed else o[:, :D]
                    ops.lora_wgrad(Q, P, ov, transposed=transposed, alpha=alpha, beta=beta, ws=ws)
                    return (o,)

                o = twice(run)[0]
                ov = o[:, :R] if transposed else o[:, :D]
                close(ov, r + (view.double() if beta else 0.0))
                assert (o[:, (R if transposed else D):] == SENT).all()  # the padding of the output rows is untouched


def test_lora_wgrad_rejects_bad_arguments():
    from pizero_native import ops
    from pizero_native._lib import NativeError

    Q, P = bf(64, 64), bf(64, 8)
    out = torch.empty(8, 64, device=dev, dtype=torch.bfloat16)
    small = torch.empty(16, device=dev, dtype=torch.float32)
    with pytest.raises(NativeError, match="workspace"):
        ops.lora_wgrad(Q, P, out, ws=small)
    with pytest.raises(NativeError, match="R"):
        ops.lora_wgrad(Q, bf(64, 136), torch.empty(136, 64, device=dev, dtype=torch.bfloat16))
