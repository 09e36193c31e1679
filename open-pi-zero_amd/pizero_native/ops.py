"""Thin torch-tensor front-ends over the C ABI (pointer/size plumbing only).

Every function enqueues HIP kernels on torch's current stream; tensors are
owned by the caller (PyTorch caching allocator), nothing is allocated on the
native side, so every sequence of these calls is hipGraph-capturable.
"""

from __future__ import annotations

import ctypes as C

import torch

from ._lib import (
    PZ_EPI_DGEGLU,
    PZ_EPI_DGELU,
    PZ_EPI_DSILU,
    PZ_EPI_GEGLU,
    PZ_EPI_GELU,
    PZ_EPI_NONE,
    PZ_EPI_SILU,
    PZ_OBS_MAX_EXTENT,
    PZ_OBS_MAX_TAPS,
    PZ_OBS_NORM_BOUND,
    PZ_OBS_NORM_GAUSSIAN,
    PZ_Q4_MAX_SEGS,
    PZ_SUMSQ_PARTS,
    AdamW8Args,
    QkvRopeArgs,
    DecodeAttnArgs,
    ExpertAttnBwdArgs,
    FlashArgs,
    GemmArgs,
    Q4Seg,
    SmallGemmArgs,
    NativeError,
    SoftmaxArgs,
    call,
    lib,
)

__all__ = ["PZ_EPI_NONE", "PZ_EPI_GELU", "PZ_EPI_GEGLU", "PZ_EPI_SILU", "PZ_EPI_DGELU", "PZ_EPI_DSILU", "PZ_EPI_DGEGLU"]

BF16 = torch.bfloat16


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


_PROBE = None


def set_probe(pred):
    """Record (start, end) HIP events around every pz_gemm launch for which pred(M, N, K, epi, batch)
    is true, on the launch stream (bench.py measures the dominant kernel's duration live)."""
    global _PROBE
    _PROBE = None if pred is None else (pred, [])
    return None if _PROBE is None else _PROBE[1]


def gemm(M, N, K, A, lda, a_kc, B, ldb, b_kc, Cm, ldc, *, epi=PZ_EPI_NONE, alpha=1.0, beta=False,
         bias=None, resid=None, ld_resid=0, aux=None, ld_aux=0, geglu_inter=0, batch=1, batch_inner=1,
         sA=(0, 0), sB=(0, 0), sC=(0, 0), sR=(0, 0), norm=None, ext=None):
    """Raw GEMM: see pz_gemm_args in include/pz_abi.h.  Element strides.  norm = (w, eps): fused
    Gemma RMSNorm of the A rows (few-row path only).  ext = (A2, lda2, B2, ldb2, K2): the rank extension
    (a second operand pair with the k-contiguity of A / B, summed before the epilogue)."""
    if _PROBE is not None and _PROBE[0](M, N, K, epi, batch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _gemm(M, N, K, A, lda, a_kc, B, ldb, b_kc, Cm, ldc, epi, alpha, beta, bias, resid, ld_resid, aux, ld_aux,
              geglu_inter, batch, batch_inner, sA, sB, sC, sR, norm, ext)
        e1.record()
        _PROBE[1].append((e0, e1))
        return
    _gemm(M, N, K, A, lda, a_kc, B, ldb, b_kc, Cm, ldc, epi, alpha, beta, bias, resid, ld_resid, aux, ld_aux,
          geglu_inter, batch, batch_inner, sA, sB, sC, sR, norm, ext)


_WS_BYTES = 160 << 20  # split-K / split-tail fp32 partials (multi-round tails: up to 640 x 256 KiB)
_WS = {}


_WS_SLOT = [0]


class workspace_slot:
    """``with workspace_slot(1):`` -- GEMMs enqueued inside use their own split-K / split-tail scratch (the
    engine's second stream for the action-expert group runs GEMMs concurrently with the main stream's)."""

    def __init__(self, slot):
        self.slot, self.prev = slot, None

    def __enter__(self):
        self.prev = _WS_SLOT[0]
        _WS_SLOT[0] = self.slot

    def __exit__(self, *exc):
        _WS_SLOT[0] = self.prev


def workspace(device=None):
    """Per-device fp32 split-K scratch for pz_gemm (allocated once, before any graph capture
    reuses it; GEMMs are stream-ordered within a stream, so one buffer per stream slot is enough:
    slot 0 = the main stream, slot 1 = the engine's action-expert stream)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (dev, _WS_SLOT[0])
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(_WS_BYTES // 4, dtype=torch.float32, device=dev)
        _WS[key] = ws
    return ws


def _args(M, N, K, A, lda, a_kc, B, ldb, b_kc, Cm, ldc, epi, alpha, beta, bias, resid, ld_resid, aux, ld_aux,
          geglu_inter, batch, batch_inner, sA, sB, sC, sR, ws=None, norm=None):
    a = GemmArgs()
    a.M, a.N, a.K = int(M), int(N), int(K)
    a.A, a.lda, a.a_kcontig = _p(A), int(lda), int(bool(a_kc))
    a.B, a.ldb, a.b_kcontig = _p(B), int(ldb), int(bool(b_kc))
    a.C, a.ldc, a.c_fp32 = _p(Cm), int(ldc), int(Cm.dtype == torch.float32)
    a.batch, a.batch_inner = int(batch), int(batch_inner)
    a.sA_outer, a.sA_inner = int(sA[0]), int(sA[1])
    a.sB_outer, a.sB_inner = int(sB[0]), int(sB[1])
    a.sC_outer, a.sC_inner = int(sC[0]), int(sC[1])
    a.sR_outer, a.sR_inner = int(sR[0]), int(sR[1])
    a.epilogue, a.alpha, a.beta_accum = int(epi), float(alpha), int(bool(beta))
    a.bias, a.resid, a.ld_resid = _p(bias), _p(resid), int(ld_resid)
    a.aux, a.ld_aux, a.geglu_inter = _p(aux), int(ld_aux), int(geglu_inter)
    if ws is not None:
        a.workspace, a.ws_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    if norm is not None:
        a.norm_w, a.norm_eps = _p(norm[0]), float(norm[1])
    return a


def _gemm(M, N, K, A, lda, a_kc, B, ldb, b_kc, Cm, ldc, epi, alpha, beta, bias, resid, ld_resid, aux, ld_aux,
          geglu_inter, batch, batch_inner, sA, sB, sC, sR, norm=None, ext=None):
    ws = workspace(Cm.device) if batch == 1 else None
    a = _args(M, N, K, A, lda, a_kc, B, ldb, b_kc, Cm, ldc, epi, alpha, beta, bias, resid, ld_resid, aux, ld_aux,
              geglu_inter, batch, batch_inner, sA, sB, sC, sR, ws, norm)
    if ext is not None:
        a.A2, a.lda2, a.B2, a.ldb2, a.K2 = _p(ext[0]), int(ext[1]), _p(ext[2]), int(ext[3]), int(ext[4])
    call("pz_gemm", C.byref(a), _st())


def gemm_kernel_name(M, N, K, *, a_kc=True, b_kc=True, epi=PZ_EPI_NONE, geglu_inter=0, batch=1, c_fp32=False,
                     workspace_bytes=_WS_BYTES, fp8_mode=0, K2=0):
    """Name of the kernel pz_gemm dispatches for this problem (bench / profile labels; fp8_mode 1 = W8A8 with row
    scales, 2 = W8A16, K in codes; K2: depth of the rank extension)."""
    a = GemmArgs()
    a.M, a.N, a.K = int(M), int(N), int(K)
    a.a_kcontig, a.b_kcontig, a.c_fp32 = int(a_kc), int(b_kc), int(c_fp32)
    a.batch, a.batch_inner, a.epilogue, a.geglu_inter = int(batch), 1, int(epi), int(geglu_inter)
    a.workspace, a.ws_bytes = (256 if workspace_bytes else None), int(workspace_bytes)
    a.fp8_mode = int(fp8_mode)
    a.K2 = int(K2)
    if fp8_mode == 1:
        a.a_row_scale, a.lda, a.ldb = 256, int(K), int(K)
    return lib().pz_gemm_kernel_name(C.byref(a)).decode()


def linear(x, W, out, *, bias=None, resid=None, epi=PZ_EPI_NONE, aux=None, alpha=1.0, beta=False, norm=None,
           lora=None):
    """out[M,N] = epi(x[M,K] @ W[N,K]^T): nn.Linear forward (x, out may be row-strided 2-D views).
    norm = (w, eps): x is first Gemma-RMS-normalised inside the GEMM (M <= 16 rows only).
    lora = (u [M, R], Bm [N, R]): out = epi(x W^T + u Bm^T), the adapter term summed inside the GEMM."""
    M, K = x.shape
    N = W.shape[0]
    ext = None if lora is None else (lora[0], lora[0].stride(0), lora[1], lora[1].stride(0), lora[0].shape[1])
    if epi == PZ_EPI_GEGLU:
        I = N // 2
        gemm(M, N, K, x, x.stride(0), True, W, W.stride(0), True, out, out.stride(0), epi=epi,
             aux=aux, ld_aux=0 if aux is None else aux.stride(0), geglu_inter=I, alpha=alpha, norm=norm, ext=ext)
        return out
    gemm(M, N, K, x, x.stride(0), True, W, W.stride(0), True, out, out.stride(0), epi=epi, alpha=alpha,
         beta=beta, bias=bias, resid=resid, ld_resid=0 if resid is None else resid.stride(0), aux=aux,
         ld_aux=0 if aux is None else aux.stride(0), norm=norm, ext=ext)
    return out


def lora_wgrad_ws_bytes(M, D, R):
    """bytes of fp32 workspace pz_lora_wgrad needs for Q [M, D] and P [M, R]"""
    return int(lib().pz_lora_wgrad_ws_bytes(int(M), int(D), int(R)))


def lora_wgrad(Q, P, out, *, transposed=False, alpha=1.0, beta=False, ws=None):
    """out[R, D] (+)= alpha P[M, R]^T Q[M, D] (transposed: out[D, R]); Q / P may be column slices of wider
    row-major tensors.  Deterministic fixed-order reduction over M through the fp32 workspace ws (default: the
    GEMM workspace of the current stream slot)."""
    M, D = Q.shape
    R = P.shape[1]
    ws = workspace(Q.device) if ws is None else ws
    call("pz_lora_wgrad", _p(Q), Q.stride(0), _p(P), P.stride(0), _p(out), out.stride(0), M, D, R, int(transposed),
         float(alpha), int(bool(beta)), _p(ws), ws.numel() * ws.element_size(), _st())
    return out


# ---------------------------------------------------------------- fp8 (C5) ----
ABSMAX_PARTS = 1024  # include/pz_abi.h PZ_ABSMAX_PARTS
E4M3_MAX = 448.0


def fp8_quant_rows(x, q, row_scale):
    """per-row fp8 e4m3 codes of bf16 x [R, D] (q uint8 [R, D], row_scale fp32 [R] = max|row| / 448)"""
    R, D = x.shape
    call("pz_fp8_quant_rows", _p(x), x.stride(0), _p(q), q.stride(0), _p(row_scale), R, D, _st())


def rmsnorm_f8(x, w, q, qscale, eps):
    """Gemma RMSNorm of x [R, D] straight to e4m3 codes q [R, D] + per-row scales (pz_rmsnorm_fwd_f8)"""
    R, D = x.shape
    call("pz_rmsnorm_fwd_f8", _p(x), x.stride(0), _p(w), _p(q), q.stride(0), _p(qscale), R, D, float(eps), _st())


def layernorm_f8(x, w, b, q, qscale, eps):
    """LayerNorm of x [R, D] straight to e4m3 codes q [R, D] + per-row scales (pz_layernorm_fwd_f8)"""
    R, D = x.shape
    call("pz_layernorm_fwd_f8", _p(x), x.stride(0), _p(w), _p(b), _p(q), q.stride(0), _p(qscale), R, D, float(eps),
         _st())


def fp8_quant_tensor(x, q, scale):
    """q = e4m3(x / scale) elementwise (weights; scale = max|x| / 448 from fp8_weight_scale)"""
    call("pz_fp8_quant_tensor", _p(x), x.numel(), _p(q), 1.0 / float(scale), _st())


def fp8_weight_scale(x):
    """per-tensor weight scale max|x| / 448 (load-time: pz_fp8_absmax partials, host max)"""
    parts = torch.empty(ABSMAX_PARTS, device=x.device, dtype=torch.float32)
    call("pz_fp8_absmax", _p(x), x.numel(), _p(parts), _st())
    m = float(parts.max().item())
    return m / E4M3_MAX if m > 0 else 1.0


def linear_fp8(x, Wq, w_scale, out, *, bias=None, resid=None, epi=PZ_EPI_NONE, aux=None, norm=None,
               x_scale=None):
    """out = epi(x @ W^T) with fp8 e4m3 weights Wq [N, K] (uint8 codes, per-tensor w_scale).
    x_scale None: x bf16 rows (W8A16, M <= 64: codes expanded to bf16 in registers; norm allowed);
    else x uint8 codes [M, K] with per-row scales x_scale (W8A8 on the fp8 MFMA, 256-tile kernel)."""
    M, K = x.shape
    N = Wq.shape[0]
    a = _args(M, N, K, x, x.stride(0), True, Wq, Wq.stride(0), True, out, out.stride(0), epi, w_scale, False, bias,
              resid, 0 if resid is None else resid.stride(0), aux, 0 if aux is None else aux.stride(0),
              N // 2 if epi == PZ_EPI_GEGLU else 0, 1, 1, (0, 0), (0, 0), (0, 0), (0, 0), workspace(out.device),
              norm)
    a.fp8_mode = 2 if x_scale is None else 1
    a.a_row_scale = _p(x_scale)
    call("pz_gemm", C.byref(a), _st())
    return out


def rows_w8a16_ok(M, K, ncols):
    """e4m3 weights with bf16 rows above 64 rows: the row-slab kernel's shapes (pz_gemm_host.hip plan_rows: 64 < M <=
    1024, K % 64 == 0, K <= 2048, <= 4096 output columns; PZ_GEMM_ROWS=0: never, =1: any K / width, as the planner).
    tests/test_abi.py::test_gemm_routes_golden holds this to the planner."""
    import os

    rows = os.environ.get("PZ_GEMM_ROWS")
    if rows == "0":
        return False
    return 64 < M <= 1024 and K % 64 == 0 and (rows == "1" or (K <= 2048 and ncols <= 4096))


def linear_dgrad(dy, W, dx, *, beta=False, resid=None, epi=PZ_EPI_NONE, aux=None, lora=None):
    """dx[M,K] (+)= dy[M,N] @ W[N,K] (+ resid).

    Backward epilogues (aux read): PZ_EPI_DGELU / PZ_EPI_DSILU multiply by the activation
    derivative at the saved pre-activation aux[M,K]; PZ_EPI_DGEGLU takes aux = saved [g | u]
    ([M, 2K]) and writes d(gate|up) into dx[M, 2K] (dx may be aux itself).
    lora = (v [M, R], Am [R, K]): dx = epi(dy W + v Am), the adapter's input gradient summed inside the GEMM."""
    M, N = dy.shape
    K = W.shape[1]
    ext = None if lora is None else (lora[0], lora[0].stride(0), lora[1], lora[1].stride(0), lora[0].shape[1])
    gemm(M, K, N, dy, dy.stride(0), True, W, W.stride(0), False, dx, dx.stride(0), beta=beta,
         resid=resid, ld_resid=0 if resid is None else resid.stride(0), epi=epi, aux=aux,
         ld_aux=0 if aux is None else aux.stride(0), geglu_inter=K if epi == PZ_EPI_DGEGLU else 0, ext=ext)
    return dx


def linear_dgrad_rows(dy, W, dx, *, epi=PZ_EPI_NONE, aux=None, ws=None):
    """linear_dgrad for a handful of rows (pz_dgrad_rows: M <= 16, N % 8 == 0, K % 8 == 0, PZ_EPI_NONE or
    PZ_EPI_DGEGLU): W [N, K] is reduced along its rows by every CU, not by the K / 128 workgroups of the 128-tile
    kernel that pz_gemm plans for a k-strided B.  Returns False, with nothing launched and dx untouched, when the
    kernel does not take the call -- the caller then runs linear_dgrad.  ws: fp32 scratch (default: the GEMM
    split-K scratch of the current stream slot)."""
    M, N = dy.shape
    K = W.shape[1]
    if dy.stride(1) != 1 or W.stride(1) != 1 or dx.stride(1) != 1 or (aux is not None and aux.stride(1) != 1):
        return False
    need = lib().pz_dgrad_rows_ws_bytes(M, N, K)
    if ws is None:
        ws = workspace(dx.device)
        if ws.numel() * 4 < need:
            return False
    rc = lib().pz_dgrad_rows(_p(dy), dy.stride(0), _p(W), W.stride(0), _p(dx), dx.stride(0), M, N, K, int(epi), _p(aux),
                             0 if aux is None else aux.stride(0), _p(ws), ws.numel() * ws.element_size(), _st())
    if rc == PZ_ERR_UNSUPPORTED:
        return False
    if rc != 0:
        raise NativeError(f"pz_dgrad_rows failed (rc={rc}): {lib().pz_last_error().decode(errors='replace')}")
    return True


def _split_k(M, N, K):
    """Split the token (reduction) dim when the output has too few 256x256 tiles to fill 256 CUs."""
    tiles = ((N + 255) // 256) * ((K + 255) // 256)
    if tiles >= 160 or M < 4096 or N < 512 or K < 512 or M % 8 == 0:
        return 1  # (M % 8 == 0: the 8-phase kernel splits K itself -- pz_gemm "split tail")
    best = 1
    for s in (2, 4, 8):  # fewest splits that reach ~1 wave of 256-thread... 240+ workgroups
        if M % (s * 64) == 0:
            best = s
            if tiles * s >= 240:
                break
    return best


def linear_wgrad(dy, x, dW, *, beta=False):
    """dW[N,K] (+)= dy[M,N]^T @ x[M,K]   (split-K over tokens into fp32 slabs when the output is small)."""
    M, N = dy.shape
    K = x.shape[1]
    S = _split_k(M, N, K) if dW.is_contiguous() else 1
    if S == 1:
        gemm(N, K, M, dy, dy.stride(0), False, x, x.stride(0), False, dW, dW.stride(0), beta=beta)
        return dW
    Mc = M // S
    slabs = torch.empty(S, N, K, device=dW.device, dtype=torch.float32)
    gemm(N, K, Mc, dy, dy.stride(0), False, x, x.stride(0), False, slabs, K, batch=S,
         sA=(Mc * dy.stride(0), 0), sB=(Mc * x.stride(0), 0), sC=(N * K, 0))
    reduce_parts(slabs.view(S, N * K), dW.view(-1), beta=beta)
    return dW


def small_linear(x, W, out, *, bias=None, beta=False):
    """out[M,N] = x[M,K] W[N,K]^T for tiny K or N (7-dim action/proprio)."""
    M, K = x.shape
    N = W.shape[0]
    a = SmallGemmArgs()
    a.M, a.N, a.K = M, N, K
    a.A, a.sAm, a.sAk = _p(x), x.stride(0), x.stride(1)
    a.B, a.sBk, a.sBn = _p(W), W.stride(1), W.stride(0)
    a.C, a.ldc, a.bias, a.alpha, a.beta = _p(out), out.stride(0), _p(bias), 1.0, int(beta)
    call("pz_gemm_small", C.byref(a), _st())
    return out


def small_gemm(M, N, K, A, sAm, sAk, B, sBk, sBn, out, ldc, *, beta=False, bias=None):
    a = SmallGemmArgs()
    a.M, a.N, a.K = M, N, K
    a.A, a.sAm, a.sAk = _p(A), sAm, sAk
    a.B, a.sBk, a.sBn = _p(B), sBk, sBn
    a.C, a.ldc, a.bias, a.alpha, a.beta = _p(out), ldc, _p(bias), 1.0, int(beta)
    call("pz_gemm_small", C.byref(a), _st())
    return out


def rmsnorm(x, w, y, rstd, eps):
    R, D = x.shape
    call("pz_rmsnorm_fwd", _p(x), x.stride(0), _p(w), _p(y), y.stride(0), _p(rstd), R, D, float(eps), _st())
    return y


def rmsnorm_bwd(dy, x, w, rstd, dx, dres=None, dw_part=None):
    R, D = x.shape
    call("pz_rmsnorm_bwd", _p(dy), dy.stride(0), _p(x), x.stride(0), _p(w), _p(rstd), _p(dres), _p(dx),
         dx.stride(0), _p(dw_part), R, D, _st())
    return dx


def layernorm(x, w, b, y, mean, rstd, eps):
    R, D = x.shape
    call("pz_layernorm_fwd", _p(x), x.stride(0), _p(w), _p(b), _p(y), y.stride(0), _p(mean), _p(rstd), R, D,
         float(eps), _st())
    return y


def layernorm_bwd(dy, x, w, mean, rstd, dx, dres=None, dw_part=None, db_part=None, dx_part=None):
    """dx_part: per-part column sums of the bf16 dx (reduce_parts -> the bias gradient of the Linear whose output
    gradient dx is)"""
    R, D = x.shape
    call("pz_layernorm_bwd", _p(dy), dy.stride(0), _p(x), x.stride(0), _p(w), _p(mean), _p(rstd), _p(dres),
         _p(dx), dx.stride(0), _p(dw_part), _p(db_part), R, D, _p(dx_part), _st())
    return dx


def adaln_fwd(x, mod, rows_per_sample, eps, *, y=None, gate=None, xm=None, gamma=None, beta=None, h=None, rstd=None):
    """adaLN row pass (pz_adaln_fwd).  mod: fp32 [B, N] modulation rows; gate / gamma / beta: that slot's first
    column in mod; gate = (column, bias [D]) with y, xm: xm = x + y * sigmoid(mod[b, gate] + bias);
    gamma = (column, bias [D]) with beta, h: h = norm(xm) * sigmoid(mod[b, gamma] + bias) + mod[b, beta]."""
    R, D = x.shape
    gp = gb = gmp = gmb = bp = None
    if y is not None:
        gp, gb = mod[:, gate[0]:].data_ptr(), _p(gate[1])
    if h is not None:
        gmp, gmb, bp = mod[:, gamma[0]:].data_ptr(), _p(gamma[1]), mod[:, beta:].data_ptr()
    call("pz_adaln_fwd", _p(x), x.stride(0), _p(y), 0 if y is None else y.stride(0), gp, gb, _p(xm),
         0 if xm is None else xm.stride(0), gmp, gmb, bp, _p(h), 0 if h is None else h.stride(0), _p(rstd),
         mod.stride(0), R, D, int(rows_per_sample), float(eps), _st())


def adaln_norm_bwd(dh, x, rstd, mod, gamma, dx, dmod, beta, rows_per_sample, dres=None):
    """backward of the adaptive norm: dx = dres + ...; dmod[b, gamma[0]:+D] and dmod[b, beta:+D] (fp32 [B, N], the
    layout of mod) receive the sample's d gamma_pre / d beta sums (written, deterministic)"""
    R, D = x.shape
    call("pz_adaln_norm_bwd", _p(dh), dh.stride(0), _p(x), x.stride(0), _p(rstd), mod[:, gamma[0]:].data_ptr(),
         _p(gamma[1]), _p(dres), _p(dx), dx.stride(0), None if dmod is None else dmod[:, gamma[0]:].data_ptr(),
         None if dmod is None else dmod[:, beta:].data_ptr(), mod.stride(0), R, D, int(rows_per_sample), _st())
    return dx


def adaln_gate_bwd(dout, y, mod, gate, dy, dmod, rows_per_sample):
    """backward of the gated branch: dy = dout * sigmoid(.), dmod[b, gate[0]:+D] = the sample's d gate_pre"""
    R, D = y.shape
    call("pz_adaln_gate_bwd", _p(dout), dout.stride(0), _p(y), y.stride(0), mod[:, gate[0]:].data_ptr(), _p(gate[1]),
         _p(dy), dy.stride(0), dmod[:, gate[0]:].data_ptr(), mod.stride(0), R, D, int(rows_per_sample), _st())
    return dy


def act_bwd_colsum(dh, pre, dpre, act, ws, dbias, beta=False):
    """dpre = dh * act'(pre) (dpre may alias dh) and dbias (+)= colsum(dpre) in one pass; ws fp32 [rows >= 16, N]"""
    M, N = pre.shape
    call("pz_act_bwd_colsum", _p(dh), dh.stride(0), _p(pre), pre.stride(0), _p(dpre), M, N, int(act), _p(ws),
         ws.numel() // N, _p(dbias), int(beta), _st())
    return dpre


_RPP = None


def rows_per_part():
    global _RPP
    if _RPP is None:
        from ._lib import lib

        _RPP = int(lib().pz_norm_rows_per_part())
    return _RPP


def reduce_parts(part, out, beta=False):
    P, D = part.shape
    call("pz_reduce_parts", _p(part), P, D, _p(out), int(beta), _st())
    return out


def reduce_parts_multi(items, beta=False):
    """[(part [P, D] fp32, out [D] bf16)]: every out (+)= the column sums of its part, one launch"""
    from ._lib import ReduceSeg

    if not items:
        return
    segs = (ReduceSeg * len(items))()
    for s, (part, out) in zip(segs, items):
        s.part, s.P, s.D, s.out, s.beta = _p(part), part.shape[0], part.shape[1], _p(out), int(beta)
    call("pz_reduce_parts_multi", C.cast(segs, C.c_void_p), len(items), _st())


def colsum(X, out, ws, beta=False):
    M, N = X.shape
    call("pz_colsum", _p(X), X.stride(0), M, N, _p(out), int(beta), _p(ws), _st())
    return out


def batch_sum(X, B, stride, n, out, beta=False):
    call("pz_batch_sum", _p(X), B, stride, n, _p(out), int(beta), _st())
    return out


def rope_table(cs, max_pos, head_dim, theta):
    call("pz_rope_table", _p(cs), max_pos, head_dim, float(theta), _st())
    return cs


def qkv_rope_split(qkv, pos, cs, q_out, k_out, v_out, B, T, nh, nkv, hd, Lq, qoff, Lk, koff):
    call("pz_qkv_rope_split", _p(qkv), _p(pos), _p(cs), _p(q_out), _p(k_out), _p(v_out), B, T, nh, nkv, hd,
         Lq, qoff, Lk, koff, _st())


def qkv_rope_split_bwd(dq, dk, dv, pos, cs, dqkv, B, T, nh, nkv, hd, Lq, qoff, Lk, koff):
    call("pz_qkv_rope_split_bwd", _p(dq), _p(dk), _p(dv), _p(pos), _p(cs), _p(dqkv), B, T, nh, nkv, hd, Lq,
         qoff, Lk, koff, _st())


def gemv_qkv_rope(x, W, pos, cs, q_out, k_out, v_out, T, nh, hd, Lq, qoff, Lk, koff, norm=None):
    """Few-row q|k|v projection (+ fused RMSNorm) with RoPE and the Q / K / V scatter as its epilogue."""
    a = QkvRopeArgs()
    a.x, a.ldx = _p(x), x.stride(0)
    a.W, a.ldw = _p(W), W.stride(0)
    a.M, a.N, a.K = x.shape[0], W.shape[0], x.shape[1]
    if norm is not None:
        a.norm_w, a.norm_eps = _p(norm[0]), float(norm[1])
    a.pos, a.cs = _p(pos), _p(cs)
    a.q_out, a.k_out, a.v_out = _p(q_out), _p(k_out), _p(v_out)
    a.T, a.nh, a.hd, a.Lq, a.qoff, a.Lk, a.koff = T, nh, hd, Lq, qoff, Lk, koff
    call("pz_gemv_qkv_rope", C.byref(a), _st())


PZ_ERR_UNSUPPORTED = 3  # include/pz_abi.h


def gemm_qkv_rope(x, W, pos, cs, q_out, k_out, v_out, T, nh, hd, Lq, qoff, Lk, koff, norm=None, w_scale=None,
                  lora=None):
    """q|k|v projection with RoPE and the joint Q / K / V scatter fused into the GEMM's epilogue
    (pz_gemm_qkv_rope): the 8-phase kernel for many rows, the skinny-64 kernel for 16 < M <= 64 (norm = (w, eps):
    fused Gemma RMSNorm; w_scale: W is e4m3 codes, W8A16 -- few-row path only).  Returns False (nothing launched) when the shape takes neither --
    the caller then runs linear + qkv_rope_split (same bits)."""
    a = QkvRopeArgs()
    a.x, a.ldx = _p(x), x.stride(0)
    a.W, a.ldw = _p(W), W.stride(0)
    a.M, a.N, a.K = x.shape[0], W.shape[0], x.shape[1]
    if norm is not None:
        a.norm_w, a.norm_eps = _p(norm[0]), float(norm[1])
    if w_scale is not None:  # W = e4m3 codes (uint8 [N, K]) with a per-tensor scale: few-row W8A16 path
        a.w_fp8, a.w_scale = 1, float(w_scale)
    a.pos, a.cs = _p(pos), _p(cs)
    a.q_out, a.k_out, a.v_out = _p(q_out), _p(k_out), _p(v_out)
    a.T, a.nh, a.hd, a.Lq, a.qoff, a.Lk, a.koff = T, nh, hd, Lq, qoff, Lk, koff
    if lora is not None:  # (u [M, R], Bm [N, R]): the adapter term summed inside the GEMM (8-phase path only)
        a.x2, a.ldx2, a.W2, a.ldw2, a.K2 = _p(lora[0]), lora[0].stride(0), _p(lora[1]), lora[1].stride(0), lora[0].shape[1]
    rc = lib().pz_gemm_qkv_rope(C.byref(a), _st())
    if rc == PZ_ERR_UNSUPPORTED:
        return False
    if rc != 0:
        raise NativeError(f"pz_gemm_qkv_rope failed (rc={rc}): {lib().pz_last_error().decode(errors='replace')}")
    return True


def _own_kv(name, k_own, v_own, kv_group):
    """(k_own, v_own, own_bstride, kv_group) of the shared entry points: both own buffers [B, >= nk - prefix, hd] with
    one batch stride"""
    if k_own.stride(0) != v_own.stride(0):
        raise ValueError(f"{name}: k_own and v_own must have the same batch stride")
    return _p(k_own), _p(v_own), k_own.stride(0), int(kv_group)


def decode_attn(q, Lq, qoff, k, v, o, B, nh, T, nk, scale, cap, cnt, prefix, cond, qtok0, lse=None, own=None):
    """Few-query joint attention (denoise): q [B, Lq, nh*hd] rows qoff.., k/v [B, Lk, hd], o [B*T, nh*hd].
    lse (fp32 [B, T*nh], expert_attn_fwd): the same launches also write each query row's log-sum-exp.
    own (k_own, v_own, kv_group; expert_attn_fwd_shared): key rows >= prefix come from the pair's own buffers."""
    a = DecodeAttnArgs()
    a.q, a.ldq, a.Lq, a.qoff = _p(q), q.shape[-1], Lq, qoff
    a.k, a.v = _p(k), _p(v)
    a.k_bstride, a.v_bstride = k.stride(0), v.stride(0)
    a.o, a.ldo = _p(o), o.stride(0)
    a.B, a.nh, a.T, a.nk, a.head_dim = B, nh, T, nk, k.shape[-1]
    a.scale, a.cap = float(scale), float(cap)
    a.cnt, a.prefix, a.cond, a.qtok0 = _p(cnt), prefix, cond, qtok0
    need = lib().pz_decode_attn_ws_bytes(B, T * nh, nk)
    ws = workspace(o.device)  # the GEMM split-K scratch: stream-ordered, not in use between kernels
    if ws.numel() * 4 < need and lse is not None:  # training micro-batches beyond the scratch (512 x bridge: 307 MB)
        ws = torch.empty(need // 4, device=o.device, dtype=torch.float32)
    if ws.numel() * 4 < need:
        raise ValueError(f"decode_attn: {B} samples x {nk} keys need {need} B of workspace (> {ws.numel() * 4})")
    a.ws, a.ws_bytes = _p(ws), ws.numel() * 4
    if own is not None:
        call("pz_expert_attn_fwd_shared", C.byref(a), *_own_kv("expert_attn_fwd_shared", *own), _p(lse), _st())
    elif lse is not None:
        call("pz_expert_attn_fwd", C.byref(a), _p(lse), _st())
    else:
        call("pz_decode_attn", C.byref(a), _st())


def expert_attn_fwd(q, Lq, qoff, k, v, o, lse, B, nh, T, nk, scale, cap, cnt, prefix, cond, qtok0):
    """pz_expert_attn_fwd: decode_attn (the same O bits) + the fp32 log-sum-exp lse [B, T*nh] of every query row --
    the forward of the action expert's training attention against a forward-only VLM."""
    if lse is None:
        raise ValueError("expert_attn_fwd: lse is required")
    decode_attn(q, Lq, qoff, k, v, o, B, nh, T, nk, scale, cap, cnt, prefix, cond, qtok0, lse=lse)


def expert_attn_fwd_shared(q, Lq, qoff, k, v, k_own, v_own, kv_group, o, lse, B, nh, T, nk, scale, cap, cnt, prefix,
                           cond, qtok0):
    """pz_expert_attn_fwd_shared (several flow draws per observation): expert_attn_fwd over B (observation,
    draw) pairs whose key rows < prefix are rows of k / v [B / kv_group, >= prefix, hd] (the observation's VLM keys) and
    whose key rows >= prefix are rows of k_own / v_own [B, >= nk - prefix, hd] (the pair's own, compact)."""
    if lse is None:
        raise ValueError("expert_attn_fwd_shared: lse is required")
    decode_attn(q, Lq, qoff, k, v, o, B, nh, T, nk, scale, cap, cnt, prefix, cond, qtok0, lse=lse,
                own=(k_own, v_own, kv_group))


def expert_attn_bwd_shared(q, Lq, qoff, k, v, k_own, v_own, kv_group, o, lse, dO, dq, dk, dv, key0, nkeys, B, nh, T, nk,
                           scale, cap, cnt, prefix, cond, qtok0, ws=None):
    """pz_expert_attn_bwd_shared: expert_attn_bwd with expert_attn_fwd_shared's key addressing; dq / dk / dv per pair,
    the shared k / v only read."""
    expert_attn_bwd(q, Lq, qoff, k, v, o, lse, dO, dq, dk, dv, key0, nkeys, B, nh, T, nk, scale, cap, cnt, prefix, cond,
                    qtok0, ws=ws, own=(k_own, v_own, kv_group))


def expert_attn_bwd(q, Lq, qoff, k, v, o, lse, dO, dq, dk, dv, key0, nkeys, B, nh, T, nk, scale, cap, cnt, prefix, cond,
                    qtok0, ws=None, own=None):
    """pz_expert_attn_bwd: dq (addressed like q) and dk / dv [B, >= nkeys, hd] -- the rows of keys
    [key0, key0 + nkeys), e.g. views dK[:, key0:] of [B, Lp, hd] buffers, whose other rows stay untouched -- from the
    forward's q / k / v / o / lse and dO [B*T, nh*hd].  ws: fp32 scratch (default: allocated here)."""
    a = ExpertAttnBwdArgs()
    a.q, a.ldq, a.Lq, a.qoff = _p(q), q.shape[-1], Lq, qoff
    a.k, a.v = _p(k), _p(v)
    a.k_bstride, a.v_bstride = k.stride(0), v.stride(0)
    a.o, a.ldo = _p(o), o.stride(0)
    a.dO, a.lddo = _p(dO), dO.stride(0)
    a.lse = _p(lse)
    a.B, a.nh, a.T, a.nk, a.head_dim = B, nh, T, nk, k.shape[-1]
    a.scale, a.cap = float(scale), float(cap)
    a.cnt, a.prefix, a.cond, a.qtok0 = _p(cnt), prefix, cond, qtok0
    a.dq, a.dk, a.dv = _p(dq), _p(dk), _p(dv)
    a.dk_bstride, a.dv_bstride, a.key0, a.nkeys = dk.stride(0), dv.stride(0), key0, nkeys
    need = lib().pz_expert_attn_bwd_ws_bytes(B, T * nh, nk, nkeys)
    if ws is None:
        ws = torch.empty(max(need // 4, 4), device=q.device, dtype=torch.float32)
    a.ws, a.ws_bytes = _p(ws), ws.numel() * 4
    if own is not None:
        call("pz_expert_attn_bwd_shared", C.byref(a), *_own_kv("expert_attn_bwd_shared", *own), _st())
    else:
        call("pz_expert_attn_bwd", C.byref(a), _st())


def attn_softmax(S, lds, P, ldp, R, N, scale, cap=0.0, tcap=None, mask_mode=0, rows_per_batch=1, heads=1,
                 qoff=0, cnt=None, prefix=0, cond=0, mask=None, ldm=0, mask_bstride=0):
    a = SoftmaxArgs()
    a.S, a.lds, a.P, a.ldp, a.tcap = _p(S), lds, _p(P), ldp, _p(tcap)
    a.R, a.N, a.scale, a.cap, a.mask_mode = R, N, float(scale), float(cap), mask_mode
    a.rows_per_batch, a.heads, a.qoff = rows_per_batch, heads, qoff
    a.cnt, a.prefix, a.cond = _p(cnt), prefix, cond
    a.mask, a.ldm, a.mask_bstride = _p(mask), ldm, mask_bstride
    call("pz_attn_softmax", C.byref(a), _st())


def attn_softmax_bwd(P, dP, lddp, tcap, dS, ldp, R, N, scale, cap):
    call("pz_attn_softmax_bwd", _p(P), _p(dP), lddp, _p(tcap), _p(dS), ldp, R, N, float(scale), float(cap),
         _st())


def flash_args(Z, H, nq, nk, hd, q, q_strides, k, k_strides, v, v_strides, groups, o_hstride, lse, scale,
               cap=0.0, mask_mode=0, cnt=None, prefix=0, cond=0, rows_per_token=1, dgroups=None, delta=None,
               dq=None, dk=None, dv=None, mask_row0=0, key_split=False):
    """pz_flash_args (include/pz_abi.h).  *_strides = (ld, bstride, hstride) in elements; groups =
    [(row0, O tensor, bstride, ld), ...] (dgroups: the dO tensors of the same groups).  key_split:
    hand the forward the workspace so launches with few query blocks split the keys."""
    a = FlashArgs()
    a.Z, a.H, a.nq, a.nk, a.head_dim = int(Z), int(H), int(nq), int(nk), int(hd)
    a.q, (a.ldq, a.q_bstride, a.q_hstride) = _p(q), tuple(int(x) for x in q_strides)
    a.k, (a.ldk, a.k_bstride, a.k_hstride) = _p(k), tuple(int(x) for x in k_strides)
    a.v, (a.ldv, a.v_bstride, a.v_hstride) = _p(v), tuple(int(x) for x in v_strides)
    a.n_groups = len(groups)
    for i, (r0, o, bs, ld) in enumerate(groups):
        a.g_row0[i], a.g_o[i], a.g_bstride[i], a.g_ld[i] = int(r0), _p(o), int(bs), int(ld)
        if dgroups is not None:
            a.g_do[i] = _p(dgroups[i])
    a.o_hstride = int(o_hstride)
    a.lse = _p(lse)
    a.scale, a.cap, a.mask_mode = float(scale), float(cap), int(mask_mode)
    a.cnt, a.prefix, a.cond, a.rows_per_token = _p(cnt), int(prefix), int(cond), int(rows_per_token)
    a.mask_row0 = int(mask_row0)
    a.delta, a.dq, a.dk, a.dv = _p(delta), _p(dq), _p(dk), _p(dv)
    if dq is not None or key_split:  # fp32 scratch: dK/dV query-split / forward key-split partials
        ws = flash_workspace(q.device)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    return a


_FLASH_WS_BYTES = 320 << 20
_FLASH_WS = {}


def flash_workspace(device):
    """Per-device fp32 scratch of the fused attention backward (8 query splits x dK, dV of a
    64-sample micro-batch = 295 MB); allocated once, stream-ordered like the GEMM workspace."""
    dev = torch.device(device)
    ws = _FLASH_WS.get(dev)
    if ws is None:
        ws = torch.empty(_FLASH_WS_BYTES // 4, dtype=torch.float32, device=dev)
        _FLASH_WS[dev] = ws
    return ws


def flash_fwd(a):
    call("pz_flash_fwd", C.byref(a), _st())


def fp8_quant_vt(v, Z, nk, vt, vs):
    """V^T e4m3 codes vt [Z, 256, ldt] (zero past nk) and per-head-dim scales vs [Z, 256] of bf16 V [Z, rows, 256]"""
    call("pz_fp8_quant_vt", _p(v), v.stride(1), v.stride(0), Z, nk, _p(vt), _p(vs), vt.shape[2], _st())


def fp8_quant_attn(q, k, v, Z, nk, qc, qs, kc, ks, vt, vs):
    """pz_fp8_quant_attn: Q rows q [R, 256] and key rows k [Rk, 256] per row, V [Z, rows, 256] per head dim (V^T codes
    vt [Z, 256, ldt]) -- the operands of flash_fwd_f8 in one launch"""
    call("pz_fp8_quant_attn", _p(q), q.shape[0], _p(k), k.shape[0], _p(v), v.stride(1), v.stride(0), Z, nk, _p(qc),
         _p(qs), _p(kc), _p(ks), _p(vt), _p(vs), vt.shape[2], _st())


def flash_fwd_f8(a, qc, qs, kc, ks, krows, vt, vs):
    """fp8 attention forward (pz_flash_fwd_f8): shape / mask / outputs from the pz_flash_args a"""
    call("pz_flash_fwd_f8", C.byref(a), _p(qc), _p(qs), _p(kc), _p(ks), int(krows), _p(vt), _p(vs), vt.shape[2], _st())


def flash_bwd_ds(a, P, tcap, dS, ldp):
    """dS of the joint attention from the exported softmax P / tanh(cap) and dO (a.g_do groups);
    pz_flash_bwd_ds."""
    call("pz_flash_bwd_ds", C.byref(a), _p(P), _p(tcap), _p(dS), int(ldp), _st())


def flash_fwd_probs(a, P, tcap, ldp):
    """Joint fused forward that also stores the bf16 softmax P and tanh(cap) [Z, nq, ldp] (the
    GEMM-path backward's inputs); pz_flash_fwd_probs."""
    call("pz_flash_fwd_probs", C.byref(a), _p(P), _p(tcap), int(ldp), _st())


def flash_bwd(a):
    """dQ (+ delta = rowsum(dO * O)), then dK/dV (overwritten); a.delta is fp32 scratch [Z*H, nq]."""
    call("pz_flash_bwd", C.byref(a), _st())


def flash_bwd_prep(a):
    """a.delta [Z*H, nq] = rowsum(dO * O) over the output groups (a.g_o / a.g_do); pz_flash_bwd_prep."""
    call("pz_flash_bwd_prep", C.byref(a), _st())


def siglip_flash_args(qkv, O, lse, B, nh, hd, N, dO=None, delta=None, dqkv=None):
    """SigLIP attention in place on the fused q|k|v projection rows [B*N, 3*nh*hd]; O [B*N, nh*hd]."""
    W = qkv.stride(0)
    H = nh * hd
    strides = (W, N * W, hd)
    return flash_args(B, nh, N, N, hd, qkv, strides, qkv[:, H:], strides, qkv[:, 2 * H:], strides,
                      [(0, O, N * O.stride(0), O.stride(0))], hd, lse, hd ** -0.5,
                      dgroups=None if dO is None else [dO], delta=delta,
                      dq=dqkv, dk=None if dqkv is None else dqkv[:, H:], dv=None if dqkv is None else dqkv[:, 2 * H:])


def patchify(pix, cols, ps):
    B, _, H, W = pix.shape
    call("pz_patchify", _p(pix), _p(cols), B, H, W, ps, cols.stride(0), _st())


def embed_merge(ids, table, img, out, n_img, image_token, pad_token, emb_scale, img_scale):
    B, P = ids.shape
    D = table.shape[1]
    call("pz_embed_merge", _p(ids), _p(table), table.shape[0], _p(img), _p(out), B, P, D, n_img, image_token,
         pad_token,
         float(emb_scale), float(img_scale), _st())


def embed_merge_bwd(ids, dout, dimg, n_img, image_token, img_scale):
    B, P = ids.shape
    D = dout.shape[-1]
    call("pz_embed_merge_bwd", _p(ids), _p(dout), _p(dimg), B, P, D, n_img, image_token, float(img_scale),
         _st())


def time_embed(t, out, max_period, ref_bf16=False):
    B, D = out.shape
    call("pz_time_embed", _p(t), _p(out), B, D, float(max_period), int(bool(ref_bf16)), _st())


def _prefix_len(prefix_len, B):
    """the int32 [B] device tensor of per-sample prefix lengths the pz_*_prefix entry points read"""
    assert (prefix_len.dtype == torch.int32 and prefix_len.is_cuda and prefix_len.is_contiguous()
            and prefix_len.numel() == B), "prefix_len must be a contiguous int32 [B] device tensor"
    return _p(prefix_len)


def time_embed_rows(t, out, H, max_period, ref_bf16=False, prefix_len=None):
    """time embedding of sample r // H into out[r, :] (a column slice of the concat input), B * H rows; rows
    h < prefix_len[b] get the embedding of 1.0"""
    rows, D = out.shape
    if prefix_len is not None:
        call("pz_time_embed_rows_prefix", _p(t), _p(out), out.stride(0), _prefix_len(prefix_len, rows // H), rows // H,
             H, D, float(max_period), int(bool(ref_bf16)), _st())
        return
    call("pz_time_embed_rows", _p(t), _p(out), out.stride(0), rows // H, H, D, float(max_period), int(bool(ref_bf16)),
         _st())


def concat_time(temb, e1, out, B, H, D, prefix_len=None, max_period=None, ref_bf16=False):
    """out[b*H+h] = [temb[b] | e1[b*H+h]]; with ``prefix_len`` (and the embedding's ``max_period`` / mode) the time
    columns of rows h < prefix_len[b] are the embedding of 1.0"""
    if prefix_len is not None:
        call("pz_concat_time_prefix", _p(temb), _p(e1), _p(out), _prefix_len(prefix_len, B), B, H, D,
             float(max_period), int(bool(ref_bf16)), _st())
        return
    call("pz_concat_time", _p(temb), _p(e1), _p(out), B, H, D, _st())


def split_time_grad(dcat, de1, rows, D):
    call("pz_split_time_grad", _p(dcat), _p(de1), rows, D, _st())


def flow_psi(x0, x1, t, psi, sig_min, prefix_len=None):
    """psi = bf16((1 - (1 - sig) t) x0 + t x1) for x0, x1 fp32 [B, H, A]; rows h < prefix_len[b] get bf16(x1)"""
    B = x0.shape[0]
    if prefix_len is not None:
        assert x0.dim() == 3, "flow_psi with a prefix needs [B, H, A] inputs"
        call("pz_flow_psi_prefix", _p(x0), _p(x1), _p(t), _prefix_len(prefix_len, B), _p(psi), B, x0.shape[1],
             x0.shape[2], float(sig_min), _st())
        return
    call("pz_flow_psi", _p(x0), _p(x1), _p(t), _p(psi), B, x0[0].numel(), float(sig_min), _st())


def flow_loss(v, ldv, vbs, x0, x1, loss, dv, grad_scale, B, H, A, sig_min, prefix_len=None):
    """mean squared flow error (and its gradient dv); with ``prefix_len`` over the rows h >= prefix_len[b] only, the
    element count taken from prefix_len on the device"""
    if prefix_len is not None:
        call("pz_flow_loss_prefix", _p(v), ldv, vbs, _p(x0), _p(x1), _prefix_len(prefix_len, B), _p(loss), _p(dv),
             _p(grad_scale), B, H, A, float(sig_min), _st())
        return
    call("pz_flow_loss", _p(v), ldv, vbs, _p(x0), _p(x1), _p(loss), _p(dv), _p(grad_scale), B, H, A,
         float(sig_min), _st())


def action_in(action, W1, b1, t, cat, B, H, D, max_period, ref_bf16=False, prefix_len=None):
    """cat[:, :D] = time embedding, cat[:, D:2D] = bf16(action) @ W1^T + b1 (one launch; inference); rows
    h < prefix_len[b] get the embedding of 1.0"""
    A = action.shape[-1]
    if prefix_len is not None:
        call("pz_action_in_prefix", _p(action), A, _p(W1), _p(b1), _p(t), _p(cat), cat.stride(0),
             _prefix_len(prefix_len, B), B, H, D, float(max_period), int(bool(ref_bf16)), _st())
        return
    call("pz_action_in", _p(action), A, _p(W1), _p(b1), _p(t), _p(cat), cat.stride(0), B, H, D, float(max_period),
         int(bool(ref_bf16)), _st())


def action_out(x, norm_w, eps, Wd, bd, action, t, B, H, dt, prefix_len=None):
    """action += dt * (RMSNorm(x) @ Wd^T + bd) (bf16 v), t += dt: the denoise step's tail in one launch; rows
    h < prefix_len[b] of action are left as they are (t advances all the same)"""
    D = x.shape[1]
    if prefix_len is not None:
        call("pz_action_out_prefix", _p(x), x.stride(0), _p(norm_w), float(eps), _p(Wd), _p(bd), D, Wd.shape[0],
             _p(action), _p(t), _prefix_len(prefix_len, B), B, H, float(dt), _st())
        return
    call("pz_action_out", _p(x), x.stride(0), _p(norm_w), float(eps), _p(Wd), _p(bd), D, Wd.shape[0], _p(action),
         _p(t), B, H, float(dt), _st())


def euler_step(action, v, ldv, vbs, t, B, H, A, dt, prefix_len=None):
    if prefix_len is not None:
        call("pz_euler_step_prefix", _p(action), _p(v), ldv, vbs, _p(t), _prefix_len(prefix_len, B), B, H, A,
             float(dt), _st())
        return
    call("pz_euler_step", _p(action), _p(v), ldv, vbs, _p(t), B, H, A, float(dt), _st())


def _f32c(name, x, shape):
    assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and tuple(x.shape) == tuple(shape), (
        f"{name} must be a contiguous fp32 device tensor of shape {tuple(shape)}")
    return _p(x)


def rtc_seed(action, v, ldv, vbs, target, w, t, e, dv, T, row0):
    """e = w * (target - (action + (1 - t) * v)) (fp32 [B, H, A]) and the backward seed dv [B*T, 8] bf16: bf16(e) in
    rows row0 .. row0 + H of every sample's T rows, columns < A; zero everywhere else.  v bf16 addressed
    as euler_step's."""
    B, H, A = action.shape
    assert dv.dtype == BF16 and dv.is_contiguous() and tuple(dv.shape) == (B * T, 8), "dv must be bf16 [B*T, 8]"
    call("pz_rtc_seed", _f32c("action", action, (B, H, A)), _p(v), ldv, vbs, _f32c("target", target, (B, H, A)),
         _f32c("w", w, (B, H)), _f32c("t", t, (B,)), _f32c("e", e, (B, H, A)), _p(dv), T, row0, B, H, A, _st())


def rtc_euler(action, v, ldv, vbs, e, dA, t, coef, k, dt):
    """g = e + (1 - t) * dA; action += dt * (v + coef[k] * g); t += dt once per sample.  dA bf16 [B*H, >= A]
    (row-strided), coef fp32 [steps] on the device."""
    B, H, A = action.shape
    assert dA.dtype == BF16 and dA.shape[0] == B * H and dA.shape[1] >= A and dA.stride(1) == 1
    assert coef.dtype == torch.float32 and coef.is_cuda and coef.is_contiguous() and coef.dim() == 1
    call("pz_rtc_euler", _f32c("action", action, (B, H, A)), _p(v), ldv, vbs, _f32c("e", e, (B, H, A)), _p(dA),
         dA.stride(0), _f32c("t", t, (B,)), _p(coef), coef.numel(), int(k), B, H, A, float(dt), _st())


def action_prefix_init(action, prefix, prefix_len):
    """action[b, h, :] = prefix[b, h, :] for h < prefix_len[b] (fp32 [B, H, A], in place; other rows untouched)"""
    B, H, A = action.shape
    assert action.dtype == prefix.dtype == torch.float32 and action.is_contiguous() and prefix.is_contiguous()
    assert prefix.shape == action.shape and prefix.device == action.device
    call("pz_action_prefix_init", _p(action), _p(prefix), _prefix_len(prefix_len, B), B, H, A, _st())


def copy_rows(src, sld, sbs, dst, dld, dbs, B, rows, D, scale=1.0, beta=False):
    call("pz_copy_rows", _p(src), sld, sbs, _p(dst), dld, dbs, B, rows, D, float(scale), int(beta), _st())


def clamp_(x, lo, hi, prefix_len=None):
    """in-place clamp of fp32 x; with ``prefix_len`` x is [B, H, A] and rows h < prefix_len[b] are exempt"""
    if prefix_len is not None:
        B, H, A = x.shape
        assert x.is_contiguous()
        call("pz_clamp_prefix", _p(x), _prefix_len(prefix_len, B), B, H, A, float(lo), float(hi), _st())
        return
    call("pz_clamp", _p(x), x.numel(), float(lo), float(hi), _st())


def geglu_bwd(dh, gu, dgu, h_out, M, I):
    call("pz_geglu_bwd", _p(dh), dh.stride(0), _p(gu), gu.stride(0), _p(dgu), _p(h_out),
         0 if h_out is None else h_out.stride(0), M, I, _st())


def act_bwd(dh, pre, dpre, h_out, act):
    M, N = pre.shape
    call("pz_act_bwd", _p(dh), dh.stride(0), _p(pre), pre.stride(0), _p(dpre), _p(h_out),
         0 if h_out is None else h_out.stride(0), M, N, int(act), _st())


def adamw(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, gscale=None):
    call("pz_adamw", _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(b1), float(b2), float(eps),
         float(wd), float(bc1), float(bc2), _p(gscale), _st())


ROUND_COMPENSATED, ROUND_STOCHASTIC = 1, 2  # pz_adamw8bit_r / pz_adamw_r modes (include/pz_abi.h)


def splitmix64(z):
    """The kernels' counter-based hash (csrc/pz_common.h) on the host: the stochastic-rounding key of a step."""
    m = 2 ** 64 - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def adamw_r(p, comp, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, gscale=None, *, mode, rng_key=0, rng_base=0):
    """``adamw`` with a compensated (mode 1: ``comp`` is the bf16 compensation buffer, laid out like ``p``) or
    stochastic (mode 2: draws from ``rng_key`` and the arena index ``rng_base`` of p[0]) weight store."""
    call("pz_adamw_r", _p(p), _p(comp), _p(g), _p(m), _p(v), p.numel(), float(lr), float(b1), float(b2), float(eps),
         float(wd), float(bc1), float(bc2), _p(gscale), int(mode), C.c_uint64(int(rng_key) & (2 ** 64 - 1)),
         int(rng_base), _st())


def _adamw8_args(run, g, qmap1, qmap2, lr, b1, b2, eps, wd, t, gscale):
    """pz_adamw8_args of one run.  Host precomputes the float32 constants exactly as oracle/adamw8bit.py does."""
    import numpy as np

    f = np.float32
    c1 = f(1.0 - b1 ** t)
    c2 = f(np.sqrt(1.0 - b2 ** t))
    a = AdamW8Args()
    a.p, a.g = _p(run["flat"]), _p(g)
    a.s1, a.s2 = _p(run["s1"]), _p(run["s2"])
    a.absmax1, a.absmax2 = _p(run["absmax1"]), _p(run["absmax2"])
    a.m32, a.v32 = _p(run["m32"]), _p(run["v32"])
    a.seg, a.nseg, a.nblocks = _p(run["seg"]), run["nseg"], run["nblocks"]
    a.qmap1, a.qmap2 = _p(qmap1), _p(qmap2)
    a.beta1, a.beta2 = float(f(b1)), float(f(b2))
    a.omb1, a.omb2 = float(f(1.0 - b1)), float(f(1.0 - b2))
    a.step = float(f(f(-lr) * c2 / c1))
    a.epsc = float(f(f(eps) * c2))
    a.decay = float(f(1.0 - lr * wd)) if wd > 0 else 1.0
    a.gscale = _p(gscale)
    return a


def adamw8bit(run, g, qmap1, qmap2, lr, b1, b2, eps, wd, t, gscale=None):
    """One bnb-style 8-bit AdamW step over a contiguous run (optim.FusedAdamW._prepare_8bit layout)."""
    a = _adamw8_args(run, g, qmap1, qmap2, lr, b1, b2, eps, wd, t, gscale)
    call("pz_adamw8bit", C.byref(a), _st())


def adamw8bit_r(run, g, qmap1, qmap2, lr, b1, b2, eps, wd, t, gscale=None, *, comp=None, mode, rng_key=0,
                rng_base=0):
    """``adamw8bit`` with a compensated (mode 1, ``comp``) or stochastic (mode 2, ``rng_key`` / ``rng_base``) weight
    store: same update, same state."""
    a = _adamw8_args(run, g, qmap1, qmap2, lr, b1, b2, eps, wd, t, gscale)
    call("pz_adamw8bit_r", C.byref(a), _p(comp), int(mode), C.c_uint64(int(rng_key) & (2 ** 64 - 1)), int(rng_base),
         _st())


def sumsq(g, parts):
    """writes PZ_SUMSQ_PARTS fp32 partial sums of g*g into parts[0:PZ_SUMSQ_PARTS]"""
    assert parts.dtype == torch.float32 and parts.numel() >= PZ_SUMSQ_PARTS
    call("pz_sumsq", _p(g), g.numel(), _p(parts), _st())


def clip_coef(parts, coef, norm_out, max_norm):
    """norm = sqrt(sum(parts)) (fixed order), coef = min(1, max_norm / (norm + 1e-6))"""
    call("pz_clip_coef", _p(parts), parts.numel(), _p(coef), _p(norm_out), float(max_norm), _st())


def fill_uniform(x, seed, off, scale):
    call("pz_fill_uniform", _p(x), int(x.dtype == torch.float32), x.numel(), C.c_uint64(seed & (2**64 - 1)),
         float(off), float(scale), _st())
    return x


def cast_to_bf16(x, y):
    call("pz_cast_f32_bf16", _p(x), _p(y), x.numel(), _st())


def avg_lerp(avg, p, w):
    """avg <- torch.lerp(avg, p, w) over two flat contiguous bf16 tensors of equal length, in place, bit-identical
    to torch's bf16 lerp (weight averaging: averaging.FlatAverage)."""
    assert avg.dtype == BF16 and p.dtype == BF16 and avg.numel() == p.numel()
    assert avg.is_contiguous() and p.is_contiguous()
    call("pz_avg_lerp", _p(avg), _p(p), avg.numel(), float(w), _st())


def avg_swap(a, b):
    """exchange the contents of two flat contiguous bf16 tensors of equal length, in place"""
    assert a.dtype == BF16 and b.dtype == BF16 and a.numel() == b.numel()
    assert a.is_contiguous() and b.is_contiguous()
    call("pz_avg_swap", _p(a), _p(b), a.numel(), _st())


# ---- observation front end / action back end (csrc/pz_obs.hip) ----------------------------------------
NORM_MODES = {"bound": PZ_OBS_NORM_BOUND, "gaussian": PZ_OBS_NORM_GAUSSIAN}
_TAPS = {}  # (n_in, n_out, device) -> (first int32 [n_out], count int32 [n_out], weights fp32 [n_out, T], T)
_CODE_LUT = {}  # device -> bf16 [256]


def lanczos3_taps(n_in, n_out):
    """Tap table of one axis of tf.image.resize(method="lanczos3", antialias=True), n_in -> n_out, in fp64 numpy:
    (first int32 [n_out], count int32 [n_out], weights fp64 [n_out, T]).  Output i is centred on c = (i + 0.5) scale
    (scale = n_in / n_out), the kernel is stretched by ks = max(scale, 1) (the antialias), its taps are the input
    indices [floor(c - 3 ks + 0.5), floor(c + 3 ks + 0.5)) clipped to [0, n_in), weighted by L3((x + 0.5 - c) / ks),
    L3(t) = sinc(t) sinc(t / 3) on |t| < 3, and normalised to sum 1.  Columns past an output's count are zero."""
    import numpy as np

    if int(n_in) != n_in or int(n_out) != n_out or n_in < 1 or n_out < 1:
        raise ValueError(f"lanczos3_taps: sizes must be positive integers, got {n_in} -> {n_out}")
    n_in, n_out = int(n_in), int(n_out)
    if max(n_in, n_out) > PZ_OBS_MAX_EXTENT:
        raise ValueError(f"lanczos3_taps: {n_in} -> {n_out} exceeds the extent limit PZ_OBS_MAX_EXTENT = "
                         f"{PZ_OBS_MAX_EXTENT}")
    scale = n_in / n_out
    ks = max(scale, 1.0)
    c = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.floor(c - 3.0 * ks + 0.5), 0).astype(np.int64)
    hi = np.minimum(np.floor(c + 3.0 * ks + 0.5), n_in).astype(np.int64)
    count = hi - lo
    T = int(count.max())
    if T > PZ_OBS_MAX_TAPS:
        raise ValueError(f"lanczos3_taps: {n_in} -> {n_out} needs {T} taps per output, above the kernel's limit "
                         f"PZ_OBS_MAX_TAPS = {PZ_OBS_MAX_TAPS} (a downscale of up to {(PZ_OBS_MAX_TAPS - 2) // 6}x)")
    x = lo[:, None] + np.arange(T)[None, :]
    t = (x + 0.5 - c[:, None]) / ks
    w = np.where((np.abs(t) < 3.0) & (x < hi[:, None]), np.sinc(t) * np.sinc(t / 3.0), 0.0)
    w = w / w.sum(axis=1, keepdims=True)
    return lo.astype(np.int32), count.astype(np.int32), w


def _device_taps(n_in, n_out, dev):
    key = (int(n_in), int(n_out), dev)
    t = _TAPS.get(key)
    if t is None:
        first, count, w = lanczos3_taps(n_in, n_out)
        t = _TAPS[key] = (torch.from_numpy(first).to(dev), torch.from_numpy(count).to(dev),
                          torch.from_numpy(w).to(torch.float32).contiguous().to(dev), w.shape[1])
    return t


def pixel_code_lut(dev):
    """bf16 [256]: the model's pixel normalisation of each uint8 code, ((q / 255 - 0.5) / 0.5).to(bf16)
    (vla/processing.py:109-114), evaluated by torch ON THE HOST and uploaded -- the bits a host-normalised frame
    carries into EvalAgent.infer_chunk.  (Evaluated on the device the same expression differs in a few codes around
    127 by one bf16 ulp: there torch divides by a scalar as a multiplication by its reciprocal, and q / 255 - 0.5
    cancels.)"""
    dev = torch.device(dev)
    lut = _CODE_LUT.get(dev)
    if lut is None:
        q = torch.arange(256, dtype=torch.int32).to(torch.uint8)
        lut = _CODE_LUT[dev] = ((q.to(torch.float32) / 255.0 - 0.5) / 0.5).to(BF16).contiguous().to(dev)
    return lut


def image_resize_scratch_numel(n, h_in, S):
    """fp32 elements of the scratch between the two passes of image_resize_norm"""
    return lib().pz_image_resize_scratch_bytes(int(n), int(h_in), int(S)) // 4


def image_resize_norm(frames, S, channels_last=True, out=None, scratch=None):
    """uint8 frames [n, H, W, 3] (channels_last) or [n, 3, H, W] -> bf16 [n, 3, S, S]: Lanczos-3 resize with
    antialiasing (tf.image.resize semantics, lanczos3_taps), rounded half-to-even to a uint8 code and stored in the
    model's pixel normalisation (pixel_code_lut).  The tap tables and the code table are built on first use of a
    geometry / device and cached (so: before a graph capture); ``scratch`` (fp32, image_resize_scratch_numel) and
    ``out`` are allocated from the current allocator when not given."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.is_contiguous() and frames.is_cuda
    n = frames.shape[0]
    if channels_last:
        H, W, ch = frames.shape[1:]
    else:
        ch, H, W = frames.shape[1:]
    if ch != 3:
        raise ValueError(f"image_resize_norm: frames must have 3 channels, got shape {tuple(frames.shape)}")
    dev = frames.device
    hf, hc, hw, ht = _device_taps(W, S, dev)
    vf, vc, vw, vt = _device_taps(H, S, dev)
    lut = pixel_code_lut(dev)
    need = image_resize_scratch_numel(n, H, S)
    if scratch is None:
        scratch = torch.empty(need, device=dev, dtype=torch.float32)
    assert scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= need
    if out is None:
        out = torch.empty(n, 3, S, S, device=dev, dtype=BF16)
    assert out.dtype == BF16 and out.is_contiguous() and tuple(out.shape) == (n, 3, S, S)
    call("pz_image_resize_norm", _p(frames), int(bool(channels_last)), n, H, W, S, _p(hf), _p(hc), _p(hw), ht,
         _p(vf), _p(vc), _p(vw), vt, _p(lut), _p(scratch), scratch.numel() * 4, _p(out), _st())
    return out


def image_resize_u8(frames, S, channels_last=True, out=None, scratch=None):
    """image_resize_norm's resize (same kernels, same rounding) with the uint8 code stored instead of its table
    value: uint8 frames [n, H, W, 3] (channels_last) or [n, 3, H, W] -> uint8 [n, 3, S, S], the input of
    image_augment for frames that are not at the model's size (resize first, augment after: DESIGN 7e)."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.is_contiguous() and frames.is_cuda
    n = frames.shape[0]
    if channels_last:
        H, W, ch = frames.shape[1:]
    else:
        ch, H, W = frames.shape[1:]
    if ch != 3:
        raise ValueError(f"image_resize_u8: frames must have 3 channels, got shape {tuple(frames.shape)}")
    dev = frames.device
    hf, hc, hw, ht = _device_taps(W, S, dev)
    vf, vc, vw, vt = _device_taps(H, S, dev)
    need = image_resize_scratch_numel(n, H, S)
    if scratch is None:
        scratch = torch.empty(need, device=dev, dtype=torch.float32)
    assert scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= need
    if out is None:
        out = torch.empty(n, 3, S, S, device=dev, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (n, 3, S, S)
    call("pz_image_resize_u8", _p(frames), int(bool(channels_last)), n, H, W, S, _p(hf), _p(hc), _p(hw), ht,
         _p(vf), _p(vc), _p(vw), vt, _p(scratch), scratch.numel() * 4, _p(out), _st())
    return out


# ---- training-image augmentation (csrc/pz_augment.hip) -------------------------------------------------
def image_augment_scratch_numel(n, S):
    """fp32 elements of image_augment's scratch (the partial sums of the contrast's channel means)"""
    return lib().pz_image_augment_scratch_bytes(int(n), int(S)) // 4


def image_augment(frames, params, mask, channels_last=False, out=None, scratch=None):
    """uint8 frames [n, 3, S, S] (or [n, S, S, 3] with channels_last) -> bf16 [n, 3, S, S]: crop, brightness,
    contrast, saturation, hue in that order on q / 255 (the TF ops' semantics), requantised with
    floor(255.5 x) and stored in the model's pixel normalisation (pixel_code_lut).

    ``params`` float32 [n, 8] = box (y1, x1, y2, x2), brightness delta, contrast factor, saturation factor, hue
    delta; ``mask`` int32 [n], the PZ_AUG_* ops each frame gets (pizero_native.augment.draw_params makes both).
    Host arrays (numpy / CPU tensors) are uploaded here, and the launch that sums the channel means is skipped when
    no frame's mask has the contrast; with device tensors nothing is read back, and that launch always runs."""
    import numpy as np

    from ._lib import PZ_AUG_ALL

    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.is_contiguous() and frames.is_cuda
    n = frames.shape[0]
    S = frames.shape[2]
    shape = (n, S, S, 3) if channels_last else (n, 3, S, S)
    if tuple(frames.shape) != shape:
        want = "[n, S, S, 3]" if channels_last else "[n, 3, S, S]"
        raise ValueError(f"image_augment: frames must be square with 3 channels, {want}; got shape "
                         f"{tuple(frames.shape)} (resize first: image_resize_u8)")
    dev = frames.device
    if isinstance(params, np.ndarray):
        params = torch.from_numpy(np.ascontiguousarray(params))
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    if params.dtype != torch.float32 or tuple(params.shape) != (n, 8):
        raise ValueError(f"image_augment: params must be float32 [{n}, 8], got {params.dtype} {tuple(params.shape)}")
    if mask.dtype != torch.int32 or tuple(mask.shape) != (n,):
        raise ValueError(f"image_augment: mask must be int32 [{n}], got {mask.dtype} {tuple(mask.shape)}")
    if mask.is_cuda:
        union = PZ_AUG_ALL
    else:
        union = int(np.bitwise_or.reduce(mask.numpy())) if n else 0
        if union & ~PZ_AUG_ALL:
            raise ValueError(f"image_augment: mask has bits outside PZ_AUG_ALL = {PZ_AUG_ALL}")
    params = params.to(dev).contiguous()
    mask = mask.to(dev).contiguous()
    lut = pixel_code_lut(dev)
    need = image_augment_scratch_numel(n, S)
    if scratch is None:
        scratch = torch.empty(need, device=dev, dtype=torch.float32)
    assert scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= need
    if out is None:
        out = torch.empty(n, 3, S, S, device=dev, dtype=BF16)
    assert out.dtype == BF16 and out.is_contiguous() and tuple(out.shape) == (n, 3, S, S)
    call("pz_image_augment", _p(frames), int(bool(channels_last)), n, S, _p(params), _p(mask), union, _p(lut),
         _p(scratch), scratch.numel() * 4, _p(out), _st())
    return out


def _norm_args(x, out, a, b, mode):
    assert x.dtype == torch.float32 and x.is_contiguous() and x.is_cuda
    D = x.shape[-1]
    for s in (a, b):
        assert s.dtype == torch.float32 and s.is_contiguous() and s.numel() == D and s.device == x.device
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape
    if mode not in NORM_MODES:
        raise ValueError(f"normalisation type must be one of {sorted(NORM_MODES)}, got {mode!r}")
    return out, x.numel() // D, D, NORM_MODES[mode]


def proprio_normalize(x, a, b, mode, out=None):
    """fp32 [..., D] raw proprio -> normalised (env_adapter/base.py): mode "bound" with a = p01, b = p99 gives
    clip(2 (x - a) / (b - a + 1e-8) - 1, -1, 1); "gaussian" with a = mean, b = std gives (x - a) / (b + 1e-8)."""
    out, rows, D, m = _norm_args(x, out, a, b, mode)
    call("pz_proprio_normalize", _p(x), _p(out), rows, D, _p(a), _p(b), m, _st())
    return out


def action_denormalize(x, a, b, mode, n_pass=1, out=None, prev=None, prefix_len=None):
    """fp32 [..., D] normalised actions -> robot units: "bound" (x + 1) / 2 (b - a) + a, "gaussian" x (b + 1e-8) + a;
    the trailing ``n_pass`` dimensions (the gripper, simpler.py:105-126) are copied unchanged.  With ``prev`` (robot
    units, x's shape [B, H, D]) and ``prefix_len``, rows h < prefix_len[b] of the result are prev's bits."""
    out, rows, D, m = _norm_args(x, out, a, b, mode)
    if prefix_len is not None:
        assert x.dim() == 3 and prev is not None and prev.shape == x.shape and prev.dtype == torch.float32
        assert prev.is_contiguous() and prev.device == x.device
        B, H = x.shape[:2]
        call("pz_action_denormalize_prefix", _p(x), _p(out), _p(prev), _prefix_len(prefix_len, B), B, H, D,
             int(n_pass), _p(a), _p(b), m, _st())
        return out
    call("pz_action_denormalize", _p(x), _p(out), rows, D, int(n_pass), _p(a), _p(b), m, _st())
    return out


def action_normalize(x, a, b, mode, n_pass=1, out=None):
    """the inverse of action_denormalize: fp32 [..., D] robot-unit actions -> the model's normalised actions ("bound":
    clip(2 (x - a) / (b - a + 1e-8) - 1, -1, 1), "gaussian": (x - a) / (b + 1e-8)); the trailing ``n_pass``
    dimensions are copied unchanged."""
    out, rows, D, m = _norm_args(x, out, a, b, mode)
    call("pz_action_normalize", _p(x), _p(out), rows, D, int(n_pass), _p(a), _p(b), m, _st())
    return out


# ---- micro-batch assembly from an episode store (csrc/pz_episodes.hip) ----------------------------------
def _episode_idx(who, idx, n_rows):
    """the host's check of the sample rows: int64 numpy [B], every row in [0, n_rows) -- before anything is uploaded"""
    import numpy as np

    if not isinstance(idx, np.ndarray) or idx.dtype != np.int64 or idx.ndim != 1 or idx.size < 1:
        raise ValueError(f"{who}: idx must be a non-empty one-dimensional int64 numpy array on the host, got "
                         f"{type(idx).__name__} {getattr(idx, 'dtype', '')} {getattr(idx, 'shape', '')}")
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= n_rows:
        raise ValueError(f"{who}: idx must lie in [0, {n_rows}), got values from {lo} to {hi}")
    return np.ascontiguousarray(idx)


def _episode_tensor(who, name, t, dtype, shape=None, ndim=None):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor, got "
                         f"{getattr(t, 'dtype', type(t).__name__)}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{who}: {name} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")


def _episode_on_device(who, dev, **tensors):
    for name, t in tensors.items():
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{who}: {name} must be in the memory of {dev}, it is on {t.device}")


def episode_gather_frames(store, idx=None, out=None):
    """uint8 store [N, C, H, W, 3] in device memory, frame rows ``idx`` (int64 numpy [B] on the host, checked against
    [0, N) here, before anything is uploaded or launched) -> uint8 [B * C, 3, H, W]: frame b * C + c is camera c of row
    idx[b], channels first, as image_resize_* / image_augment / TrainAgent.preprocess_batch take it.  ``idx=None`` is
    the identity: the store is a [B, C, H, W, 3] staging buffer that is already gathered."""
    who = "episode_gather_frames"
    _episode_tensor(who, "store", store, torch.uint8, ndim=5)
    N, Cn, H, W, ch = store.shape
    if ch != 3 or N < 1 or Cn < 1 or H < 1 or W < 1:
        raise ValueError(f"{who}: store must be [N, C, H, W, 3] with positive sizes, got {tuple(store.shape)}")
    if idx is None:
        B, host_idx = N, None
    else:
        host_idx = _episode_idx(who, idx, N)
        B = host_idx.size
    if out is not None:
        _episode_tensor(who, "out", out, torch.uint8, shape=(B * Cn, 3, H, W))
    _episode_on_device(who, store.device, store=store, **({"out": out} if out is not None else {}))
    if out is None:
        out = torch.empty(B * Cn, 3, H, W, device=store.device, dtype=torch.uint8)
    dev_idx = None if host_idx is None else torch.from_numpy(host_idx).to(store.device)
    call("pz_episode_gather_frames", _p(store), N, Cn, H, W, _p(dev_idx), B, _p(out), _st())
    return out


def episode_gather_rows(action, proprio, episode_of, episode_offsets, tokens, idx, window, horizon, pad_id, out=None):
    """One launch for everything of a micro-batch but its frames.  Device tensors: ``action`` fp32 [N, A] and
    ``proprio`` fp32 [N, P] (already normalised: the kernel gathers only), ``episode_of`` int32 [N], ``episode_offsets``
    int64 [E + 1], ``tokens`` int32 [E, L]; ``idx`` int64 numpy [B] on the host (checked against [0, N) here).  Returns
    {"action": fp32 [B, horizon, A], "proprio": fp32 [B, window, P], "action_pad_mask": uint8 [B, horizon],
    "input_ids": int64 [B, L], "attention_mask": int64 [B, L]}: sample b is step t = idx[b] of its episode [s, e): action
    rows min(t + h, e - 1), proprio rows max(t - window + 1 + w, s), pad mask t + h <= e - 1, the episode's tokens and
    ids != pad_id.  ``out`` may hold preallocated tensors under those names (exact shapes)."""
    who = "episode_gather_rows"
    _episode_tensor(who, "action", action, torch.float32, ndim=2)
    _episode_tensor(who, "proprio", proprio, torch.float32, ndim=2)
    N, A = action.shape
    P = proprio.shape[1]
    _episode_tensor(who, "proprio", proprio, torch.float32, shape=(N, P))
    _episode_tensor(who, "episode_of", episode_of, torch.int32, shape=(N,))
    _episode_tensor(who, "episode_offsets", episode_offsets, torch.int64, ndim=1)
    _episode_tensor(who, "tokens", tokens, torch.int32, ndim=2)
    E, L = tokens.shape
    if episode_offsets.numel() != E + 1 or E < 1 or N < 1 or A < 1 or P < 1 or L < 1:
        raise ValueError(f"{who}: episode_offsets must have E + 1 = {E + 1} entries and every size be positive, got "
                         f"{episode_offsets.numel()} offsets, N {N}, A {A}, P {P}, L {L}")
    Wn, Hn = int(window), int(horizon)
    if Wn < 1 or Hn < 1:
        raise ValueError(f"{who}: window and horizon must be positive, got {window}, {horizon}")
    host_idx = _episode_idx(who, idx, N)
    B = host_idx.size
    shapes = {"action": ((B, Hn, A), torch.float32), "proprio": ((B, Wn, P), torch.float32),
              "action_pad_mask": ((B, Hn), torch.uint8), "input_ids": ((B, L), torch.int64),
              "attention_mask": ((B, L), torch.int64)}
    dev = action.device
    if out is not None:
        if set(out) != set(shapes):
            raise ValueError(f"{who}: out must hold exactly {sorted(shapes)}, got {sorted(out)}")
        for k, (shape, dt) in shapes.items():
            _episode_tensor(who, f"out[{k!r}]", out[k], dt, shape=shape)
    _episode_on_device(who, dev, action=action, proprio=proprio, episode_of=episode_of,
                       episode_offsets=episode_offsets, tokens=tokens,
                       **({f"out_{k}": v for k, v in out.items()} if out is not None else {}))
    if out is None:
        out = {k: torch.empty(shape, device=dev, dtype=dt) for k, (shape, dt) in shapes.items()}
    dev_idx = torch.from_numpy(host_idx).to(dev)
    call("pz_episode_gather_rows", _p(action), _p(proprio), _p(episode_of), _p(episode_offsets), _p(tokens),
         _p(dev_idx), N, E, A, P, L, B, Wn, Hn, int(pad_id), _p(out["action"]), _p(out["proprio"]),
         _p(out["action_pad_mask"]), _p(out["input_ids"]), _p(out["attention_mask"]), _st())
    return out


# ---- 4-bit base weights of QLoRA (csrc/pz_q4.hip) --------------------------------------------------------
Q4_TABLES = {"fp4": 0, "nf4": 1}  # include/pz_abi.h PZ_Q4_FP4 / PZ_Q4_NF4


def _q4_table(qtype):
    if qtype not in Q4_TABLES:
        raise ValueError(f"quantize_type must be fp4 or nf4, got {qtype!r}")
    return Q4_TABLES[qtype]


def q4_quantize(w, packed, absmax, qtype="fp4"):
    """packed uint8 [n / 2] (the even element in the high nibble) and the fp32 absmax of every block of 64 of the
    flat bf16 tensor ``w`` (n = w.numel(), even: an odd n is refused before any launch)."""
    n = w.numel()
    assert w.dtype == BF16 and w.is_cuda and w.is_contiguous(), "w must be a contiguous bf16 device tensor"
    assert packed.dtype == torch.uint8 and packed.is_contiguous() and packed.numel() >= n // 2
    assert absmax.dtype == torch.float32 and absmax.is_contiguous() and absmax.numel() >= (n + 63) // 64
    call("pz_q4_quantize", _p(w), _p(packed), _p(absmax), n, _q4_table(qtype), _st())


def q4_dequant(segs, qmap, qtype="fp4"):
    """dst[:n] = the bf16 weights of every (packed, absmax_codes, nested_absmax, offset, n, dst) of ``segs`` (1 to
    PZ_Q4_MAX_SEGS weights, one launch); qmap: the fp32 [256] dynamic map on the device."""
    assert 1 <= len(segs) <= PZ_Q4_MAX_SEGS, f"1..{PZ_Q4_MAX_SEGS} segments per launch"
    assert qmap.dtype == torch.float32 and qmap.is_cuda and qmap.is_contiguous() and qmap.numel() == 256
    arr = (Q4Seg * len(segs))()
    for a, (packed, codes, nam, offset, n, dst) in zip(arr, segs):
        assert packed.dtype == torch.uint8 and packed.is_contiguous() and packed.numel() >= n // 2
        assert codes.dtype == torch.uint8 and codes.is_contiguous() and codes.numel() >= (n + 63) // 64
        assert nam.dtype == torch.float32 and nam.is_contiguous() and nam.numel() >= ((n + 63) // 64 + 255) // 256
        assert dst.dtype == BF16 and dst.is_contiguous() and dst.numel() >= n
        a.packed, a.absmax_codes, a.nested_absmax, a.dst, a.n, a.offset = (_p(packed), _p(codes), _p(nam), _p(dst),
                                                                           int(n), float(offset))
    call("pz_q4_dequant_multi", C.cast(arr, C.c_void_p), len(segs), _p(qmap), _q4_table(qtype), _st())


def debug_poison_lds(word=0xFFFFFFFF):
    """Test instrument: fill every CU's LDS with ``word`` (0xffffffff = NaN) on the current stream."""
    call("pz_debug_poison_lds", C.c_uint32(int(word) & 0xFFFFFFFF), _st())


def debug_spin(wgs, ticks):
    """Test instrument: ``wgs`` workgroups each holding a CU for ``ticks`` wall-clock ticks, on the current stream."""
    call("pz_debug_spin", int(wgs), int(ticks), _st())
