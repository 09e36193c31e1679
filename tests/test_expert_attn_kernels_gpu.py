"""pz_expert_attn_fwd / pz_expert_attn_bwd (csrc/pz_expert_attn.hip): the action expert's training attention against
cached VLM keys, against the float64 reference of tests/flash_ref.py taken on query rows [P, L).

Inputs are bf16 (upcast for the reference); nh 8, hd 256, cap 50, scale 1/16.  K / V rows [L, Lp) hold NaN and every
output is pre-filled with NaN, so a read past nk or an unwritten element shows; dk / dv are [B, Lp, hd] buffers with a
sentinel outside rows [P, P + T) that must survive.  q / dq are passed compact ([B, T, nh*hd]) and as rows P.. of
[B, L, nh*hd] (qoff = P).  Every launch runs twice and is compared bit for bit (no atomics, fixed-order merges).

Tolerances are the project's own for the same quantities (tests/test_flash_shapes_gpu.py): O rtol = atol = 2e-2,
lse rtol 1e-3 / atol 2e-3, dQ rtol 2e-2 / atol 3e-2 max|ref| / 4, dK and dV rtol 2e-2 / atol 3e-2 max|ref|.
"""

import functools

import pytest
import torch

from tests.flash_ref import attention, attention_grads, block_mask

pytestmark = pytest.mark.gpu

NH, HD, CAP, SCALE = 8, 256, 50.0, 1.0 / 16.0
SENTINEL = 1234.0

# the smallest geometries that hit each edge of the 32-key chunk / 32-row tile decomposition
CASES = {
    # the expert keys straddle the 32-key chunk edge; 40 rows = one full and one quarter row tile
    "E1": dict(P=30, C=1, H=4, cnt=[30, 7, 1]),
    # the bridge geometry; a 25-key last chunk
    "E2": dict(P=276, C=1, H=4, cnt=[276, 150]),
    # 408 rows = 13 row tiles; over 256 workgroups, so chunks are grouped; dK / dV summed over 13 tiles
    "E3": dict(P=276, C=1, H=50, cnt=[276, 40, 1]),
    # exactly 1024 rows
    "E4": dict(P=40, C=1, H=127, cnt=[40]),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(name, zero_proprio=False):
    """inputs of a case and its float64 reference, computed once"""
    c = CASES[name]
    P, C, H, cnt = c["P"], c["C"], c["H"], c["cnt"]
    B, T, L = len(cnt), C + H, P + C + H
    Lp = (L + 7) // 8 * 8
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    W = NH * HD
    q = torch.randn(B, T, W, generator=g).to(torch.bfloat16)
    k = torch.randn(B, Lp, HD, generator=g).to(torch.bfloat16)
    v = torch.randn(B, Lp, HD, generator=g).to(torch.bfloat16)
    dO = torch.randn(B * T, W, generator=g).to(torch.bfloat16)
    if zero_proprio:  # an untied proprio mixture's last layer: its outputs reach nothing
        dO.view(B, T, W)[:, :C] = 0
    k[:, L:] = float("nan")
    v[:, L:] = float("nan")
    dev = "cuda"
    q, k, v, dO = q.to(dev), k.to(dev), v.to(dev), dO.to(dev)
    allowed = block_mask(cnt, P, C, L)[0][:, P:].to(dev)  # expert rows are never dead rows
    q64 = q.double().view(B, T, NH, HD).permute(0, 2, 1, 3)
    k64, v64 = k[:, :L].double()[:, None], v[:, :L].double()[:, None]
    dO64 = dO.double().view(B, T, NH, HD).permute(0, 2, 1, 3)
    O, lse, _, _ = attention(q64, k64, v64, SCALE, CAP, allowed)
    dq, dk, dv = attention_grads(q64, k64, v64, dO64, SCALE, CAP, allowed)
    ref = dict(O=O.permute(0, 2, 1, 3).reshape(B * T, W), lse=lse.permute(0, 2, 1).reshape(B, T * NH),
               dq=dq.permute(0, 2, 1, 3).reshape(B, T, W), dk=dk.reshape(B, L, HD)[:, P:], dv=dv.reshape(B, L, HD)[:, P:])
    return dict(P=P, C=C, H=H, B=B, T=T, L=L, Lp=Lp, q=q, k=k, v=v, dO=dO, ref=ref,
                cnt=torch.tensor(cnt, dtype=torch.int32, device=dev))


def _q_strided(c):
    """q as rows [P, L) of a [B, L, nh*hd] buffer whose other rows hold NaN"""
    qs = torch.full((c["B"], c["L"], NH * HD), float("nan"), device="cuda", dtype=torch.bfloat16)
    qs[:, c["P"]:] = c["q"]
    return qs


def _fwd(c, strided):
    from pizero_native import ops

    B, T, L, P = c["B"], c["T"], c["L"], c["P"]
    q, Lq, qoff = (_q_strided(c), L, P) if strided else (c["q"], T, 0)
    O = torch.full((B * T, NH * HD), float("nan"), device="cuda", dtype=torch.bfloat16)
    lse = torch.full((B, T * NH), float("nan"), device="cuda", dtype=torch.float32)
    ops.expert_attn_fwd(q, Lq, qoff, c["k"], c["v"], O, lse, B, NH, T, L, SCALE, CAP, c["cnt"], P, c["C"], P)
    torch.cuda.synchronize()
    return O, lse


def _bwd(c, strided, O, lse):
    from pizero_native import ops

    B, T, L, P, Lp = c["B"], c["T"], c["L"], c["P"], c["Lp"]
    q, Lq, qoff = (_q_strided(c), L, P) if strided else (c["q"], T, 0)
    dq = torch.full_like(q, float("nan"))
    dk = torch.full((B, Lp, HD), SENTINEL, device="cuda", dtype=torch.bfloat16)
    dv = torch.full((B, Lp, HD), SENTINEL, device="cuda", dtype=torch.bfloat16)
    dk[:, P:L] = float("nan")
    dv[:, P:L] = float("nan")
    ops.expert_attn_bwd(q, Lq, qoff, c["k"], c["v"], O, lse, c["dO"], dq, dk[:, P:], dv[:, P:], P, T, B, NH, T, L, SCALE,
                        CAP, c["cnt"], P, c["C"], P)
    torch.cuda.synchronize()
    for t in (dk, dv):  # rows outside [P, P + T) are not written
        assert bool((t[:, :P] == SENTINEL).all()) and bool((t[:, L:] == SENTINEL).all())
    if strided:
        assert bool(torch.isnan(dq[:, :P]).all())
        dq = dq[:, P:].contiguous()
    return dq, dk[:, P:L].contiguous(), dv[:, P:L].contiguous()


def _close(name, got, ref, rtol, atol):
    got = got.double()
    err = (got - ref).abs()
    print(f"{name}: max|err| {float(err.max()):.4g}, max|ref| {float(ref.abs().max()):.4g}, atol {atol:.4g}")
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite"
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} outside, worst {float(err.max()):.4g}"


def _check(c, strided):
    ref = c["ref"]
    O, lse = _fwd(c, strided)
    O2, lse2 = _fwd(c, strided)
    assert torch.equal(O, O2) and torch.equal(lse, lse2)
    _close("O", O, ref["O"], 2e-2, 2e-2)
    _close("lse", lse, ref["lse"], 1e-3, 2e-3)
    dq, dk, dv = _bwd(c, strided, O, lse)
    dq2, dk2, dv2 = _bwd(c, strided, O, lse)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
    _close("dQ", dq, ref["dq"], 2e-2, 3e-2 * float(ref["dq"].abs().max()) / 4)
    _close("dK", dk, ref["dk"], 2e-2, 3e-2 * float(ref["dk"].abs().max()))
    _close("dV", dv, ref["dv"], 2e-2, 3e-2 * float(ref["dv"].abs().max()))
    return O, lse, dq, dk, dv


@pytest.mark.parametrize("name", sorted(CASES))
def test_expert_attn_matches_reference(name):
    c = _case(name)
    a = _check(c, strided=False)
    b = _check(c, strided=True)
    for x, y in zip(a, b):  # the addressing of q / dq changes nothing
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", sorted(CASES))
def test_expert_attn_fwd_equals_decode_attn(name):
    """O of pz_expert_attn_fwd is pz_decode_attn's, bit for bit"""
    from pizero_native import ops

    c = _case(name)
    B, T, L, P = c["B"], c["T"], c["L"], c["P"]
    O, _ = _fwd(c, False)
    Od = torch.full_like(O, float("nan"))
    ops.decode_attn(c["q"], T, 0, c["k"], c["v"], Od, B, NH, T, L, SCALE, CAP, c["cnt"], P, c["C"], P)
    torch.cuda.synchronize()
    assert torch.equal(O, Od)


def test_expert_attn_untied_zero_proprio_dO():
    """E2 with dO = 0 on the proprio rows (an untied proprio mixture whose last-layer output is dropped)"""
    c = _case("E2", True)
    _, _, dq, _, _ = _check(c, strided=False)
    assert float(dq[:, : c["C"]].float().abs().max()) == 0.0


def test_expert_attn_refuses_more_than_1024_rows():
    """H = 128 in E4 (1032 rows): an argument error before any launch, forward and backward"""
    from pizero_native import ops
    from pizero_native._lib import NativeError

    P, C, H = 40, 1, 128
    T, L = C + H, P + C + H
    Lp = (L + 7) // 8 * 8
    dev = "cuda"
    q = torch.zeros(1, T, NH * HD, device=dev, dtype=torch.bfloat16)
    k = torch.zeros(1, Lp, HD, device=dev, dtype=torch.bfloat16)
    O = torch.full((T, NH * HD), float("nan"), device=dev, dtype=torch.bfloat16)
    lse = torch.full((1, T * NH), float("nan"), device=dev, dtype=torch.float32)
    cnt = torch.tensor([P], dtype=torch.int32, device=dev)
    with pytest.raises(NativeError, match="1024 query rows"):
        ops.expert_attn_fwd(q, T, 0, k, k, O, lse, 1, NH, T, L, SCALE, CAP, cnt, P, C, P)
    dq = torch.full_like(q, float("nan"))
    dk = torch.full_like(k, SENTINEL)
    with pytest.raises(NativeError, match="1024 query rows"):
        ops.expert_attn_bwd(q, T, 0, k, k, O, lse, O, dq, dk[:, P:], dk[:, P:], P, T, 1, NH, T, L, SCALE, CAP, cnt, P, C, P,
                            ws=torch.empty(1024, device=dev))
    torch.cuda.synchronize()
    assert bool(torch.isnan(O).all()) and bool(torch.isnan(dq).all()) and bool((dk == SENTINEL).all())
