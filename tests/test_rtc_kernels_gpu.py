"""pz_rtc_seed / pz_rtc_euler (csrc/pz_rtc.hip) on the MI355X against the numpy float32 restatement of
their arithmetic (tests/rtc_ref.py), bit for bit: the file is built without FMA contraction and every multiply and
add is rounded by itself.

B in {1, 3}, H in {1, 4, 50} (one row, the bridge chunk, several 256-thread blocks), A in {7, 8}; the weights hold
zeros, ones and fractions; the seed buffer is checked both for action rows only (T = H) and for the tied group's
layout (T = C + H rows per sample, the action rows after the proprio row); v is addressed through a row stride of 8
and the batch stride of that layout, as pz_euler_step addresses it.
"""

import numpy as np
import pytest
import torch

from tests import rtc_ref as R

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
GRID = [(B, H, A) for B in (1, 3) for H in (1, 4, 50) for A in (7, 8)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(B, H, A, C, seed):
    """inputs on the host (numpy) -- v and dA hold bf16 values"""
    rng = np.random.default_rng(seed)
    T = C + H
    x = dict(action=rng.standard_normal((B, H, A)).astype(np.float32),
             target=rng.standard_normal((B, H, A)).astype(np.float32),
             v=R.bf16_round(rng.standard_normal((B, H, A)).astype(np.float32)),
             dA=R.bf16_round(rng.standard_normal((B, H, A)).astype(np.float32)),
             t=(rng.random(B) * 0.9).astype(np.float32))
    w = rng.random((B, H)).astype(np.float32)
    w[:, ::3] = 1.0  # ones, ...
    w[:, 1::3] = 0.0  # ... zeros and fractions in every sample (H = 1: a one)
    if H == 1 and B > 1:
        w[1, 0], w[2, 0] = 0.0, 0.37
    x["w"] = w
    # v as the decoder leaves it: [B * T, 8] bf16, the action rows after the C proprio rows, NaN everywhere else
    vbuf = torch.full((B * T, 8), float("nan"), dtype=F32)
    vbuf.view(B, T, 8)[:, C:, :A] = torch.from_numpy(x["v"])
    x["vbuf"] = vbuf.to(BF16).cuda()
    return x, T


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


@pytest.mark.parametrize("C", [0, 1])
@pytest.mark.parametrize("B,H,A", GRID)
def test_seed(B, H, A, C):
    from pizero_native import ops

    x, T = _case(B, H, A, C, seed=100 * H + 10 * B + A)
    e_ref, eb_ref = R.seed_np(x["action"], x["v"], x["target"], x["w"], x["t"])
    e = torch.full((B, H, A), float("nan"), device="cuda", dtype=F32)
    dv = torch.full((B * T, 8), float("nan"), device="cuda", dtype=BF16)
    action, t = _dev(x["action"]), _dev(x["t"])
    ops.rtc_seed(action, x["vbuf"][C:], 8, T * 8, _dev(x["target"]), _dev(x["w"]), t, e, dv, T, C)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e), torch.from_numpy(e_ref).view(torch.int32))
    want = torch.zeros(B, T, 8)
    want[:, C:, :A] = torch.from_numpy(eb_ref)
    got = dv.view(B, T, 8)
    assert torch.equal(_bits(got), _bits(want.to(BF16)))  # exact: eb_ref holds bf16 values
    assert (got[:, :C] == 0).all() and (got[:, :, A:] == 0).all()  # proprio rows and pad columns
    assert (got[:, C:, :A][torch.from_numpy(x["w"] == 0).cuda()] == 0).all()
    # inputs untouched
    assert torch.equal(_bits(action), torch.from_numpy(x["action"]).view(torch.int32))
    assert torch.equal(_bits(t), torch.from_numpy(x["t"]).view(torch.int32))


@pytest.mark.parametrize("B,H,A", GRID)
def test_euler(B, H, A):
    from pizero_native import ops

    C = 1
    x, T = _case(B, H, A, C, seed=7 + 100 * H + 10 * B + A)
    coef = np.asarray([5.0, 4.25, 2.7619047], dtype=np.float32)
    e_ref, _ = R.seed_np(x["action"], x["v"], x["target"], x["w"], x["t"])
    dt = 0.1
    action, t, e = _dev(x["action"]), _dev(x["t"]), _dev(e_ref)
    dA = torch.full((B * H, 8), float("nan"), dtype=F32)  # row stride 8, as the small GEMM writes it
    dA[:, :A] = torch.from_numpy(x["dA"]).view(B * H, A)
    dA = dA.to(BF16).cuda()
    a_ref, t_ref = x["action"], x["t"]
    for k in (1, 2):  # two steps on the same buffers: t advances once per sample and per call
        ops.rtc_euler(action, x["vbuf"][C:], 8, T * 8, e, dA[:, :A], t, _dev(coef), k, dt)
        a_ref, t_ref = R.euler_np(a_ref, x["v"], e_ref, x["dA"], t_ref, coef[k], dt)
        torch.cuda.synchronize()
        assert torch.equal(_bits(action), torch.from_numpy(a_ref).view(torch.int32)), f"step {k}"
        assert torch.equal(_bits(t), torch.from_numpy(t_ref).view(torch.int32)), f"step {k}"
    assert torch.equal(_bits(e), torch.from_numpy(e_ref).view(torch.int32))


def test_argument_checks():
    from pizero_native import ops
    from pizero_native._lib import NativeError

    B, H, A = 1, 4, 7
    z = torch.zeros(B, H, A, device="cuda")
    v = torch.zeros(B * H, 8, device="cuda", dtype=BF16)
    t = torch.zeros(B, device="cuda")
    coef = torch.ones(10, device="cuda")
    with pytest.raises(NativeError, match="coefficient table"):
        ops.rtc_euler(z, v, 8, H * 8, z.clone(), v, t, coef, 10, 0.1)
    with pytest.raises(NativeError, match="row0"):
        ops.rtc_seed(z, v, 8, H * 8, z.clone(), torch.ones(B, H, device="cuda"), t, z.clone(), v.clone(), H, 1)
    torch.cuda.synchronize()
    assert (z == 0).all() and (t == 0).all()
