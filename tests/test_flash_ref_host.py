"""CPU checks of tests/flash_ref.py, the float64 reference the fused-attention shape tests compare against."""

import pytest
import torch

from tests import flash_ref
from tests.flash_ref import JOINT


def _brute_mask(cnt, P, C, L):
    """the mask drawn in pizero.py:271-285, one (b, i, j) at a time"""
    B = len(cnt)
    allowed = torch.zeros(B, L, L, dtype=torch.bool)
    dead = torch.zeros(B, L, dtype=torch.bool)
    for b in range(B):
        for i in range(L):
            for j in range(L):
                key_valid = j < cnt[b]
                if i < P:  # image / text row (pad rows see nothing)
                    ok = i < cnt[b] and key_valid
                elif i < P + C:  # proprio row
                    ok = key_valid or P <= j < P + C
                else:  # action row
                    ok = key_valid or j >= P
                allowed[b, i, j] = ok
            dead[b, i] = cnt[b] <= i < P
    return allowed, dead


@pytest.mark.parametrize("jid", sorted(JOINT))
def test_block_mask_matches_brute_force(jid):
    g = JOINT[jid]
    L = g["P"] + g["C"] + g["Hc"]
    allowed, dead = flash_ref.block_mask(g["cnt"], g["P"], g["C"], L)
    ra, rd = _brute_mask(g["cnt"], g["P"], g["C"], L)
    assert torch.equal(allowed, ra)
    assert torch.equal(dead, rd)


def _qkv(B=2, H=3, Lq=5, Lk=7, D=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, Lq, D, generator=g, dtype=torch.float64),
            torch.randn(B, H, Lk, D, generator=g, dtype=torch.float64),
            torch.randn(B, H, Lk, D, generator=g, dtype=torch.float64))


def test_attention_plain_matches_sdpa():
    q, k, v = _qkv()
    o, lse, p, t = flash_ref.attention(q, k, v, 0.37)
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=0.37)
    assert t is None
    assert (o - ref).abs().max().item() <= 1e-12
    assert (p.sum(-1) - 1).abs().max().item() <= 1e-12
    assert (lse - torch.log(torch.exp(q @ k.transpose(-1, -2) * 0.37).sum(-1))).abs().max().item() <= 1e-12


def test_attention_softcap_matches_direct_softmax():
    q, k, v = _qkv(seed=1)
    q = q * 30  # logits well into the cap's curved range
    o, _, p, t = flash_ref.attention(q, k, v, 0.5, cap=50.0)
    s = 50.0 * torch.tanh((q @ k.transpose(-1, -2)) * 0.5 / 50.0)
    pr = torch.softmax(s, -1)
    ref = pr @ v
    assert (o - ref).abs().max().item() <= 1e-12
    assert (p - pr).abs().max().item() <= 1e-12
    assert (t - s / 50.0).abs().max().item() <= 1e-12


def test_attention_block_mask_rows():
    """masked keys get p exactly 0, dead rows are uniform over all keys with t = 0 and lse = log L"""
    P, C, Hc, cnt = 5, 1, 2, [5, 2]
    L = P + C + Hc
    allowed, dead = flash_ref.block_mask(cnt, P, C, L)
    q, k, v = _qkv(B=2, H=3, Lq=L, Lk=L, seed=2)
    o, lse, p, t = flash_ref.attention(q, k, v, 0.5, 50.0, allowed, dead)
    masked = (~allowed & ~dead[..., None])[:, None].expand_as(p)
    assert (p[masked] == 0).all() and (p[~masked] > 0).all()
    assert (p.permute(0, 2, 1, 3)[dead] - 1.0 / L).abs().max().item() <= 1e-15
    assert (t.permute(0, 2, 1, 3)[dead] == 0).all()
    assert (lse.permute(0, 2, 1)[dead] - torch.log(torch.tensor(float(L), dtype=torch.float64))).abs().max() <= 1e-12
    assert (o.permute(0, 2, 1, 3)[dead] - v.mean(2)[1][None]).abs().max().item() <= 1e-12


def test_attention_grads_gradcheck():
    B, H, L, D = 2, 3, 5, 4
    P, C, cnt = 3, 1, [3, 1]
    allowed, dead = flash_ref.block_mask(cnt, P, C, L)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, H, L, D, generator=g, dtype=torch.float64, requires_grad=True)
    k = torch.randn(B, 1, L, D, generator=g, dtype=torch.float64, requires_grad=True)
    v = torch.randn(B, 1, L, D, generator=g, dtype=torch.float64, requires_grad=True)
    for cap, al, de in ((0.0, None, None), (2.0, allowed, dead)):
        fn = lambda q, k, v: flash_ref.attention(q, k, v, 0.7, cap, al, de)[0]  # noqa: E731
        assert torch.autograd.gradcheck(fn, (q, k, v))
        dO = torch.randn(B, H, L, D, generator=g, dtype=torch.float64)
        dq, dk, dv = flash_ref.attention_grads(q, k, v, dO, 0.7, cap, al, de)
        rq, rk, rv = torch.autograd.grad(fn(q, k, v), (q, k, v), dO)
        assert torch.equal(dq, rq) and torch.equal(dk, rk) and torch.equal(dv, rv)
        assert dk.shape == k.shape and dv.shape == v.shape


def test_softmax_bwd_ds_matches_autograd():
    """dS from (P, t, dP) equals autograd's gradient of the logits s through cap * tanh(s / cap) and softmax"""
    g = torch.Generator().manual_seed(4)
    s = torch.randn(2, 6, 9, generator=g, dtype=torch.float64) * 3
    dP = torch.randn(2, 6, 9, generator=g, dtype=torch.float64)
    for cap in (0.0, 4.0):
        raw = s.clone().requires_grad_()
        x = raw * 0.3
        t = torch.tanh(x / cap) if cap > 0 else None
        p = torch.softmax(cap * t if cap > 0 else x, -1)
        (ref,) = torch.autograd.grad(p, raw, dP)
        got = flash_ref.softmax_bwd_ds(p.detach(), None if t is None else t.detach(), dP, 0.3, cap)
        assert (got - ref).abs().max().item() <= 1e-12


def test_masked_keys_inert():
    """overwriting K / V at masked prefix keys [cnt, P) leaves every live row's O, lse and P bitwise unchanged"""
    P, C, Hc, cnt = 6, 1, 2, [6, 2]
    L = P + C + Hc
    allowed, dead = flash_ref.block_mask(cnt, P, C, L)
    q, k, v = _qkv(B=2, H=2, Lq=L, Lk=L, seed=5)
    k2, v2 = k.clone(), v.clone()
    for b, c in enumerate(cnt):
        k2[b, :, c:P] = 100 * torch.randn(P - c, k.shape[-1], dtype=torch.float64)
        v2[b, :, c:P] = 100 * torch.randn(P - c, v.shape[-1], dtype=torch.float64)
    a = flash_ref.attention(q, k, v, 0.5, 50.0, allowed, dead)
    b_ = flash_ref.attention(q, k2, v2, 0.5, 50.0, allowed, dead)
    live = ~dead
    for x, y in zip(a[:3], b_[:3]):
        x, y = x.movedim(1, 2), y.movedim(1, 2)  # [B, L, H, ...]
        assert torch.equal(x[live], y[live])
