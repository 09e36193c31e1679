"""float64 reference of the fused attention kernels (csrc/pz_flash.hip), independent of test_flash_gpu.py's.

The Pi0 block mask is restated from the reference model's own rule (pizero.py:271-306: three slice assignments
over a finfo.min-filled mask), not from the kernels' predicate or test_flash_gpu.joint_mask.  Everything runs in
float64 on whatever device the inputs live on; callers upcast the bf16 operands, so kernel and reference see
identical inputs.

Layout: q [..., Lq, D], k / v [..., Lk, D] with leading dims broadcastable to [B, heads]; allowed [B, Lq, Lk]
(bool) and dead [B, Lq] broadcast over the heads.
"""

import torch

# joint geometries of tests/test_flash_shapes_gpu.py: P prefix, C proprio, Hc action tokens, valid prefix per sample
JOINT = {
    "J1": dict(P=7, C=1, Hc=1, cnt=[7, 3, 1]),  # below one key block; nq = 72: a partial workgroup, half a 16-row tile
    "J2": dict(P=56, C=1, Hc=7, cnt=[56, 1]),  # exactly one 64-key block; nq = 512: exactly four workgroups
    "J3": dict(P=60, C=1, Hc=4, cnt=[60, 33]),  # one key past a block; nq = 520: an 8-row tail
    "J4": dict(P=130, C=2, Hc=3, cnt=[130, 128, 65, 64, 63, 32]),  # cnt on / around 64- and 32-key edges; C = 2
    "J5": dict(P=300, C=1, Hc=19, cnt=[300, 257]),  # L = 320: the probs / ds maximum, five full blocks
    "J6": dict(P=300, C=1, Hc=20, cnt=[300, 256]),  # L = 321: a sixth block of one key; above the probs / ds limit
    "J7": dict(P=12, C=1, Hc=3, cnt=[12, 5]),  # the tiny config: nh = 2, hd 16 / 32
}


def block_mask(cnt, P, C, L):
    """allowed [B, L, L] (bool) and dead [B, L] of the Pi0 block attention: P prefix (image / text) tokens of which
    the first cnt[b] are valid, C proprio tokens, L - P - C action tokens."""
    B = len(cnt)
    allowed = torch.zeros(B, L, L, dtype=torch.bool)
    for b, c in enumerate(cnt):
        c = int(c)
        allowed[b, :c, :c] = True  # image / text attend to itself
        allowed[b, P:, :c] = True  # proprio / action attend to image / text
    allowed[:, P:P + C, P:P + C] = True  # proprio attends to itself
    allowed[:, P + C:, P:] = True  # action attends to itself and proprio
    # rows [cnt, P): every key carries finfo.min, which absorbs the logit -> uniform over all L keys
    dead = ~allowed.any(-1)
    return allowed, dead


def attention(q, k, v, scale, cap=0.0, allowed=None, dead=None):
    """-> O, lse, P, t.  t = tanh(s / cap) of the scaled logits (None without soft-cap), taken before the mask, so
    it is defined at masked keys too; dead rows have logit 0 at every key: P = 1 / Lk, lse = log Lk, t = 0."""
    assert q.dtype == torch.float64 and k.dtype == torch.float64 and v.dtype == torch.float64
    s = (q @ k.transpose(-1, -2)) * scale
    if dead is not None:
        s = torch.where(dead[:, None, :, None], torch.zeros_like(s), s)
    t = None
    if cap > 0:
        t = torch.tanh(s / cap)
        s = cap * t
    if allowed is not None:
        masked = ~allowed if dead is None else ~allowed & ~dead[..., None]
        s = s.masked_fill(masked[:, None], float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    return p @ v, lse, p, t


def attention_grads(q, k, v, dO, scale, cap=0.0, allowed=None, dead=None):
    """dQ, dK, dV of sum(O * dO) by float64 autograd; k / v broadcast over heads (MQA) get the summed gradient."""
    q, k, v = (x.detach().clone().requires_grad_() for x in (q, k, v))
    o = attention(q, k, v, scale, cap, allowed, dead)[0]
    return torch.autograd.grad(o, (q, k, v), dO)


def softmax_bwd_ds(p, t, dP, scale, cap=0.0):
    """dS = scale (1 - t^2) P (dP - rowsum(P dP)): the soft-cap softmax backward from P and t = tanh(s / cap)."""
    ds = p * (dP - (p * dP).sum(-1, keepdim=True)) * scale
    if cap > 0:
        ds = ds * (1 - t * t)
    return ds
