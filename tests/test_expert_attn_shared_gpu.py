"""pz_expert_attn_fwd_shared / pz_expert_attn_bwd_shared (csrc/pz_expert_attn.hip): the action expert's
training attention for several flow draws per observation.  The batch counts (observation, draw) pairs e = b * S + s;
key rows below P come from the observation's K / V (one copy for its S draws), the rest from the pair's own compact
buffers.  Checked per pair against the float64 reference of tests/flash_ref.py on concat(shared[e // S][:P], own[e]).

Inputs are bf16 (upcast for the reference); nh 8, hd 256, cap 50, scale 1/16.  The shared buffers hold NaN in rows
>= P, the own buffers hold NaN in their pad rows, different observations and pairs hold different data and every
output is pre-filled with NaN, so a read from the wrong buffer, batch or row shows.  dk / dv carry a sentinel outside
rows [key0, key0 + nkeys) that must survive, and the shared K / V bytes are compared before and after the backward.
Every launch runs twice and is compared bit for bit (no atomics, fixed-order merges).

Tolerances are the project's own for the same quantities (tests/test_expert_attn_kernels_gpu.py): O rtol = atol = 2e-2,
lse rtol 1e-3 / atol 2e-3, dQ rtol 2e-2 / atol 3e-2 max|ref| / 4, dK and dV rtol 2e-2 / atol 3e-2 max|ref|.
"""

import functools

import pytest
import torch

from tests.flash_ref import attention, attention_grads, block_mask

pytestmark = pytest.mark.gpu

NH, HD, CAP, SCALE = 8, 256, 50.0, 1.0 / 16.0
SENTINEL = 1234.0

# the smallest geometries at which the two-buffer addressing can go wrong (cnt per observation; a pair has its
# observation's count)
CASES = {
    # shared keys 0..29 and own keys 30, 31 in one 16-key tile and one 32-key chunk; 40 rows = one full and one quarter
    # row tile
    "S1": dict(P=30, C=1, H=4, S=3, cnt=[30, 7]),
    # the own keys begin exactly at a chunk edge / at a tile edge
    "S2": dict(P=32, C=1, H=4, S=3, cnt=[32, 5]),
    "S3": dict(P=16, C=1, H=4, S=3, cnt=[16, 9]),
    # the bridge geometry; a 25-key last chunk
    "S4": dict(P=276, C=1, H=4, S=4, cnt=[276, 150]),
    # 13 row tiles per pair; enough workgroups that chunks are grouped; dK / dV summed over 13 tiles
    "S5": dict(P=276, C=1, H=50, S=2, cnt=[276, 40]),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs of a case and its float64 reference per pair, computed once"""
    c = CASES[name]
    P, C, H, S = c["P"], c["C"], c["H"], c["S"]
    nobs, T, L = len(c["cnt"]), C + H, P + C + H
    E = nobs * S
    Lps = (L + 7) // 8 * 8  # the shared buffers are joint K / V buffers: rows [P, Lps) exist and are poison
    Tp = T // 8 * 8 + 8     # own buffers with at least one pad row
    cnt = [n for n in c["cnt"] for _ in range(S)]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    W = NH * HD
    bf = torch.bfloat16
    q = torch.randn(E, T, W, generator=g).to(bf)
    ks = torch.randn(nobs, Lps, HD, generator=g).to(bf)
    vs = torch.randn(nobs, Lps, HD, generator=g).to(bf)
    ko = torch.randn(E, Tp, HD, generator=g).to(bf)
    vo = torch.randn(E, Tp, HD, generator=g).to(bf)
    dO = torch.randn(E * T, W, generator=g).to(bf)
    for t in (ks, vs):
        t[:, P:] = float("nan")
    for t in (ko, vo):
        t[:, T:] = float("nan")
    # the keys of pair e as one [L, HD] block: what the existing entry points take, and what the reference sees
    kf = torch.cat([ks[:, :P].repeat_interleave(S, 0), ko[:, :T]], 1)
    vf = torch.cat([vs[:, :P].repeat_interleave(S, 0), vo[:, :T]], 1)
    allowed = block_mask(cnt, P, C, L)[0][:, P:]  # expert rows are never dead rows
    q64 = q.double().view(E, T, NH, HD).permute(0, 2, 1, 3)
    dO64 = dO.double().view(E, T, NH, HD).permute(0, 2, 1, 3)
    k64, v64 = kf.double()[:, None], vf.double()[:, None]
    dev = "cuda"  # the float64 reference on the device: the same arithmetic, seconds faster for S5
    q64, dO64, k64, v64, allowed = (x.to(dev) for x in (q64, dO64, k64, v64, allowed))
    O, lse, _, _ = attention(q64, k64, v64, SCALE, CAP, allowed)
    dq, dk, dv = attention_grads(q64, k64, v64, dO64, SCALE, CAP, allowed)
    ref = dict(O=O.permute(0, 2, 1, 3).reshape(E * T, W), lse=lse.permute(0, 2, 1).reshape(E, T * NH),
               dq=dq.permute(0, 2, 1, 3).reshape(E, T, W), dk=dk.reshape(E, L, HD)[:, P:], dv=dv.reshape(E, L, HD)[:, P:])
    kfull = torch.full((E, Lps, HD), float("nan"), dtype=bf)
    vfull = torch.full((E, Lps, HD), float("nan"), dtype=bf)
    kfull[:, :L], vfull[:, :L] = kf, vf
    return dict(P=P, C=C, H=H, S=S, E=E, T=T, L=L, Tp=Tp, q=q.to(dev), ks=ks.to(dev), vs=vs.to(dev), ko=ko.to(dev),
                vo=vo.to(dev), dO=dO.to(dev), kfull=kfull.to(dev), vfull=vfull.to(dev), ref=ref,
                cnt=torch.tensor(cnt, dtype=torch.int32, device=dev))


def _fwd(c, ks=None, vs=None, group=None):
    from pizero_native import ops

    E, T, L, P = c["E"], c["T"], c["L"], c["P"]
    ks, vs = (c["ks"], c["vs"]) if ks is None else (ks, vs)
    O = torch.full((E * T, NH * HD), float("nan"), device="cuda", dtype=torch.bfloat16)
    lse = torch.full((E, T * NH), float("nan"), device="cuda", dtype=torch.float32)
    ops.expert_attn_fwd_shared(c["q"], T, 0, ks, vs, c["ko"], c["vo"], c["S"] if group is None else group, O, lse, E, NH,
                               T, L, SCALE, CAP, c["cnt"], P, c["C"], P)
    torch.cuda.synchronize()
    return O, lse


def _grad_bufs(c):
    """dq pre-filled with NaN; dk / dv [E, 1 + T + 2, hd]: NaN in rows [1, 1 + T), the sentinel around them"""
    E, T = c["E"], c["T"]
    dq = torch.full_like(c["q"], float("nan"))
    dk = torch.full((E, T + 3, HD), SENTINEL, device="cuda", dtype=torch.bfloat16)
    dv = torch.full((E, T + 3, HD), SENTINEL, device="cuda", dtype=torch.bfloat16)
    dk[:, 1:1 + T] = float("nan")
    dv[:, 1:1 + T] = float("nan")
    return dq, dk, dv


def _grads_out(c, dq, dk, dv):
    T = c["T"]
    for t in (dk, dv):  # rows outside [key0, key0 + nkeys) are not written
        assert bool((t[:, :1] == SENTINEL).all()) and bool((t[:, 1 + T:] == SENTINEL).all())
    return dq, dk[:, 1:1 + T].contiguous(), dv[:, 1:1 + T].contiguous()


def _bwd(c, O, lse, ks=None, vs=None, group=None):
    from pizero_native import ops

    E, T, L, P = c["E"], c["T"], c["L"], c["P"]
    ks, vs = (c["ks"], c["vs"]) if ks is None else (ks, vs)
    dq, dk, dv = _grad_bufs(c)
    before = [t.clone() for t in (ks, vs)]
    ops.expert_attn_bwd_shared(c["q"], T, 0, ks, vs, c["ko"], c["vo"], c["S"] if group is None else group, O, lse,
                               c["dO"], dq, dk[:, 1:], dv[:, 1:], P, T, E, NH, T, L, SCALE, CAP, c["cnt"], P, c["C"], P)
    torch.cuda.synchronize()
    for t, b in zip((ks, vs), before):  # the shared buffers are read-only (bytes: NaN rows included)
        assert torch.equal(t.view(torch.int16), b.view(torch.int16))
    return _grads_out(c, dq, dk, dv)


def _close(name, got, ref, rtol, atol):
    got = got.double()
    err = (got - ref).abs()
    print(f"{name}: max|err| {float(err.max()):.4g}, max|ref| {float(ref.abs().max()):.4g}, atol {atol:.4g}")
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite"
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} outside, worst {float(err.max()):.4g}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_expert_attn_shared_matches_reference(name):
    c = _case(name)
    ref = c["ref"]
    O, lse = _fwd(c)
    O2, lse2 = _fwd(c)
    assert torch.equal(O, O2) and torch.equal(lse, lse2)
    _close("O", O, ref["O"], 2e-2, 2e-2)
    _close("lse", lse, ref["lse"], 1e-3, 2e-3)
    dq, dk, dv = _bwd(c, O, lse)
    dq2, dk2, dv2 = _bwd(c, O, lse)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
    _close("dQ", dq, ref["dq"], 2e-2, 3e-2 * float(ref["dq"].abs().max()) / 4)
    _close("dK", dk, ref["dk"], 2e-2, 3e-2 * float(ref["dk"].abs().max()))
    _close("dV", dv, ref["dv"], 2e-2, 3e-2 * float(ref["dv"].abs().max()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_expert_attn_shared_equals_unshared(name):
    """kv_group 1 with own = rows P.. of the same data: O, lse, dq, dk, dv of pz_expert_attn_fwd / _bwd, bit for bit --
    and the same bits again with kv_group S reading the observation's one copy"""
    from pizero_native import ops

    c = _case(name)
    E, T, L, P, S = c["E"], c["T"], c["L"], c["P"], c["S"]
    O0 = torch.full((E * T, NH * HD), float("nan"), device="cuda", dtype=torch.bfloat16)
    lse0 = torch.full((E, T * NH), float("nan"), device="cuda", dtype=torch.float32)
    ops.expert_attn_fwd(c["q"], T, 0, c["kfull"], c["vfull"], O0, lse0, E, NH, T, L, SCALE, CAP, c["cnt"], P, c["C"], P)
    dq0, dk0, dv0 = _grad_bufs(c)
    ops.expert_attn_bwd(c["q"], T, 0, c["kfull"], c["vfull"], O0, lse0, c["dO"], dq0, dk0[:, 1:], dv0[:, 1:], P, T, E, NH,
                        T, L, SCALE, CAP, c["cnt"], P, c["C"], P)
    torch.cuda.synchronize()
    want = (O0, lse0, *_grads_out(c, dq0, dk0, dv0))
    # one shared copy per pair, poisoned from row P on
    ks1, vs1 = c["ks"].repeat_interleave(S, 0).contiguous(), c["vs"].repeat_interleave(S, 0).contiguous()
    for ks, vs, group in ((ks1, vs1, 1), (c["ks"], c["vs"], S)):
        O, lse = _fwd(c, ks, vs, group)
        got = (O, lse, *_bwd(c, O, lse, ks, vs, group))
        for n, x, y in zip(("O", "lse", "dq", "dk", "dv"), got, want):
            assert torch.equal(x, y), f"{n} differs from the unshared entry point (kv_group {group})"


def test_expert_attn_shared_refuses_bad_arguments():
    """kv_group < 1, B not a multiple of kv_group, prefix > nk, head_dim != 256, more than 1024 rows: an argument
    error before any launch, forward and backward"""
    from pizero_native import ops
    from pizero_native._lib import NativeError

    c = _case("S1")
    E, T, L, P, S = c["E"], c["T"], c["L"], c["P"], c["S"]
    O = torch.full((E * T, NH * HD), float("nan"), device="cuda", dtype=torch.bfloat16)
    lse = torch.full((E, T * NH), float("nan"), device="cuda", dtype=torch.float32)
    dq, dk, dv = _grad_bufs(c)
    ws = torch.empty(1 << 20, device="cuda")

    def both(match, group=S, prefix=P, ks=c["ks"], vs=c["vs"], T_=T):
        with pytest.raises(NativeError, match=match):
            ops.expert_attn_fwd_shared(c["q"], T_, 0, ks, vs, c["ko"], c["vo"], group, O, lse, E, NH, T_, L, SCALE, CAP,
                                       c["cnt"], prefix, c["C"], prefix)
        with pytest.raises(NativeError, match=match):
            ops.expert_attn_bwd_shared(c["q"], T_, 0, ks, vs, c["ko"], c["vo"], group, O, lse, c["dO"], dq, dk[:, 1:],
                                       dv[:, 1:], prefix, T, E, NH, T_, L, SCALE, CAP, c["cnt"], prefix, c["C"], prefix,
                                       ws=ws)

    both("kv_group must be >= 1", group=0)
    both("multiple of kv_group", group=4)
    both(r"prefix must lie in \[0, nk\]", prefix=L + 1)
    both("1024 query rows", T_=129)
    both("head_dim 256", ks=c["ks"][..., :128], vs=c["vs"][..., :128])
    torch.cuda.synchronize()
    assert bool(torch.isnan(O).all()) and bool(torch.isnan(lse).all()) and bool(torch.isnan(dq).all())
    assert bool(torch.isnan(dk[:, 1:1 + T]).all()) and bool(torch.isnan(dv[:, 1:1 + T]).all())
