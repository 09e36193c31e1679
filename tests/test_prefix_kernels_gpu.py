"""The action-prefix kernels (pz_*_prefix, pz_action_prefix_init, pz_clamp_prefix, pz_action_normalize,
pz_action_denormalize_prefix) on the MI355X, each against a restatement of its own arithmetic.

Row h of sample b is a prefix row iff h < prefix_len[b].  Shapes: H = 4 with d in {0, 1, 3} and H = 50 with d in
{0, 7, 49} (first row, one short of the horizon, several 256-thread blocks), B in {1, 3}, A in {7, 8}, the action
expert's width D in {64 (the tiny model's), 1024}, both time-embedding modes.  At B = 3 the three d's are the three
samples'; at B = 1 each is run on its own.

What "restatement" means here: the project's device code is compiled with FMA contraction, so an expression such as
a + dt * v has no bit-exact torch twin.  Where a kernel shares an expression with its prefix-free sibling, the
non-prefix rows are compared bit for bit with that sibling (itself pinned by tests/test_kernels_gpu.py), and the
prefix rows with the plain torch statement of what a prefix row holds (a cast, a copy, a zero, the embedding of 1.0).
"""

import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.oracle_helpers import O

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SIG = 0.001
SHAPES = [(4, (0, 1, 3)), (50, (0, 7, 49))]
WIDTHS = (O.TINY_DIMS["act_hidden"], 1024)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cases(H, ds, B):
    """the prefix-length vectors of one (H, ds, B): all three at B = 3, one at a time at B = 1"""
    return [list(ds)] if B == 3 else [[d] for d in ds]


def _pl(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _pre(pl, H):
    return torch.arange(H, device="cuda")[None, :] < pl[:, None].long()  # [B, H]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(*shape, device="cuda", generator=g) * 2 - 1) * scale


def _t(B, seed=1):
    return torch.rand(B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) * 0.98 + 0.01


GRID = [(H, ds, B, A) for H, ds in SHAPES for B in (1, 3) for A in (7, 8)]


@pytest.mark.parametrize("H,ds,B,A", GRID)
def test_flow_psi_prefix(H, ds, B, A):
    from pizero_native import ops

    x0, x1, t = _rand(B, H, A, seed=2), _rand(B, H, A, seed=3), _t(B)
    plain = torch.empty(B * H, A, device="cuda", dtype=BF16)
    ops.flow_psi(x0, x1, t, plain, SIG)
    for v in _cases(H, ds, B):
        pl = _pl(v)
        got = torch.full((B * H, A), float("nan"), device="cuda", dtype=BF16)
        ops.flow_psi(x0, x1, t, got, SIG, prefix_len=pl)
        want = torch.where(_pre(pl, H)[..., None], x1.to(BF16), plain.view(B, H, A))
        assert torch.equal(_bits(got.view(B, H, A)), _bits(want)), v
    # the sibling itself is psi_t to within one bf16 rounding of the fp64 value
    ref = (1 - (1 - SIG) * t.double()[:, None, None]) * x0.double() + t.double()[:, None, None] * x1.double()
    assert (plain.view(B, H, A).double() - ref).abs().max() <= 2.0 ** -8 * ref.abs().max()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,ds,B,A", GRID)
def test_time_columns_are_the_embedding_of_one_on_prefix_rows(H, ds, B, A, mode):
    """pz_concat_time_prefix (training), pz_time_embed_rows_prefix and pz_action_in_prefix (inference): the time
    columns are bit for bit pz_time_embed of 1.0f on prefix rows and of t_b elsewhere, in both modes; the other
    columns are what the prefix-free kernels write"""
    from pizero_native import ops

    t = _t(B)
    one = torch.ones(1, device="cuda", dtype=F32)
    for D in WIDTHS:
        temb = torch.empty(B, D, device="cuda", dtype=BF16)
        temb1 = torch.empty(1, D, device="cuda", dtype=BF16)
        ops.time_embed(t, temb, 100.0, ref_bf16=bool(mode))
        ops.time_embed(one, temb1, 100.0, ref_bf16=bool(mode))
        assert not torch.equal(temb1.expand(B, D), temb)
        e1 = _rand(B * H, D, seed=5).to(BF16)
        action = _rand(B, H, A, seed=6)
        W1, b1 = _rand(D, A, seed=7).to(BF16), _rand(D, seed=8).to(BF16)
        lin = torch.empty(B * H, D, device="cuda", dtype=BF16)
        ops.small_linear(action.view(B * H, A).to(BF16), W1, lin, bias=b1)
        for v in _cases(H, ds, B):
            pl = _pl(v)
            pre = _pre(pl, H)[..., None]
            want_t = torch.where(pre, temb1.view(1, 1, D), temb[:, None, :].expand(B, H, D)).reshape(B * H, D)
            cat = torch.full((B * H, 2 * D), float("nan"), device="cuda", dtype=BF16)
            ops.concat_time(temb, e1, cat, B, H, D, prefix_len=pl, max_period=100.0, ref_bf16=bool(mode))
            assert torch.equal(_bits(cat[:, :D]), _bits(want_t)), ("concat", D, v)
            assert torch.equal(_bits(cat[:, D:]), _bits(e1))
            rows = torch.full((B * H, 2 * D), float("nan"), device="cuda", dtype=BF16)
            ops.time_embed_rows(t, rows[:, :D], H, 100.0, ref_bf16=bool(mode), prefix_len=pl)
            assert torch.equal(_bits(rows[:, :D]), _bits(want_t)), ("rows", D, v)
            assert torch.isnan(rows[:, D:]).all()
            fused = torch.full((B * H, 2 * D), float("nan"), device="cuda", dtype=BF16)
            ops.action_in(action, W1, b1, t, fused, B, H, D, 100.0, ref_bf16=bool(mode), prefix_len=pl)
            assert torch.equal(_bits(fused[:, :D]), _bits(want_t)), ("action_in", D, v)
            assert torch.equal(_bits(fused[:, D:]), _bits(lin)), ("action_in linear", D, v)


@pytest.mark.parametrize("H,ds,B,A", GRID)
def test_action_out_and_euler_prefix(H, ds, B, A):
    """one step: pz_action_out_prefix equals RMSNorm + decoder + pz_euler_step_prefix bit for bit, which equals
    pz_euler_step on the other rows and leaves prefix rows alone; ten steps: t equals the prefix-free t bit for bit
    (row 0 is a prefix row whenever d >= 1: its lane still advances t) and prefix rows never change"""
    from pizero_native import ops

    dt = 0.1
    for D in WIDTHS:
        nw, Wd, bd = _rand(D, seed=11).to(BF16), _rand(A, D, seed=12, scale=0.2).to(BF16), _rand(A, seed=13).to(BF16)
        xs = [_rand(B * H, D, seed=20 + i).to(BF16) for i in range(10)]
        a0 = _rand(B, H, A, seed=14)

        def unfused(x, action, t, pl):
            y = torch.empty_like(x)
            ops.rmsnorm(x, nw, y, None, 1e-6)
            v = torch.zeros(B * H, 8, device="cuda", dtype=BF16)
            ops.small_linear(y, Wd, v[:, :A], bias=bd)
            ops.euler_step(action, v, 8, H * 8, t, B, H, A, dt, prefix_len=pl)

        plain_a, plain_t = a0.clone(), torch.zeros(B, device="cuda")
        unfused(xs[0], plain_a, plain_t, None)
        t_ref = torch.zeros(B, device="cuda")
        for x in xs:
            ops.action_out(x, nw, 1e-6, Wd, bd, a0.clone(), t_ref, B, H, dt)
        for v in _cases(H, ds, B):
            pl = _pl(v)
            pre = _pre(pl, H)[..., None]
            fa, ft = a0.clone(), torch.zeros(B, device="cuda")
            ops.action_out(xs[0], nw, 1e-6, Wd, bd, fa, ft, B, H, dt, prefix_len=pl)
            ua, ut = a0.clone(), torch.zeros(B, device="cuda")
            unfused(xs[0], ua, ut, pl)
            assert torch.equal(_bits(fa), _bits(ua)) and torch.equal(_bits(ft), _bits(ut)), (D, v)
            assert torch.equal(_bits(fa), _bits(torch.where(pre, a0, plain_a))), (D, v)
            assert torch.equal(_bits(ft), _bits(plain_t))
            for x in xs[1:]:
                ops.action_out(x, nw, 1e-6, Wd, bd, fa, ft, B, H, dt, prefix_len=pl)
                unfused(x, ua, ut, pl)
            assert torch.equal(_bits(ft), _bits(t_ref)) and torch.equal(_bits(ut), _bits(t_ref)), (D, v, ft, t_ref)
            assert torch.equal(_bits(fa), _bits(ua))
            assert torch.equal(_bits(fa)[pre.expand_as(fa)], _bits(a0)[pre.expand_as(a0)])
            if max(v) > 0:
                assert not torch.equal(fa[~pre.expand_as(fa)], a0[~pre.expand_as(a0)])


@pytest.mark.parametrize("H,ds,B,A", GRID)
def test_flow_loss_prefix(H, ds, B, A):
    """dv: zero on prefix rows and bit for bit the fp32 statement of the kernel elsewhere, at the model's sig_min with a
    grad scale that is no power of two (and at sig_min = 0), for every d.  The one contractable expression is
    u = x1 - (1 - sig) x0 = fma(-(1 - sig), x0, x1), restated as fp32(fp64(x1) - fp64(1 - sig) fp64(x0)): the product of
    two fp32 values is exact in fp64.  The rest -- e = v - u, (g 2) e, one division by the live count, one bf16
    rounding -- has no product-sum and is plain fp32.  With every d = 0 the loss and dv are the sibling's bits.
    loss: against the fp64 sum over the n live elements, relative bound n 2^-24 (every term is non-negative, so an
    fp32 accumulation in any order loses at most that)."""
    from pizero_native import ops

    Tg = H + 1  # the action rows sit behind one proprio row per sample, as in the tied expert group
    x0, x1 = _rand(B, H, A, seed=31), _rand(B, H, A, seed=32)
    v = _rand(B * Tg, 8, seed=33).to(BF16)
    va = v.view(B, Tg, 8)[:, 1:, :A]
    for v_pl in _cases(H, ds, B):
        pl = _pl(v_pl)
        pre = _pre(pl, H)[..., None].expand(B, H, A)
        n = A * int((H - pl.long()).sum())
        for sig, g in ((0.0, 0.5), (SIG, 0.37)):
            gs = torch.tensor([g], device="cuda", dtype=F32)
            loss = torch.full((1,), float("nan"), device="cuda")
            dv = torch.full((B * Tg, 8), 7.0, device="cuda", dtype=BF16)
            ops.flow_loss(v[1:], 8, Tg * 8, x0, x1, loss, dv[1:], gs, B, H, A, sig, prefix_len=pl)
            got = dv.view(B, Tg, 8)[:, 1:, :A]
            assert (got[pre] == 0).all(), (v_pl, sig)
            assert (dv.view(B, Tg, 8)[:, 0] == 7).all() and (dv.view(B, Tg, 8)[:, :, A:] == 7).all()  # untouched
            oms = float(np.float32(1.0) - np.float32(sig))  # the kernel's fp32 (1 - sig_min)
            u = (x1.double() - oms * x0.double()).float()
            e = va.float() - u
            want = (((gs * 2.0) * e) / float(n)).to(BF16)
            assert torch.equal(_bits(got[~pre]), _bits(want[~pre])), (v_pl, sig)
            ref = float((e.double()[~pre] ** 2).sum() / n)
            rel = abs(float(loss) - ref) / ref
            print(f"flow_loss H={H} B={B} A={A} d={v_pl} sig={sig}: n={n} loss {float(loss):.7f} fp64 {ref:.7f} "
                  f"rel {rel:.2e} (bound {n * 2.0 ** -24:.2e})")
            assert rel <= n * 2.0 ** -24, (rel, n)
            if max(v_pl) == 0:
                loss0 = torch.empty(1, device="cuda")
                dv0 = torch.full((B * Tg, 8), 7.0, device="cuda", dtype=BF16)
                ops.flow_loss(v[1:], 8, Tg * 8, x0, x1, loss0, dv0[1:], gs, B, H, A, sig)
                assert torch.equal(_bits(loss), _bits(loss0)) and torch.equal(_bits(dv), _bits(dv0)), (v_pl, sig)
            # loss only (the forward's call): the same loss, dv not written
            loss2 = torch.empty(1, device="cuda")
            ops.flow_loss(v[1:], 8, Tg * 8, x0, x1, loss2, None, None, B, H, A, sig, prefix_len=pl)
            assert torch.equal(_bits(loss2), _bits(loss))


@pytest.mark.parametrize("H,ds,B,A", GRID)
def test_prefix_init_and_clamp_prefix(H, ds, B, A):
    from pizero_native import ops

    noise, prefix = _rand(B, H, A, seed=41, scale=2.0), _rand(B, H, A, seed=42, scale=2.0)
    for v in _cases(H, ds, B):
        pl = _pl(v)
        pre = _pre(pl, H)[..., None]
        a = noise.clone()
        ops.action_prefix_init(a, prefix, pl)
        want = torch.where(pre, prefix, noise)
        assert torch.equal(_bits(a), _bits(want)), v
        ops.clamp_(a, -1.0, 1.0, prefix_len=pl)
        assert torch.equal(_bits(a), _bits(torch.where(pre, prefix, noise.clamp(-1.0, 1.0)))), v
        if max(v) > 0:
            assert a.abs().max() > 1.0  # a prefix value outside the clip range is returned as given
        b = noise.clone()
        ops.clamp_(b, -1.0, 1.0)
        assert torch.equal(_bits(b)[~pre.expand_as(b)], _bits(a)[~pre.expand_as(a)])


def _stats():
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")))
    f = lambda k: torch.tensor(np.asarray(s["action"][k], np.float64)).to(F32).cuda()  # noqa: E731
    return {"bound": (f("p01"), f("p99"), ("p01", "p99")), "gaussian": (f("mean"), f("std"), ("mean", "std"))}


@pytest.mark.parametrize("kind", ["bound", "gaussian"])
@pytest.mark.parametrize("H,ds,B", [(H, ds, B) for H, ds in SHAPES for B in (1, 3)])
def test_action_normalize_and_denormalize_passthrough(H, ds, B, kind):
    """pz_action_normalize against the numpy twin BaseEnvAdapter.normalize_action evaluated in fp64 on the fp32 inputs
    (statistics included: the kernel sees them as fp32), to 1 fp32 ulp.  gaussian, (x - a) / (b + 1e-8): three
    correctly rounded operations, each within half an ulp relative, so the result is within 1.5 2^-24 < one ulp of
    |want|.  bound, 2 (x - a) / (b - a + 1e-8) - 1: the ulp is that of the largest intermediate, the quotient
    want + 1 in [0, 2] (the final subtraction cancels, so an ulp of the result itself is not attainable near 0):
    2^-23 max(1, |want + 1|).  And bit for bit against the same expression in fp32 torch.
    pz_action_denormalize_prefix: rows h < d_b are the caller's bits, the rest pz_action_denormalize's."""
    from pizero_native import ops
    from src.agent.env_adapter.base import BaseEnvAdapter

    a, b, names = _stats()[kind]
    A = 7
    stats = {"action": {names[0]: a.double().cpu().numpy(), names[1]: b.double().cpu().numpy()}}
    ad = BaseEnvAdapter()
    y = _rand(B, H, A, seed=51, scale=1.2)  # normalised values, some outside [-1, 1]
    raw = ops.action_denormalize(y, a, b, kind)
    raw[..., -1] = _rand(B, H, seed=52, scale=3.0)
    got = ops.action_normalize(raw, a, b, kind)
    want = ad.normalize_action(raw.double().cpu().numpy(), stats, kind)
    g = got.double().cpu().numpy()
    ulp = 2.0 ** -23
    if kind == "bound":
        scale = np.maximum(1.0, np.abs(want + 1.0))
        assert (want[..., :-1] == 1).any() or (want[..., :-1] == -1).any()  # the clip acts
    else:
        scale = np.maximum(np.abs(want), 2.0 ** -100)
    err = np.abs(g - want) / scale
    print(f"action_normalize {kind} H={H} B={B}: max err {err[..., :-1].max() / ulp:.3f} ulp of the scale")
    assert err[..., :-1].max() <= ulp, err[..., :-1].max() / ulp
    # the kernel is compiled without FMA contraction, so the fp32 statement of its expression is its bits
    head, p, q = raw[..., :-1], a[:-1], b[:-1]
    if kind == "bound":
        f32 = (2.0 * (head - p) / (q - p + 1e-8) - 1.0).clamp(-1.0, 1.0)
    else:
        f32 = (head - p) / (q + 1e-8)
    assert f32.dtype == F32 and torch.equal(_bits(got[..., :-1]), _bits(f32))
    assert torch.equal(_bits(got[..., -1]), _bits(raw[..., -1]))  # the gripper passes through
    assert got[..., :-1].abs().max() <= 1.0 or kind == "gaussian"
    for n_pass in (0, 3):
        gp = ops.action_normalize(raw, a, b, kind, n_pass=n_pass)
        assert torch.equal(_bits(gp[..., :A - max(n_pass, 1)]), _bits(got[..., :A - max(n_pass, 1)]))
        if n_pass:
            assert torch.equal(_bits(gp[..., A - n_pass:]), _bits(raw[..., A - n_pass:]))
    prev = _rand(B, H, A, seed=53, scale=5.0)
    plain = ops.action_denormalize(y, a, b, kind)
    for v in _cases(H, ds, B):
        pl = _pl(v)
        pre = _pre(pl, H)[..., None]
        out = ops.action_denormalize(y, a, b, kind, prev=prev, prefix_len=pl)
        assert torch.equal(_bits(out), _bits(torch.where(pre, prev, plain))), v


def test_wrappers_refuse_a_malformed_prefix_len():
    from pizero_native import ops

    x = torch.zeros(3, 4, 7, device="cuda")
    for bad in (torch.zeros(3, device="cuda", dtype=torch.int64), torch.zeros(2, device="cuda", dtype=torch.int32),
                torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(AssertionError, match="prefix_len"):
            ops.action_prefix_init(x, x.clone(), bad)
