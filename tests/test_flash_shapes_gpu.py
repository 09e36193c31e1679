"""The fused attention kernels (csrc/pz_flash.hip) away from the one Pi0 geometry, against tests/flash_ref.py (float64).

Small joint geometries J1..J7 (tests/flash_ref.py: JOINT) put the key count, the query-row count and the valid-prefix
counts on, one past and below the kernels' tile edges (64 / 32 keys per block, 32 query rows per dK / dV step, 128 query
rows per workgroup, 320 keys at most for the probs / ds kernels), where one dropped or duplicated key moves the output
by far more than the tolerance.  K / V rows [L, Lp) hold NaN (every kernel guards key < nk), and every output buffer
sits between two NaN guard rows and is itself NaN-filled: after a call the guards are still NaN (nothing written out of
range) and the payload holds none (everything in range written).

Tolerances are test_flash_gpu.py's / test_fp8_gpu.py's for the same kernels.  Two are not set there:
  * delta = rowsum(dO * O) from pz_flash_bwd, against rowsum(dO * O_ref): the kernel's O is bf16 (relative 2^-9 per
    element) of a product with the bf16-rounded P (relative 2^-9 per probability), so |O - O_ref| <= 2^-8 (P |V|) per
    element in the worst case; a factor 2 covers the fast exp / tanh and the fp32 accumulation:
    |delta - ref| <= 2^-7 sum_d |dO_d| (P |V|)_d + 1e-6.
  * delta from pz_flash_bwd_prep on given bf16 O / dO (products exact in fp32, at most 256 terms summed in fp32):
    |delta - ref| <= 255 * 2^-24 sum_d |dO_d O_d| < 2e-5 sum_d |dO_d O_d|.
"""

import functools
import math
import zlib

import pytest
import torch

from tests import flash_ref
from tests.flash_ref import JOINT

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pizero_native

    pizero_native.lib()
    torch.manual_seed(0)


def close(out, ref, rtol=2e-2, atol=2e-2):
    out, ref = out.float(), ref.float()
    err = (out - ref).abs()
    bad = (err > atol + rtol * ref.abs()).sum().item()
    assert bad == 0, f"{bad} mismatches, max err {err.max().item():.4g}"


def _ops():
    from pizero_native import ops

    return ops


def _gen(*key):
    return torch.Generator(device=dev).manual_seed(zlib.crc32(repr(key).encode()))


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, device=dev, generator=g) * scale).to(BF16)


class Guarded:
    """a NaN-filled [rows, cols] buffer with one NaN guard row before and one after it"""

    def __init__(self, rows, cols, dtype=BF16):
        self.full = torch.full((rows + 2, cols), NAN, device=dev, dtype=dtype)
        self.t = self.full[1:-1]

    def check(self, what, untouched=None):
        """guards intact, payload fully written -- except the rows flagged in untouched, which must still be NaN"""
        assert bool(torch.isnan(self.full[0]).all() and torch.isnan(self.full[-1]).all()), f"{what}: guard row written"
        nan = torch.isnan(self.t)
        if untouched is None:
            assert not bool(nan.any()), f"{what}: {int(nan.sum())} NaN / unwritten elements"
        else:
            assert not bool(nan[~untouched].any()), f"{what}: {int(nan[~untouched].sum())} NaN / unwritten elements"
            assert bool(nan[untouched].all()), f"{what}: rows the kernel documents as untouched were written"

    def untouched(self, what):
        assert bool(torch.isnan(self.full).all()), f"{what}: written although the call was rejected"


class Case:
    """inputs of one joint geometry in the kernels' row layout (query row r = token * nh + head of Q [B, L*nh, hd],
    one K / V head [B, Lp, hd]) and, computed once and shared, its float64 reference in the same layout"""

    def __init__(self, jid, hd, nh, cap, mode):
        geo = JOINT[jid]
        self.jid, self.hd, self.nh, self.cap, self.mode = jid, hd, nh, float(cap), mode
        self.P, self.C, self.Hc, self.cnt = geo["P"], geo["C"], geo["Hc"], list(geo["cnt"])
        self.B, self.L = len(self.cnt), self.P + self.C + self.Hc
        self.Lp = (self.L + 7) // 8 * 8
        self.nq = self.L * nh
        self.scale = 1 / math.sqrt(hd)
        B, L, Lp = self.B, self.L, self.Lp
        g = _gen(jid, hd, nh)
        self.Q = _randn(g, B, L * nh, hd, scale=2.0)
        self.K = torch.full((B, Lp, hd), NAN, device=dev, dtype=BF16)
        self.V = torch.full((B, Lp, hd), NAN, device=dev, dtype=BF16)
        self.K[:, :L] = _randn(g, B, L, hd, scale=2.0)
        self.V[:, :L] = _randn(g, B, L, hd)
        self.dO = _randn(g, B, L * nh, hd)
        if mode == 1:
            self.cnt_t = torch.tensor(self.cnt, device=dev, dtype=torch.int32)
            allowed, dead = flash_ref.block_mask(self.cnt, self.P, self.C, L)
            # row layout: every token's nh rows share its mask row
            self.allowed = allowed.repeat_interleave(nh, 1).to(dev)
            self.dead = dead.repeat_interleave(nh, 1).to(dev)
            self.dO[self.dead] = 0  # the pad rows' outputs reach nothing downstream in the model
        else:
            self.cnt_t = self.allowed = self.dead = None

    def qkv64(self, K=None, V=None):
        K, V = self.K if K is None else K, self.V if V is None else V
        return self.Q.double()[:, None], K.double()[:, None, :self.L], V.double()[:, None, :self.L]

    @functools.cached_property
    def ref(self):
        """O [B, nq, hd], lse [B, nq], P / t [B, nq, L]"""
        o, lse, p, t = flash_ref.attention(*self.qkv64(), self.scale, self.cap, self.allowed, self.dead)
        return dict(O=o[:, 0], lse=lse[:, 0], P=p[:, 0], t=None if t is None else t[:, 0])

    @functools.cached_property
    def grads(self):
        """dQ [B, nq, hd], dK / dV [B, L, hd], delta [B, nq] and its bound (module docstring)"""
        dO = self.dO.double()
        dq, dk, dv = flash_ref.attention_grads(*self.qkv64(), dO[:, None], self.scale, self.cap, self.allowed,
                                               self.dead)
        r = self.ref
        delta = (dO * r["O"]).sum(-1)
        tol = 2.0 ** -7 * (dO.abs() * (r["P"] @ self.V.double()[:, :self.L].abs())).sum(-1) + 1e-6
        return dict(dQ=dq[:, 0], dK=dk[:, 0], dV=dv[:, 0], delta=delta, delta_tol=tol)

    def spans(self, n_groups):
        """(first token, tokens) of the output groups: 3 = vlm / proprio / action as Engine._joint_flash builds them"""
        P, C, Hc = self.P, self.C, self.Hc
        return {3: [(0, P), (P, C), (P + C, Hc)], 2: [(0, P), (P, C + Hc)], 1: [(0, self.L)]}[n_groups]

    def rows(self, spans):
        """the query rows of the tokens in spans (contiguous)"""
        return slice(spans[0][0] * self.nh, (spans[-1][0] + spans[-1][1]) * self.nh)


@functools.lru_cache(maxsize=None)
def case(jid, hd=256, nh=8, cap=50.0, mode=1):
    return Case(jid, hd, nh, cap, mode)


def out_groups(c, spans):
    """one guarded [B*T, nh*hd] buffer per span and the groups list of ops.flash_args (rows relative to the first)"""
    bufs = [Guarded(c.B * T, c.nh * c.hd) for _, T in spans]
    tok0 = spans[0][0]
    return bufs, [((off - tok0) * c.nh, b.t, T * c.nh * c.hd, c.hd) for (off, T), b in zip(spans, bufs)]


def gather(c, bufs, spans, what):
    for i, b in enumerate(bufs):
        b.check(f"{what} group {i}")
    return torch.cat([b.t.view(c.B, T * c.nh, c.hd) for (_, T), b in zip(spans, bufs)], 1)


def do_groups(c, spans, dO=None):
    dO = c.dO if dO is None else dO
    return [dO[:, off * c.nh:(off + T) * c.nh].reshape(c.B * T, c.nh * c.hd).contiguous() for off, T in spans]


def jargs(c, spans, groups, lse=None, key_split=False, K=None, V=None, **kw):
    K, V = c.K if K is None else K, c.V if V is None else V
    hd, Lp = c.hd, c.Lp
    rows = c.rows(spans)
    Q = c.Q[:, rows].contiguous()
    nq = Q.shape[1]
    mask = dict(mask_mode=1, cnt=c.cnt_t, prefix=c.P, cond=c.C, mask_row0=rows.start) if c.mode == 1 else {}
    a = _ops().flash_args(c.B, 1, nq, c.L, hd, Q, (hd, nq * hd, 0), K, (hd, Lp * hd, 0), V, (hd, Lp * hd, 0), groups,
                          0, lse, c.scale, cap=c.cap, rows_per_token=c.nh, key_split=key_split, **mask, **kw)
    a.keep = (Q, K, V, groups, lse, kw)  # the struct holds raw pointers: its operands live as long as it does
    return a


def G(jid, hd=256, nh=8, cap=50.0, mode=1):
    """the arguments of case() as one parametrize value"""
    return (jid, hd, nh, float(cap), mode)


def _id(v):
    if isinstance(v, tuple):
        jid, hd, _, cap, mode = v
        return jid + (f"-hd{hd}" if hd != 256 else "") + ("" if (cap, mode) == (50.0, 1) else f"-cap{cap:g}-mask{mode}")
    if isinstance(v, dict):
        return "-".join(f"{k[9:]}{x}" for k, x in v.items()) or "default"
    return str(v)


J15 = [G(f"J{i}") for i in range(1, 6)]
J16 = J15 + [G("J6")]
TINY = [G("J7", 16, 2), G("J7", 32, 2)]
VARIANTS = [G("J3", cap=0.0, mode=1), G("J3", cap=50.0, mode=0), G("J3", cap=0.0, mode=0)]  # part F


# ------------------------------------------------------------------------------------------- A, B: pz_flash_fwd --
def run_fwd(c, spans, key_split, K=None, V=None):
    bufs, groups = out_groups(c, spans)
    rows = c.rows(spans)
    lse = Guarded(c.B, rows.stop - rows.start, torch.float32)
    _ops().flash_fwd(jargs(c, spans, groups, lse.t, key_split, K, V))
    O = gather(c, bufs, spans, "O")
    lse.check("lse")
    return O, lse.t


def check_fwd(c, spans, key_split):
    O, lse = run_fwd(c, spans, key_split)
    rows = c.rows(spans)
    first = 0
    for off, T in spans:  # O per group
        sl = slice(first, first + T * c.nh)
        close(O[:, sl], c.ref["O"][:, rows][:, sl])
        first = sl.stop
    close(lse, c.ref["lse"][:, rows], rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("key_split", [False, True])
@pytest.mark.parametrize("key,n_groups", [(k, 3) for k in J16 + TINY + VARIANTS] +
                         [(G(j), n) for j in ("J1", "J4") for n in (1, 2)], ids=_id)
def test_fwd(key, n_groups, key_split):
    """pz_flash_fwd, O per output group and lse; the key split takes effect only with few workgroups and more than
    one key block (J3..J6), and both ways must match"""
    c = case(*key)
    check_fwd(c, c.spans(n_groups), key_split)


@pytest.mark.parametrize("key_split", [False, True])
@pytest.mark.parametrize("rows", ["action", "proprio+action"])
@pytest.mark.parametrize("key", [G("J1"), G("J3"), G("J4")], ids=_id)
def test_fwd_denoise(key, rows, key_split):
    """the inference forms: only the action rows query (mask_row0 = first action row, one group), or the proprio
    and action rows (mask_row0 = first proprio row, two groups), over all L keys"""
    c = case(*key)
    check_fwd(c, c.spans(3)[2:] if rows == "action" else c.spans(3)[1:], key_split)


# ------------------------------------------------------------------------------------- C: pz_flash_fwd_probs --
def run_probs(c, n_groups=3, want_tc=True, K=None, V=None, expect_error=None):
    spans = c.spans(n_groups)
    bufs, groups = out_groups(c, spans)
    Pm = Guarded(c.B * c.nq, c.Lp)
    tc = Guarded(c.B * c.nq, c.Lp) if want_tc else None
    a = jargs(c, spans, groups, None, False, K, V)
    if expect_error is not None:
        from pizero_native._lib import NativeError

        with pytest.raises(NativeError, match=expect_error):
            _ops().flash_fwd_probs(a, Pm.t, None if tc is None else tc.t, c.Lp)
        torch.cuda.synchronize()
        for b in bufs + [Pm, tc]:
            b.untouched("flash_fwd_probs")
        return None
    _ops().flash_fwd_probs(a, Pm.t, None if tc is None else tc.t, c.Lp)
    O = gather(c, bufs, spans, "O")
    Pm.check("P")
    if tc is not None:
        tc.check("tcap")
    return O, Pm.t.view(c.B, c.nq, c.Lp), None if tc is None else tc.t.view(c.B, c.nq, c.Lp)


@pytest.mark.parametrize("key,want_tc", [(k, "tcap") for k in J15] + [(G("J3"), "no-tcap")] +
                         [(k, "tcap" if k[3] > 0 else "no-tcap") for k in VARIANTS], ids=_id)
def test_fwd_probs(key, want_tc):
    """pz_flash_fwd_probs: O, the exported bf16 softmax P and tanh(s / cap) (dead rows uniform 1 / L with tcap 0,
    exact zeros in the pad columns [L, Lp)); without soft-cap there is no tanh to export"""
    c = case(*key)
    L = c.L
    O, Pm, tc = run_probs(c, 3, want_tc == "tcap")
    r = c.ref
    close(O, r["O"])
    close(Pm[..., :L], r["P"], rtol=1e-2, atol=1e-3)
    assert bool((Pm[..., L:] == 0).all())
    assert (Pm.float().sum(-1) - 1).abs().max().item() < 2e-2  # rows sum to 1 within bf16 rounding
    if tc is not None:
        close(tc[..., :L], r["t"], rtol=1e-2, atol=2e-3)
        assert bool((tc[..., L:] == 0).all())
    if c.dead is not None and bool(c.dead.any()):
        assert (Pm[..., :L][c.dead].float() - 1.0 / L).abs().max().item() <= 2.0 ** -9 / L  # bf16(1 / L)
        if tc is not None:
            assert bool((tc[c.dead] == 0).all())


def test_fwd_probs_rejects_more_than_320_keys():
    """J6 (L = 321): an invalid-argument error naming nk, before any launch"""
    run_probs(case("J6"), expect_error=r"\bnk\b")


# ---------------------------------------------------------------------------------------- D: pz_flash_bwd_ds --
def run_ds(c, Pm, tc, dgroups, want_dq, expect_error=None):
    spans = c.spans(3)
    bufs, groups = out_groups(c, spans)  # (O is not read: only the groups' geometry and their dO)
    dS = Guarded(c.B * c.nq, c.Lp)
    dQ = Guarded(c.B * c.nq, c.hd) if want_dq else None
    a = jargs(c, spans, groups, None, False, dgroups=dgroups, dq=None if dQ is None else dQ.t)
    if expect_error is not None:
        from pizero_native._lib import NativeError

        with pytest.raises(NativeError, match=expect_error):
            _ops().flash_bwd_ds(a, Pm, tc, dS.t, c.Lp)
        torch.cuda.synchronize()
        dS.untouched("flash_bwd_ds")
        return None
    _ops().flash_bwd_ds(a, Pm, tc, dS.t, c.Lp)
    dS.check("dS")
    if dQ is not None:
        dQ.check("dQ")
    return dS.t.view(c.B, c.nq, c.Lp), None if dQ is None else dQ.t.view(c.B, c.nq, c.hd)


@pytest.mark.parametrize("key,skip_action", [(k, False) for k in J15 + VARIANTS] + [(G("J4"), True)], ids=_id)
def test_bwd_ds(key, skip_action):
    """pz_flash_bwd_ds on the P / tanh(cap) that pz_flash_fwd_probs exported: dS on every row against the float64
    softmax backward of the same P / t with dP = dO V^T, zeros in [L, Lp); with dq set the same dS and dQ = dS K;
    a group without dO (the last layer's skipped mixture) contributes dP = 0"""
    c = case(*key)
    L = c.L
    _, Pm, tc = run_probs(c, 3, c.cap > 0)
    dO = c.dO.clone()
    dgroups = do_groups(c, c.spans(3), dO)
    if skip_action:
        off = c.spans(3)[2][0]
        dO[:, off * c.nh:] = 0
        dgroups[2] = None
    dP = dO.double() @ c.V.double()[:, :L].transpose(1, 2)
    ref = flash_ref.softmax_bwd_ds(Pm.double()[..., :L], None if tc is None else tc.double()[..., :L], dP, c.scale,
                                   c.cap)
    dS, _ = run_ds(c, Pm, tc, dgroups, False)
    close(dS[..., :L], ref, rtol=2e-2, atol=2e-2 * ref.abs().max().item() / 8)
    assert bool((dS[..., L:] == 0).all())
    dS2, dQ = run_ds(c, Pm, tc, dgroups, True)
    assert torch.equal(dS2, dS)
    refq = ref @ c.K.double()[:, :L]
    close(dQ, refq, rtol=2e-2, atol=2e-2 * refq.abs().max().item() / 8)


def test_bwd_ds_rejects_more_than_320_keys():
    c = case("J6")
    Pm = torch.zeros(c.B, c.nq, c.Lp, device=dev, dtype=BF16)
    run_ds(c, Pm, torch.zeros_like(Pm), do_groups(c, c.spans(3)), False, expect_error=r"\bnk\b")


# ------------------------------------------------------------------------------------------- E: pz_flash_bwd --
@pytest.mark.parametrize("workspace", [True, False])
@pytest.mark.parametrize("key", J16 + TINY + VARIANTS, ids=_id)
def test_bwd(key, workspace):
    """pz_flash_fwd then pz_flash_bwd: dQ, dK, dV and delta = rowsum(dO * O), with the workspace (the dK / dV pass
    split over the query rows, up to 8 ways at these sizes) and without it (one pass, splits == 1).  dK / dV rows
    [L, Lp) are left untouched: the dK / dV kernels return at key >= nk."""
    c = case(*key)
    B, L, Lp, hd = c.B, c.L, c.Lp, c.hd
    spans = c.spans(3)
    bufs, groups = out_groups(c, spans)
    lse = Guarded(B, c.nq, torch.float32)
    delta = Guarded(B, c.nq, torch.float32)
    dQ, dK, dV = Guarded(B * c.nq, hd), Guarded(B * Lp, hd), Guarded(B * Lp, hd)
    a = jargs(c, spans, groups, lse.t, False, dgroups=do_groups(c, spans), delta=delta.t, dq=dQ.t, dk=dK.t, dv=dV.t)
    if not workspace:
        a.ws = None
        a.ws_bytes = 0
    _ops().flash_fwd(a)
    _ops().flash_bwd(a)
    gather(c, bufs, spans, "O")
    pad = (torch.arange(B * Lp, device=dev) % Lp) >= L
    for buf, what in ((lse, "lse"), (delta, "delta"), (dQ, "dQ")):
        buf.check(what)
    dK.check("dK", untouched=pad)
    dV.check("dV", untouched=pad)
    g = c.grads
    close(dQ.t.view(B, c.nq, hd), g["dQ"], atol=3e-2 * g["dQ"].abs().max().item() / 4)
    close(dK.t.view(B, Lp, hd)[:, :L], g["dK"], atol=3e-2 * g["dK"].abs().max().item())
    close(dV.t.view(B, Lp, hd)[:, :L], g["dV"], atol=3e-2 * g["dV"].abs().max().item())
    err = (delta.t.double() - g["delta"]).abs()
    assert bool((err <= g["delta_tol"]).all()), f"delta: max err {err.max().item():.4g}"


# -------------------------------------------------------------------------------------- G: pz_flash_bwd_prep --
def _check_delta(delta, O, dO):
    """delta [rows] against float64 rowsum(dO * O) of [rows, hd] operands (bound: module docstring)"""
    prod = O.double() * dO.double()
    err = (delta.double() - prod.sum(-1)).abs()
    assert bool((err <= 2e-5 * prod.abs().sum(-1)).all()), f"delta: max err {err.max().item():.4g}"


@pytest.mark.parametrize("key", [G("J1"), G("J4")], ids=_id)
def test_bwd_prep_joint(key):
    """pz_flash_bwd_prep over three output groups (the proprio group: 8 rows inside a 16-row tile)"""
    c = case(*key)
    spans = c.spans(3)
    g = _gen("prep", c.jid)
    O = _randn(g, c.B, c.nq, c.hd)
    og = do_groups(c, spans, O)
    dg = do_groups(c, spans)
    delta = Guarded(c.B, c.nq, torch.float32)
    groups = [(off * c.nh, o, T * c.nh * c.hd, c.hd) for (off, T), o in zip(spans, og)]
    _ops().flash_bwd_prep(jargs(c, spans, groups, None, False, dgroups=dg, delta=delta.t))
    delta.check("delta")
    _check_delta(delta.t.reshape(-1), O.view(-1, c.hd), c.dO.view(-1, c.hd))


def test_bwd_prep_siglip_layout():
    """pz_flash_bwd_prep with heads strided inside the O / dO rows (o_hstride = hd), head dim 72"""
    B, nh, hd, N = 2, 3, 72, 40
    g = _gen("prep-siglip")
    qkv = _randn(g, B * N, 3 * nh * hd)
    O, dO = _randn(g, B * N, nh * hd), _randn(g, B * N, nh * hd)
    delta = Guarded(B * nh, N, torch.float32)
    _ops().flash_bwd_prep(_ops().siglip_flash_args(qkv, O, None, B, nh, hd, N, dO=dO, delta=delta.t))
    delta.check("delta")
    rows = lambda x: x.view(B, N, nh, hd).permute(0, 2, 1, 3).reshape(-1, hd)  # noqa: E731
    _check_delta(delta.t.reshape(-1), rows(O), rows(dO))


# ----------------------------------------------------------------------------------------- H: SigLIP layout --
@pytest.mark.parametrize("hd,nh,N,env", [
    (72, 3, 200, {"PZ_FLASH_UNIT": "1"}),  # resident, one workgroup per unit, ragged
    (72, 3, 200, {"PZ_FLASH_UNIT": "0"}),  # resident, 2 / 4 workgroups per unit
    (72, 3, 256, {"PZ_FLASH_RESIDENT": "0"}),  # generic head dim 72
    (72, 2, 264, {}),  # generic: N > 256
    (32, 4, 40, {}), (32, 2, 264, {}), (16, 4, 40, {}), (16, 2, 264, {}),
], ids=_id)
def test_siglip_layout(hd, nh, N, env, monkeypatch):
    """forward and backward in place on fused q|k|v rows, no mask, no soft-cap: O, lse, dQ, dK, dV"""
    ops = _ops()
    for k in ("PZ_FLASH_UNIT", "PZ_FLASH_RESIDENT", "PZ_FLASH_SIG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = 2
    g = _gen("siglip", hd, nh, N)
    qkv = _randn(g, B * N, 3 * nh * hd, scale=1.5)
    dO = _randn(g, B * N, nh * hd)
    O = Guarded(B * N, nh * hd)
    lse = Guarded(B * nh, N, torch.float32)
    delta = Guarded(B * nh, N, torch.float32)
    dqkv = Guarded(B * N, 3 * nh * hd)
    ops.flash_fwd(ops.siglip_flash_args(qkv, O.t, lse.t, B, nh, hd, N))
    ops.flash_bwd(ops.siglip_flash_args(qkv, O.t, lse.t, B, nh, hd, N, dO=dO, delta=delta.t, dqkv=dqkv.t))
    for buf, what in ((O, "O"), (lse, "lse"), (delta, "delta"), (dqkv, "dqkv")):
        buf.check(what)
    x = qkv.double().view(B, N, 3, nh, hd).permute(2, 0, 3, 1, 4)  # [3, B, nh, N, hd]
    go = dO.double().view(B, N, nh, hd).permute(0, 2, 1, 3)
    ro, rlse, _, _ = flash_ref.attention(x[0], x[1], x[2], hd ** -0.5)
    close(O.t.view(B, N, nh, hd).permute(0, 2, 1, 3), ro)
    close(lse.t.view(B, nh, N), rlse, rtol=1e-3, atol=1e-3)
    got = dqkv.t.view(B, N, 3, nh, hd).permute(2, 0, 3, 1, 4)
    for out, ref in zip(got, flash_ref.attention_grads(x[0], x[1], x[2], go, hd ** -0.5)):
        close(out, ref, rtol=3e-2, atol=3e-2 * ref.abs().max().item() / 4)


# ---------------------------------------------------------------------------------------- I: pz_flash_fwd_f8 --
def _deq(q, s):
    """codes uint8 -> fp32 values times scale (per-row [R] or scalar)"""
    v = q.view(torch.float8_e4m3fn).float()
    return v * (s[:, None] if torch.is_tensor(s) else s)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("key_split", [False, True])
@pytest.mark.parametrize("P", [8, 127, 128])
def test_fwd_f8(P, key_split):
    """the fp8 prefill attention with prefix-only queries at nk = 9, 128 and 129 against its 128-key block: the
    dequantised float64 reference and the bf16 kernel, with test_fp8_gpu.py::test_flash_fwd_f8's bounds"""
    ops = _ops()
    C, nh, hd = 1, 8, 256
    cnt = [P, max(1, P // 2)]
    B, L = len(cnt), P + C
    Lp = (L + 3 + 7) // 8 * 8  # the cache rows past the prefix (the action rows) hold stale data: NaN here
    g = _gen("f8", P)
    Q = _randn(g, B, L * nh, hd, scale=2.0)
    K = _randn(g, B, Lp, hd, scale=2.0)
    V = _randn(g, B, Lp, hd)
    K[:, L:] = NAN
    V[:, L:] = NAN
    cnt_t = torch.tensor(cnt, device=dev, dtype=torch.int32)

    def run(fn, *extra):
        Ov, Oe = Guarded(B * P, nh * hd), Guarded(B * C, nh * hd)
        a = ops.flash_args(B, 1, L * nh, L, hd, Q, (hd, L * nh * hd, 0), K, (hd, Lp * hd, 0), V, (hd, Lp * hd, 0),
                           [(0, Ov.t, P * nh * hd, hd), (P * nh, Oe.t, C * nh * hd, hd)], 0, None, 1 / math.sqrt(hd),
                           cap=50.0, mask_mode=1, cnt=cnt_t, prefix=P, cond=C, rows_per_token=nh,
                           key_split=key_split)
        fn(a, *extra)
        Ov.check("O vlm")
        Oe.check("O proprio")
        return torch.cat([Ov.t.view(B, P * nh, hd), Oe.t.view(B, C * nh, hd)], 1).float()

    qc = torch.empty(B * L * nh, hd, device=dev, dtype=torch.uint8)
    qs = torch.empty(B * L * nh, device=dev, dtype=torch.float32)
    ops.fp8_quant_rows(Q.reshape(-1, hd), qc, qs)
    kc = torch.empty(B * Lp, hd, device=dev, dtype=torch.uint8)
    ks = torch.empty(B * Lp, device=dev, dtype=torch.float32)
    ops.fp8_quant_rows(K.reshape(-1, hd), kc, ks)
    vt = torch.empty(B, hd, (L + 127) // 128 * 128, device=dev, dtype=torch.uint8)
    vs = torch.empty(B, hd, device=dev, dtype=torch.float32)
    ops.fp8_quant_vt(V, B, L, vt, vs)
    got = run(ops.flash_fwd_f8, qc, qs, kc, ks, Lp, vt, vs)
    qd = _deq(qc, qs).view(B, L * nh, hd).double()
    kd = _deq(kc, ks).view(B, Lp, hd)[:, :L].double()
    vd = (vt[:, :, :L].view(torch.float8_e4m3fn).float() * vs[:, :, None]).transpose(1, 2).double()
    allowed, dead = flash_ref.block_mask(cnt, P, C, L)
    ref = flash_ref.attention(qd[:, None], kd[:, None], vd[:, None], 1 / math.sqrt(hd), 50.0,
                              allowed.repeat_interleave(nh, 1).to(dev), dead.repeat_interleave(nh, 1).to(dev))[0][:, 0]
    bf = run(ops.flash_fwd)
    print(f"[fp8 attention P={P}] rel-L2 vs dequantised fp64 {_rel(got, ref):.4f}, vs the bf16 kernel {_rel(got, bf):.4f}")
    assert _rel(got, ref) <= 3e-2, _rel(got, ref)
    assert _rel(got, bf) <= 0.15, _rel(got, bf)


# ----------------------------------------------------------------------------- J: masked keys are inert, bitwise --
@pytest.mark.parametrize("kernel", ["fwd", "fwd-key-split", "probs"])
def test_masked_keys_inert(kernel):
    """J4: a masked key has p exactly 0, so overwriting K / V at the pad keys [cnt_b, P) of every sample must leave
    O and lse / P of every live row bitwise unchanged (dead rows attend to those keys by design)"""
    c = case("J4")
    g = _gen("inert")
    K2, V2 = c.K.clone(), c.V.clone()
    for b, n in enumerate(c.cnt):
        K2[b, n:c.P] = _randn(g, c.P - n, c.hd, scale=100.0)
        V2[b, n:c.P] = _randn(g, c.P - n, c.hd, scale=100.0)
    live = ~c.dead
    if kernel == "probs":
        first, second = run_probs(c)[:2], run_probs(c, K=K2, V=V2)[:2]
    else:
        first = run_fwd(c, c.spans(3), kernel == "fwd-key-split")
        second = run_fwd(c, c.spans(3), kernel == "fwd-key-split", K2, V2)
    for x, y in zip(first, second):
        assert torch.equal(x[live], y[live])
    ra = flash_ref.attention(*c.qkv64(), c.scale, c.cap, c.allowed, c.dead)
    rb = flash_ref.attention(*c.qkv64(K2, V2), c.scale, c.cap, c.allowed, c.dead)
    for x, y in zip(ra[:3], rb[:3]):
        assert torch.equal(x[:, 0][live], y[:, 0][live])
