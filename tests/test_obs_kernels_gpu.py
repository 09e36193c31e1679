"""pz_image_resize_norm, pz_proprio_normalize and pz_action_denormalize on the MI355X.

Resize against the fp64 restatement (tests/obs_ref.py): every pixel's decoded code q satisfies
|q - clip(v, 0, 255)| <= 0.5 + 0.01, v the restatement's unrounded value.  The 0.01 bounds the fp32 accumulation: two
passes of <= ~20 taps with sum |w| <= 1.4 on values <= 255 contribute about 20 * 2^-24 * 1.4 * 255 = 4e-4 each, below
2e-3 after propagation -- a margin of about 5x.  The criterion is on v and not on equal codes because about 2 % of
pixels lie within 0.01 of a rounding boundary; no share of pixels is exempted.  On input already at the output size
the result equals today's torch expression bit for bit.  The normalisation kernels are held to the fp64 formulas on the
fp32 inputs within 2e-5 (|x| <= 4, hi - lo >= 0.1: ulp(4) * 2 / 0.1 = 1e-5, doubled).
"""

import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import obs_ref as R
from tests.conftest import ROOT
from tests.oracle_helpers import load_golden

pytestmark = pytest.mark.gpu

TOL = 0.5 + 0.01
ATOL = 2e-5
GEOMETRIES = [(37, 53, 56), (131, 97, 56), (57, 55, 56), (56, 56, 56)]
CONTENTS = ("noise", "zeros", "full", "checker")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _frames(kind, n, h, w):
    if kind == "noise":
        return np.random.default_rng(h * 7 + w * 3 + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((n, h, w, 3), np.uint8)
    if kind == "full":
        return np.full((n, h, w, 3), 255, np.uint8)
    return R.checkerboard(n, h, w, 3)


@functools.lru_cache(maxsize=None)
def _reference(kind, n, h, w, S):
    """(frames uint8 [n, h, w, 3], v fp64 [n, 3, S, S]) -- computed once per case, shared by both layouts"""
    x = _frames(kind, n, h, w)
    v, _ = R.resize(x, S)
    x.setflags(write=False)
    v.setflags(write=False)
    return x, v


def _decode(out):
    """bf16 [n, 3, S, S] -> the uint8 code each value stands for (every value must be one of the 256 table entries)"""
    from pizero_native import ops

    lut = ops.pixel_code_lut(out.device).float()
    assert bool((lut[1:] > lut[:-1]).all())
    o = out.float()
    idx = torch.searchsorted(lut, o.contiguous()).clamp_(0, 255)
    assert torch.equal(lut[idx], o), "an output value is not in the code table"
    return idx.cpu().numpy().astype(np.float64)


def _check(kind, n, h, w, S):
    from pizero_native import ops

    x, v = _reference(kind, n, h, w, S)
    want = np.clip(v, 0, 255)
    for cl in (True, False):
        fr = torch.from_numpy(x.copy() if cl else np.ascontiguousarray(x.transpose(0, 3, 1, 2))).cuda()
        out = ops.image_resize_norm(fr, S, channels_last=cl)
        assert out.shape == (n, 3, S, S) and out.dtype == torch.bfloat16
        err = np.abs(_decode(out) - want)
        print(f"{kind:8s} n={n} {h}x{w}->{S} channels_last={cl}: max |q - clip(v)| = {err.max():.6f}")
        assert err.max() <= TOL, (kind, n, h, w, cl, err.max(), int((err > TOL).sum()))
    return v


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w,S", GEOMETRIES)
def test_resize_matches_the_restatement(h, w, S, n):
    for kind in CONTENTS:
        v = _check(kind, n, h, w, S)
        if kind == "checker" and (h, w) != (S, S):  # the fixture does reach the clip on both sides
            assert v.min() < -1 and v.max() > 256, (v.min(), v.max())


@pytest.mark.parametrize("kind", CONTENTS)
def test_resize_deployment_shape(kind):
    _check(kind, 1, 480, 640, 224)


@pytest.mark.parametrize("S", [56, 224])
def test_resize_identity_is_todays_expression_bit_for_bit(S):
    from pizero_native import ops

    x = torch.randint(0, 256, (2, 3, S, S), dtype=torch.uint8, generator=torch.Generator().manual_seed(S))
    x[0, :, :4, :4] = torch.tensor([0, 255, 127, 128], dtype=torch.uint8)
    # the expression as the host evaluates it (what a host-normalised frame carries into infer_chunk); PyTorch's
    # device evaluation divides by 255 as a multiplication by the reciprocal and differs in a few codes by one ulp
    want = ((x.float() / 255 - 0.5) / 0.5).to(torch.bfloat16).cuda()
    x = x.cuda()
    on_dev = ((x.float() / 255 - 0.5) / 0.5).to(torch.bfloat16)
    print(f"S={S}: the device evaluation of the expression differs from the host's in "
          f"{int((on_dev != want).sum())} of {want.numel()} elements, codes {x[on_dev != want].unique().tolist()}")
    got = ops.image_resize_norm(x, S, channels_last=False)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    got_cl = ops.image_resize_norm(x.permute(0, 2, 3, 1).contiguous(), S, channels_last=True)
    assert torch.equal(got_cl.view(torch.int16), want.view(torch.int16))


def test_resize_wrapper_refusals():
    from pizero_native import ops

    with pytest.raises(ValueError, match="PZ_OBS_MAX_TAPS"):
        ops.image_resize_norm(torch.zeros(1, 700, 60, 3, dtype=torch.uint8, device="cuda"), 56)
    with pytest.raises(ValueError, match="3 channels"):
        ops.image_resize_norm(torch.zeros(1, 60, 60, 4, dtype=torch.uint8, device="cuda"), 56)


def _stat_sets():
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")))
    g = load_golden("obs_norm")
    p, a = s["proprio"], s["action"]
    return {"bridge": dict(x=g["proprio_raw"], y=g["action_norm"], plo=p["p01"], phi=p["p99"], pm=p["mean"],
                           ps=p["std"], alo=a["p01"], ahi=a["p99"], am=a["mean"], as_=a["std"]),
            "synth": dict(x=g["synth/x"], y=g["synth/a"], plo=g["synth/lo"], phi=g["synth/hi"], pm=g["synth/mean"],
                          ps=g["synth/std"], alo=g["synth/lo"], ahi=g["synth/hi"], am=g["synth/mean"],
                          as_=g["synth/std"])}


def _f32(a):
    return torch.tensor(np.asarray(a, np.float64)).to(torch.float32).cuda()


@pytest.mark.parametrize("tag", ["bridge", "synth"])
def test_normalise_and_denormalise_match_the_fp64_formulas(tag):
    """fp64 formulas on the fp32 inputs (statistics included: the kernel sees them as fp32)"""
    from pizero_native import ops

    t = _stat_sets()[tag]
    x, y = _f32(t["x"]), _f32(t["y"])
    st = {k: _f32(t[k]) for k in ("plo", "phi", "pm", "ps", "alo", "ahi", "am", "as_")}
    h = lambda z: z.double().cpu().numpy()  # noqa: E731
    xr = h(x)
    assert ((xr < h(st["plo"])) | (xr > h(st["phi"]))).any()  # values outside [p01, p99]: the clip is hit
    got = h(ops.proprio_normalize(x, st["plo"], st["phi"], "bound"))
    want = R.normalize_bound(xr, h(st["plo"]), h(st["phi"]))
    assert (want == 1).any() and (want == -1).any()
    assert np.abs(got - want).max() <= ATOL, np.abs(got - want).max()
    assert got.min() >= -1 and got.max() <= 1
    got = h(ops.proprio_normalize(x.view(8, 8, 7), st["pm"], st["ps"], "gaussian")).reshape(64, 7)
    want = R.normalize_gaussian(xr, h(st["pm"]), h(st["ps"]))
    assert np.abs(got - want).max() <= ATOL, np.abs(got - want).max()
    for mode, a, b, fn in (("bound", st["alo"], st["ahi"], R.denormalize_bound),
                           ("gaussian", st["am"], st["as_"], R.denormalize_gaussian)):
        for n_pass in (1, 0, 3):
            out = ops.action_denormalize(y.view(16, 4, 7), a, b, mode, n_pass=n_pass).view(64, 7)
            k = 7 - n_pass
            want = fn(h(y)[:, :k], h(a)[:k], h(b)[:k])
            assert np.abs(h(out)[:, :k] - want).max() <= ATOL, (mode, n_pass, np.abs(h(out)[:, :k] - want).max())
            # the trailing dimensions (the gripper) pass through bit for bit
            assert torch.equal(out[:, k:].contiguous().view(torch.int32), y[:, k:].contiguous().view(torch.int32))
    # in place
    z = x.clone()
    ops.proprio_normalize(z, st["plo"], st["phi"], "bound", out=z)
    assert torch.equal(z, ops.proprio_normalize(x, st["plo"], st["phi"], "bound"))
    with pytest.raises(ValueError):
        ops.proprio_normalize(x, st["plo"], st["phi"], "minmax")
