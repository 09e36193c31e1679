"""pz_image_augment and pz_image_resize_u8 on the MI355X.

The kernel's decoded code q against the fp64 restatement's unquantised value x (tests/augment_ref.py), for every pixel:

    |q + 0.5 - min(255.5 x, 255.5)| <= 0.5 + 0.01

q = floor(255.5 x) puts 255.5 x in [q, q + 1), i.e. within 0.5 of q + 0.5; the 0.01 accepts the neighbouring code only
within 0.01 of a code boundary.  Basis: a float32 evaluation of the same chain differs from fp64 by at most 1e-3 of a
code over these contents and corner parameters (test_augment_host.py measures 2.3e-4 at S = 33), so 0.01 leaves a factor
of ten for the hardware's fused multiply-adds and summation order -- the criterion and margin of
test_obs_kernels_gpu.py.  No share of pixels is exempted.
"""

import numpy as np
import pytest
import torch

from tests import augment_ref as R

pytestmark = pytest.mark.gpu

TOL = 0.5 + 0.01
SHAPES = [(1, 8), (3, 33), (2, 224)]
CONTENTS = ("noise", "zeros", "full", "grey", "primaries", "gradient")
# the smallest boxes of the reference's settings (scale 0.8 at ratio 0.9 and at ratio 1.1), at offset 0 and at the
# largest offset
_H0, _W0 = (0.8 / 0.9) ** 0.5, (0.8 * 0.9) ** 0.5
_H1, _W1 = (0.8 / 1.1) ** 0.5, (0.8 * 1.1) ** 0.5
BOX_A, BOX_B = (0.0, 0.0, _H0, _W0), (1.0 - _H1, 1.0 - _W1, 1.0, 1.0)
FULL = (0.0, 0.0, 1.0, 1.0)
ROWS = [  # (name, parameter row, mask)
    ("identity", R.IDENTITY, R.ALL),
    ("brightness+", (*FULL, 0.1, 1, 1, 0), R.BRIGHTNESS), ("brightness-", (*FULL, -0.1, 1, 1, 0), R.BRIGHTNESS),
    ("contrast-", (*FULL, 0, 0.9, 1, 0), R.CONTRAST), ("contrast+", (*FULL, 0, 1.1, 1, 0), R.CONTRAST),
    ("saturation-", (*FULL, 0, 1, 0.9, 0), R.SATURATION), ("saturation+", (*FULL, 0, 1, 1.1, 0), R.SATURATION),
    ("hue-", (*FULL, 0, 1, 1, -0.05), R.HUE), ("hue+", (*FULL, 0, 1, 1, 0.05), R.HUE),
    ("box at 0", (*BOX_A, 0, 1, 1, 0), R.CROP), ("box at max offset", (*BOX_B, 0, 1, 1, 0), R.CROP),
    ("chain+", (*BOX_A, 0.1, 1.1, 1.1, 0.05), R.ALL), ("chain-", (*BOX_B, -0.1, 0.9, 0.9, -0.05), R.ALL),
    ("hue -0.5", (*FULL, 0, 1, 1, -0.5), R.HUE), ("hue +0.5", (*FULL, 0, 1, 1, 0.5), R.HUE),
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _frames(kind, n, S):
    """uint8 [n, 3, S, S], a different frame per index"""
    rng = np.random.default_rng(S * 31 + n)
    if kind == "noise":
        return rng.integers(0, 256, (n, 3, S, S), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((n, 3, S, S), np.uint8)
    if kind == "full":
        return np.full((n, 3, S, S), 255, np.uint8)
    if kind == "grey":  # zero chroma everywhere
        return np.repeat(rng.integers(0, 256, (n, 1, S, S), dtype=np.uint8), 3, axis=1)
    if kind == "primaries":  # every channel 0 or 255: the hue sits on the sextant boundaries and wraps
        return (rng.integers(0, 2, (n, 3, S, S)) * 255).astype(np.uint8)
    y, x = np.mgrid[0:S, 0:S] / max(S - 1, 1)
    g = np.stack([255 * x, 255 * y, 255 * (1 - 0.5 * x - 0.5 * y)])
    return np.stack([np.roll(g, i, axis=0) for i in range(n)]).round().astype(np.uint8)


def _decode(out):
    """bf16 [n, 3, S, S] -> the uint8 code each value stands for (every value must be one of the 256 table entries)"""
    from pizero_native import ops

    lut = ops.pixel_code_lut(out.device).float()
    o = out.float()
    idx = torch.searchsorted(lut, o.contiguous()).clamp_(0, 255)
    assert torch.equal(lut[idx], o), "an output value is not in the code table"
    return idx.cpu().numpy()


def _both_layouts(x):
    """(channels_last, device frames) for a planar uint8 array [n, 3, S, S]"""
    yield False, torch.from_numpy(x.copy()).cuda()
    yield True, torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("n,S", SHAPES)
def test_augment_matches_the_restatement(n, S, kind):
    from pizero_native import ops

    x = _frames(kind, n, S)
    worst = 0.0
    for name, row, mask in ROWS:
        params = np.tile(np.asarray(row, np.float32), (n, 1))
        masks = np.full(n, mask, np.int32)
        want = np.minimum(255.5 * R.augment(x, params, masks), 255.5)  # computed once, shared by both layouts
        for cl, fr in _both_layouts(x):
            out = ops.image_augment(fr, params, masks, channels_last=cl)
            assert out.shape == (n, 3, S, S) and out.dtype == torch.bfloat16
            err = np.abs(_decode(out) + 0.5 - want)
            worst = max(worst, err.max() - 0.5)
            assert err.max() <= TOL, (kind, n, S, name, cl, err.max(), int((err > TOL).sum()))
    print(f"{kind:9s} n={n} S={S}: max over rows and layouts of |q + 0.5 - min(255.5 x, 255.5)| - 0.5 = {worst:.2e}")


def _mixed(n):
    """a different row and mask for every frame of a batch"""
    pick = [ROWS[(7 * i + 11) % len(ROWS)] for i in range(n)]
    return np.asarray([p[1] for p in pick], np.float32), np.asarray([p[2] for p in pick], np.int32)


@pytest.mark.parametrize("n,S", SHAPES)
def test_identity_gives_the_code_table_bit_for_bit(n, S):
    from pizero_native import ops

    x = _frames("noise", n, S)
    x[0, :, 0, :4] = np.array([0, 255, 127, 128], np.uint8)
    ident = np.tile(np.asarray(R.IDENTITY, np.float32), (n, 1))
    for cl, fr in _both_layouts(x):
        want = ops.pixel_code_lut("cuda")[torch.from_numpy(x.astype(np.int64)).cuda()]
        for mask in (R.ALL, 0):  # every op with parameters that change nothing, and no op at all
            got = ops.image_augment(fr, ident, np.full(n, mask, np.int32), channels_last=cl)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (cl, mask)


@pytest.mark.parametrize("n,S", [(3, 33), (2, 224)])
def test_repeatable_and_independent_of_the_batch(n, S):
    """two runs give the same bits (fixed reduction order, no atomics), and frame i of a batch equals that frame
    launched alone (the partition of the channel sums depends on S only)"""
    from pizero_native import ops

    x = _frames("noise", n, S)
    params, masks = _mixed(n)
    params[:, 5] = np.where(masks & R.CONTRAST, params[:, 5], 1.07)
    masks |= R.CONTRAST  # every frame takes the two-pass path
    for cl, fr in _both_layouts(x):
        a = ops.image_augment(fr, params, masks, channels_last=cl)
        b = ops.image_augment(fr, params, masks, channels_last=cl)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        for i in range(n):
            alone = ops.image_augment(fr[i:i + 1].contiguous(), params[i:i + 1], masks[i:i + 1], channels_last=cl)
            assert torch.equal(alone.view(torch.int16), a[i:i + 1].view(torch.int16)), (cl, i)
        # device-resident parameters (nothing read back: the sums are always taken) give the same bits
        c = ops.image_augment(fr, torch.from_numpy(params).cuda(), torch.from_numpy(masks).cuda(), channels_last=cl)
        assert torch.equal(a.view(torch.int16), c.view(torch.int16))


def test_per_frame_masks_in_one_launch():
    """frames of one launch with different ops, among them frames without the contrast next to frames with it"""
    from pizero_native import ops

    n, S = 7, 33
    x = _frames("noise", n, S)
    params, masks = _mixed(n)
    assert len(set(masks.tolist())) >= 4 and (masks & R.CONTRAST).any() and not (masks & R.CONTRAST).all()
    want = np.minimum(255.5 * R.augment(x, params, masks), 255.5)
    for cl, fr in _both_layouts(x):
        err = np.abs(_decode(ops.image_augment(fr, params, masks, channels_last=cl)) + 0.5 - want)
        assert err.max() <= TOL, (cl, err.max())


@pytest.mark.parametrize("h,w,S", [(37, 53, 56), (131, 97, 56)])  # an upscale and a downscale of the resize tests
def test_resize_u8_is_the_decoded_resize_norm(h, w, S):
    from pizero_native import ops

    x = np.random.default_rng(h * 7 + w * 3).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    for cl in (True, False):
        fr = torch.from_numpy(x.copy() if cl else np.ascontiguousarray(x.transpose(0, 3, 1, 2))).cuda()
        codes = ops.image_resize_u8(fr, S, channels_last=cl)
        assert codes.dtype == torch.uint8 and codes.shape == (2, 3, S, S)
        norm = ops.image_resize_norm(fr, S, channels_last=cl)
        assert np.array_equal(codes.cpu().numpy(), _decode(norm))
        assert torch.equal(ops.pixel_code_lut("cuda")[codes.long()].view(torch.int16), norm.view(torch.int16))


def test_wrapper_refusals():
    from pizero_native import ops

    ident = np.tile(np.asarray(R.IDENTITY, np.float32), (2, 1))
    m = np.zeros(2, np.int32)
    with pytest.raises(ValueError, match="square"):
        ops.image_augment(torch.zeros(2, 3, 8, 9, dtype=torch.uint8, device="cuda"), ident, m)
    fr = torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="params"):
        ops.image_augment(fr, ident[:, :7], m)
    with pytest.raises(ValueError, match="mask"):
        ops.image_augment(fr, ident, m.astype(np.int64))
    with pytest.raises(ValueError, match="PZ_AUG_ALL"):
        ops.image_augment(fr, ident, m + 64)
    with pytest.raises(ValueError, match="3 channels"):
        ops.image_resize_u8(torch.zeros(1, 60, 60, 4, dtype=torch.uint8, device="cuda"), 56)
