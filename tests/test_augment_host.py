"""Training-image augmentation: the parts that need no GPU.

The numpy restatement (tests/augment_ref.py) against independent witnesses (the standard library's colorsys, closed
forms), pizero_native.augment's parsing and counter-based draws, and the C entry points' argument checks, which return
before anything is launched or dereferenced.
"""

import colorsys
import ctypes
import os

import numpy as np
import pytest

from tests import augment_ref as R
from tests.conftest import ROOT

NEW = ("pz_image_augment", "pz_image_augment_scratch_bytes", "pz_image_resize_u8")
PRIMARIES = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)]


def _frame_kinds(S, seed=0):
    rng = np.random.default_rng(seed)
    prim = np.array(PRIMARIES, np.uint8)[rng.integers(0, 8, (S, S))].transpose(2, 0, 1) * 255
    return {"noise": rng.integers(0, 256, (3, S, S), dtype=np.uint8),
            "grey": np.repeat(rng.integers(0, 256, (1, S, S), dtype=np.uint8), 3, axis=0),
            "constant": np.full((3, S, S), 77, np.uint8), "primaries": np.ascontiguousarray(prim)}


# ---- the restatement ------------------------------------------------------------------------------------------
def test_hsv_both_ways_matches_colorsys():
    rng = np.random.default_rng(0)
    px = np.concatenate([rng.random((10000, 3)), np.array(PRIMARIES, np.float64),
                         np.repeat(np.linspace(0, 1, 17)[:, None], 3, axis=1)])
    h, s, v = R.rgb_to_hsv(px.T.copy())
    want = np.array([colorsys.rgb_to_hsv(*p) for p in px])
    # colorsys gives h in [0, 1) too; compare the hue on the circle
    dh = np.abs(h - want[:, 0])
    assert np.minimum(dh, 1 - dh).max() < 1e-12
    assert np.abs(s - want[:, 1]).max() < 1e-12 and np.abs(v - want[:, 2]).max() < 1e-12
    hsv = np.concatenate([rng.random((10000, 3)), np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0.5, 1, 1], [1, 1, 1]])])
    got = R.hsv_to_rgb(*hsv.T.copy()).T
    want = np.array([colorsys.hsv_to_rgb(*p) for p in hsv])
    assert np.abs(got - want).max() < 1e-12


def _solid(rgb, S=4):
    return (np.array(rgb, np.uint8)[:, None, None] * np.ones((1, S, S), np.uint8)) * 255


def test_hue_rotates_the_primaries():
    red = _solid((1, 0, 0))
    row = list(R.IDENTITY)
    row[7] = 1 / 3
    assert np.array_equal(R.quantise(R.augment_frame(red, row, R.HUE)), _solid((0, 1, 0)))
    row[7] = -1 / 3
    assert np.array_equal(R.quantise(R.augment_frame(red, row, R.HUE)), _solid((0, 0, 1)))


def test_saturation_zero_gives_the_maximum_channel():
    q = _frame_kinds(9)["noise"]
    row = list(R.IDENTITY)
    row[6] = 0.0
    x = R.augment_frame(q, row, R.SATURATION)
    mx = q.max(axis=0).astype(np.float64) / 255
    assert np.abs(x - mx[None]).max() < 1e-15


def test_contrast_zero_gives_the_mean_and_one_is_the_identity():
    q = _frame_kinds(9)["noise"]
    row = list(R.IDENTITY)
    row[5] = 0.0
    x = R.augment_frame(q, row, R.CONTRAST)
    m = (q.astype(np.float64) / 255).mean(axis=(1, 2))
    assert np.abs(x - m[:, None, None]).max() < 1e-15
    row[5] = 1.0
    assert np.abs(R.augment_frame(q, row, R.CONTRAST) - q / 255).max() < 1e-15


def test_brightness_extremes():
    q = _frame_kinds(9)["noise"]
    for d, code in ((1.0, 255), (-1.0, 0)):
        row = list(R.IDENTITY)
        row[4] = d
        assert (R.quantise(R.augment_frame(q, row, R.BRIGHTNESS)) == code).all()


@pytest.mark.parametrize("S", [1, 5, 33])
def test_full_box_is_the_identity(S):
    q = _frame_kinds(S)["noise"]
    assert np.array_equal(R.augment_frame(q, R.IDENTITY, R.CROP), q.astype(np.float64) / 255)


def test_half_box_on_a_ramp_is_the_closed_form():
    """codes 10 y + x on 5 x 5 under the box (0, 0, .5, .5): in = i / 2, bilinear on a bilinear image is exact"""
    S = 5
    y, x = np.mgrid[0:S, 0:S]
    q = np.repeat((10 * y + x)[None], 3, axis=0).astype(np.uint8)
    got = R.augment_frame(q, (0, 0, 0.5, 0.5, 0, 1, 1, 0), R.CROP)
    want = (10 * (y / 2) + x / 2) / 255
    assert np.abs(got - want[None]).max() < 1e-15


def test_float_round_trip_of_every_code():
    q = np.arange(256, dtype=np.uint8)
    for dt in (np.float64, np.float32):
        assert np.array_equal(R.quantise(q.astype(dt) / dt(255)), q)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("S", [8, 33])
def test_identity_row_returns_the_input_codes(S, dtype):
    for kind, q in _frame_kinds(S).items():
        got = R.quantise(R.augment_frame(q, R.IDENTITY, R.ALL, dtype))
        assert np.array_equal(got, q), kind


def test_float32_chain_stays_far_inside_the_gpu_criterion():
    """the basis of test_augment_gpu's 0.01: float32 against fp64 over corner parameters, in codes"""
    worst = 0.0
    for kind, q in _frame_kinds(33).items():
        for row in ((0, 0, 0.8, 0.8, 0.1, 1.1, 1.1, 0.05), (0.2, 0.2, 1, 1, -0.1, 0.9, 0.9, -0.05),
                    (0.05, 0.1, 0.95, 0.9, 0.1, 0.9, 1.1, 0.5)):
            d = np.abs(R.augment_frame(q, row, R.ALL, np.float32).astype(np.float64) - R.augment_frame(q, row, R.ALL))
            worst = max(worst, 255.5 * d.max())
    print(f"max |float32 - fp64| = {worst:.2e} codes")
    assert worst < 1e-3


# ---- parsing and draws ------------------------------------------------------------------------------------------
def test_reference_settings_parse():
    from pizero_native import augment as A

    p, w = A.parse_spec(A.REFERENCE_PRIMARY), A.parse_spec(A.REFERENCE_WRIST)
    assert p["mask"] == 31 and w["mask"] == 30 and w["crop"] is None
    assert p["crop"] == (0.8, 1.0, 0.9, 1.1) and p["brightness"] == 0.1 and p["hue"] == 0.05
    assert p["contrast"] == (0.9, 1.1) == p["saturation"]
    # positional crop arguments, keyword jitter arguments
    s = A.parse_spec({"augment_order": ["random_resized_crop", "random_hue"],
                      "random_resized_crop": [[0.5, 1.0], [0.75, 1.25]], "random_hue": {"max_delta": 0.1}})
    assert s["mask"] == 17 and s["crop"] == (0.5, 1.0, 0.75, 1.25) and s["hue"] == 0.1


def test_refusals_name_what_they_refuse():
    from pizero_native import augment as A

    swapped = dict(A.REFERENCE_PRIMARY, augment_order=["random_brightness", "random_resized_crop", "random_contrast",
                                                       "random_saturation", "random_hue"])
    with pytest.raises(ValueError, match="augment_order"):
        A.parse_spec(swapped)
    with pytest.raises(ValueError, match="augment_order"):
        A.parse_spec(dict(A.REFERENCE_WRIST, augment_order=["random_hue", "random_hue", "random_brightness",
                                                            "random_contrast", "random_saturation"]))
    with pytest.raises(ValueError, match="augment_order"):
        A.parse_spec({"random_hue": [0.05]})
    for op in ("random_flip_left_right", "random_flip_up_down", "random_rot90"):
        with pytest.raises(ValueError, match=op):
            A.parse_spec({"augment_order": ["random_brightness", op], "random_brightness": [0.1]})
    with pytest.raises(ValueError, match="random_blur"):
        A.parse_spec({"augment_order": ["random_blur"]})
    with pytest.raises(ValueError, match="random_hue"):
        A.parse_spec({"augment_order": ["random_hue"], "random_hue": [0.7]})
    with pytest.raises(ValueError, match="scale"):
        A.parse_spec({"augment_order": ["random_resized_crop"], "random_resized_crop": {"scale": [0.8, 1.2],
                                                                                       "ratio": [0.9, 1.1]}})
    with pytest.raises(ValueError, match="image_augment_crop_draws"):
        A.draw_params(A.REFERENCE_PRIMARY, 4, 0, 0, 0, crop_draws="both")


def _invert_crop(params, spec):
    """the uniforms behind a box, where neither side was clipped to 1: (keep, u_scale, u_ratio, u_off_y, u_off_x)"""
    p = params.astype(np.float64)
    nh, nw = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    keep = (nh < 0.999) & (nw < 0.999)
    s_lo, s_hi, r_lo, r_hi = spec["crop"]
    us = (nh * nw - s_lo) / (s_hi - s_lo)
    ur = (np.log(nw / nh) - np.log(r_lo)) / (np.log(r_hi) - np.log(r_lo))
    with np.errstate(divide="ignore", invalid="ignore"):  # clipped sides (1 - new = 0) are not kept
        return keep, us, ur, p[:, 0] / (1 - nh), p[:, 1] / (1 - nw)


def test_draw_params_ranges_and_keys():
    import torch

    from pizero_native import augment as A

    np_state, torch_state = np.random.get_state(), torch.get_rng_state()
    spec = A.parse_kwargs(A.REFERENCE_PRIMARY)
    n = 4096
    p, m = A.draw_params(spec, n, seed=7, cnt_batch=3, rank=0)
    assert p.dtype == np.float32 and p.shape == (n, 8) and m.dtype == np.int32 and (m == 31).all()
    y1, x1, y2, x2 = p[:, :4].T
    assert (y1 >= 0).all() and (x1 >= 0).all() and (y2 <= 1).all() and (x2 <= 1).all()
    assert (y2 > y1).all() and (x2 > x1).all()
    area, ratio = (y2 - y1) * (x2 - x1), (x2 - x1) / (y2 - y1)
    unclipped = ((y2 - y1) < 0.999) & ((x2 - x1) < 0.999)
    assert area[unclipped].min() >= 0.8 - 1e-5 and area.max() <= 1 + 1e-6
    assert ratio[unclipped].min() >= 0.9 - 1e-5 and ratio[unclipped].max() <= 1.1 + 1e-5
    f = np.float32  # the bounds as the float32 rows can represent them
    assert (np.abs(p[:, 4]) <= f(0.1)).all() and p[:, 4].min() < -0.09 and p[:, 4].max() > 0.09
    for c in (5, 6):
        assert p[:, c].min() >= f(0.9) and p[:, c].max() <= f(1.1) and p[:, c].min() < 0.91 and p[:, c].max() > 1.09
    assert (np.abs(p[:, 7]) <= f(0.05)).all() and p[:, 7].min() < -0.045 and p[:, 7].max() > 0.045
    # a pure function of (seed, cnt_batch, rank): repeatable, and each key changes the draws
    p2, m2 = A.draw_params(spec, n, seed=7, cnt_batch=3, rank=0)
    assert p.tobytes() == p2.tobytes() and m.tobytes() == m2.tobytes()
    for kw in (dict(seed=7, cnt_batch=4, rank=0), dict(seed=7, cnt_batch=3, rank=1), dict(seed=8, cnt_batch=3, rank=0)):
        q, _ = A.draw_params(spec, n, **kw)
        assert (q != p).mean() > 0.9, kw
    # a shorter batch is a prefix (a frame's draws do not depend on the batch size)
    assert A.draw_params(spec, 16, seed=7, cnt_batch=3, rank=0)[0].tobytes() == p[:16].tobytes()
    # the global generators are untouched
    assert torch.equal(torch.get_rng_state(), torch_state)
    s2 = np.random.get_state()
    assert s2[0] == np_state[0] and np.array_equal(s2[1], np_state[1]) and s2[2:] == np_state[2:]


def test_crop_draws_shared_and_independent():
    from pizero_native import augment as A

    spec = A.parse_kwargs(A.REFERENCE_PRIMARY)
    p, _ = A.draw_params(spec, 2048, seed=1, cnt_batch=0, rank=0)  # "shared" is the default
    keep, us, ur, uy, ux = _invert_crop(p, spec[0])
    assert keep.sum() > 1000
    for other in (ur, uy, ux):  # one u per frame drives all four (float32 boxes: ~1e-5 after the inversion)
        assert np.abs(other[keep] - us[keep]).max() < 1e-3
    q, _ = A.draw_params(spec, 2048, seed=1, cnt_batch=0, rank=0, crop_draws="independent")
    keep, us, ur, uy, ux = _invert_crop(q, spec[0])
    assert keep.sum() > 1000
    for a, b in ((us, ur), (us, uy), (us, ux), (uy, ux)):
        assert abs(np.corrcoef(a[keep], b[keep])[0, 1]) < 0.2
    # the colour draws are the same in both modes
    assert p[:, 4:].tobytes() == q[:, 4:].tobytes()


def test_per_slot_list_is_honoured():
    from pizero_native import augment as A

    specs = A.parse_kwargs([A.REFERENCE_PRIMARY, A.REFERENCE_WRIST])
    assert len(specs) == 2
    p, m = A.draw_params(specs, 6, seed=0, cnt_batch=0, rank=0)
    assert m.tolist() == [31, 30, 31, 30, 31, 30]
    assert (p[1::2, :4] == np.array([0, 0, 1, 1], np.float32)).all()  # the wrist slot has no crop
    assert (p[0::2, 2] - p[0::2, 0] < 1).all()
    one, _ = A.draw_params(A.parse_kwargs(A.REFERENCE_PRIMARY), 6, seed=0, cnt_batch=0, rank=0)
    assert one[0::2].tobytes() == p[0::2].tobytes() and one[1::2, 4:].tobytes() == p[1::2, 4:].tobytes()
    with pytest.raises(ValueError, match="empty"):
        A.parse_kwargs([])


# ---- ABI ------------------------------------------------------------------------------------------------------
def test_abi_declares_exports_and_binds_the_entry_points():
    import pizero_native
    from pizero_native import _lib
    from tests.test_abi import declared_symbols

    syms = declared_symbols()
    L = pizero_native.lib()
    for s in NEW:
        assert s in syms, f"{s} not declared in include/pz_abi.h"
        assert hasattr(L, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    assert "#define PZ_ABI_VERSION 22\n" in hdr and _lib.ABI_VERSION == 22 and L.pz_abi_version() == 22
    for name in ("CROP", "BRIGHTNESS", "CONTRAST", "SATURATION", "HUE", "ALL"):
        assert f"PZ_AUG_{name} = {getattr(_lib, 'PZ_AUG_' + name)}" in hdr
    # 224 x 224 is dealt to ceil(50176 / 4096) = 13 workgroups per frame, three fp32 sums each
    assert L.pz_image_augment_scratch_bytes(256, 224) == 256 * 13 * 3 * 4
    assert L.pz_image_augment_scratch_bytes(2, 8) == 2 * 1 * 3 * 4
    assert L.pz_image_augment_scratch_bytes(0, 8) == 0


def _arena(size=1 << 16):
    buf = ctypes.create_string_buffer(size + 64)
    return buf, (ctypes.addressof(buf) + 63) // 64 * 64


def test_augment_entry_point_refuses_bad_arguments_before_launch():
    import pizero_native

    L = pizero_native.lib()
    buf, base = _arena()
    n, S = 2, 8
    fr, par, msk, lut, sc, out = base, base + 1024, base + 2048, base + 3072, base + 4096, base + 8192
    need = n * 1 * 3 * 4

    def call(**kw):
        a = dict(frames=fr, cl=0, n=n, S=S, params=par, mask=msk, union=31, lut=lut, scratch=sc, sb=need, out=out)
        a.update(kw)
        return L.pz_image_augment(a["frames"], a["cl"], a["n"], a["S"], a["params"], a["mask"], a["union"], a["lut"],
                                  a["scratch"], a["sb"], a["out"], None)

    cases = [("null frames", dict(frames=None), b"null pointer"), ("null params", dict(params=None), b"params"),
             ("null mask", dict(mask=None), b"mask"), ("null out", dict(out=None), b"out"),
             ("null scratch", dict(scratch=None), b"null scratch"), ("layout flag", dict(cl=2), b"channels_last"),
             ("n = 0", dict(n=0), b"n and S must be positive"), ("n < 0", dict(n=-1), b"n and S must be positive"),
             ("S = 0", dict(S=0), b"n and S must be positive"), ("extent", dict(S=16385), b"S is limited to 16384"),
             ("union bits", dict(union=32), b"ops_union"), ("misaligned params", dict(params=par + 2), b"params"),
             ("misaligned out", dict(out=out + 1), b"misaligned out"),
             ("misaligned scratch", dict(scratch=sc + 2), b"misaligned scratch"),
             ("small scratch", dict(sb=need - 4), b"scratch has"),
             ("scratch inside out", dict(scratch=out + 64), b"scratch overlaps"),
             ("out inside frames", dict(out=fr + 64), b"out overlaps"),
             ("out over params", dict(out=par - 64), b"out overlaps")]
    for label, kw, msg in cases:
        assert call(**kw) == 1, f"{label} was not refused"
        err = L.pz_last_error()
        assert err.startswith(b"image_augment") and msg in err, (label, err)
    del buf


def test_resize_u8_entry_point_refuses_bad_arguments_before_launch():
    import pizero_native

    L = pizero_native.lib()
    buf, base = _arena()
    fr, sc, out, tab = base, base + 8192, base + 40000, base + 50000
    n, H, W, S = 1, 8, 8, 4
    need = n * 3 * H * S * 4

    def call(**kw):
        a = dict(frames=fr, n=n, W=W, vt=8, scratch=sc, sb=need, out=out)
        a.update(kw)
        return L.pz_image_resize_u8(a["frames"], 1, a["n"], H, a["W"], S, tab, tab, tab, 8, tab, tab, tab, a["vt"],
                                    a["scratch"], a["sb"], a["out"], None)

    for label, kw, msg in [("null frames", dict(frames=None), b"null pointer"), ("n = 0", dict(n=0), b"positive"),
                           ("extent", dict(W=16385), b"limited to 16384"), ("taps", dict(vt=65), b"limit of 64"),
                           ("small scratch", dict(sb=need - 4), b"scratch has"),
                           ("out inside scratch", dict(out=sc + 64), b"overlap")]:
        assert call(**kw) == 1, f"{label} was not refused"
        err = L.pz_last_error()
        assert err.startswith(b"image_resize_u8") and msg in err, (label, err)
    del buf


def test_train_agent_surface():
    import inspect

    from pizero_native import ops
    from src.agent.train import TrainAgent

    sig = inspect.signature(TrainAgent.preprocess_batch)
    assert sig.parameters["augment"].default is False
    assert list(inspect.signature(ops.image_augment).parameters) == ["frames", "params", "mask", "channels_last", "out",
                                                                     "scratch"]
    assert list(inspect.signature(ops.image_resize_u8).parameters) == ["frames", "S", "channels_last", "out", "scratch"]
