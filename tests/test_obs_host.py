"""Observation front end / action back end: the parts that need no GPU.

The fp64 restatement of the resize (tests/obs_ref.py) is the identity on same-size input and agrees with
PIL.Image.resize(LANCZOS), an independent implementation, to 1 code on low-frequency mid-range images; the tap-table
builder (pizero_native.ops.lanczos3_taps) reproduces the restatement's weights and refuses what the kernel was not
sized for; BaseEnvAdapter reproduces the reference methods' recorded outputs (tests/golden/obs_norm.npz, written by
tests/golden/make_golden_obs.py); the C entry points refuse bad arguments before any launch.
"""

import ctypes
import json
import os

import numpy as np
import pytest

from tests import obs_ref as R
from tests.conftest import ROOT
from tests.oracle_helpers import load_golden

NEW = ("pz_image_resize_norm", "pz_proprio_normalize", "pz_action_denormalize", "pz_image_resize_scratch_bytes")


def _bridge_stats():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")))


def test_abi_declares_exports_and_binds_the_entry_points():
    import pizero_native
    from pizero_native._lib import SIGNATURES
    from tests.test_abi import declared_symbols

    syms = declared_symbols()
    L = pizero_native.lib()
    for s in NEW:
        assert s in syms, f"{s} not declared in include/pz_abi.h"
        assert hasattr(L, s), f"{s} not exported"
        assert s in SIGNATURES, f"{s} has no ctypes signature"
    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    from pizero_native import _lib

    assert f"#define PZ_OBS_MAX_TAPS {_lib.PZ_OBS_MAX_TAPS}\n" in hdr
    assert f"#define PZ_OBS_MAX_EXTENT {_lib.PZ_OBS_MAX_EXTENT}\n" in hdr
    assert L.pz_image_resize_scratch_bytes(3, 131, 56) == 3 * 3 * 131 * 56 * 4


@pytest.mark.parametrize("s", [224, 56, 37])
def test_restatement_is_identity_on_same_size_input(s):
    x = np.random.default_rng(1).integers(0, 256, (2, s, s, 3), dtype=np.uint8)
    assert np.abs(R.axis_matrix(s, s) - np.eye(s)).max() < 1e-15
    v, codes = R.resize(x, s)
    assert np.array_equal(codes, x.transpose(0, 3, 1, 2))
    assert np.abs(v - x.transpose(0, 3, 1, 2)).max() < 1e-12


@pytest.mark.parametrize("hw", [(480, 640), (256, 320), (37, 53), (225, 223), (300, 200)])
def test_restatement_agrees_with_pil_lanczos(hw):
    """PIL rounds to uint8 (and clips) between its two passes, so it is a witness only where nothing overshoots:
    low-frequency, mid-range images.  There the two differ by at most 1 code."""
    from PIL import Image

    h, w = hw
    img = R.low_frequency_frame(h, w, seed=h * 1000 + w)
    pil = np.asarray(Image.fromarray(img).resize((224, 224), Image.LANCZOS))
    _, codes = R.resize(img[None], 224)
    d = np.abs(codes[0].transpose(1, 2, 0).astype(np.int32) - pil.astype(np.int32))
    print(f"{h}x{w} -> 224: max |restatement - PIL| = {d.max()} codes, {100 * (d > 0).mean():.1f} % of pixels differ")
    assert d.max() <= 1


GEOMETRIES = [(37, 56), (53, 56), (131, 56), (97, 56), (57, 56), (55, 56), (56, 56), (480, 224), (640, 224),
              (224, 224), (1, 56), (560, 56)]


@pytest.mark.parametrize("n_in,n_out", GEOMETRIES)
def test_tap_tables_match_the_restatement(n_in, n_out):
    from pizero_native import ops

    first, count, w = ops.lanczos3_taps(n_in, n_out)
    assert first.dtype == np.int32 and count.dtype == np.int32 and w.dtype == np.float64
    assert first.shape == count.shape == (n_out,) and w.shape == (n_out, count.max())
    assert (first >= 0).all() and (count >= 1).all() and (first + count <= n_in).all()
    assert w.shape[1] <= ops.PZ_OBS_MAX_TAPS
    M = np.zeros((n_out, n_in))
    for i in range(n_out):
        M[i, first[i]:first[i] + count[i]] = w[i, :count[i]]
        assert (w[i, count[i]:] == 0).all()
    assert np.abs(M - R.axis_matrix(n_in, n_out)).max() < 1e-14
    assert np.abs(w.sum(1) - 1).max() < 1e-14


def test_tap_table_refusals():
    from pizero_native import ops

    with pytest.raises(ValueError, match="PZ_OBS_MAX_TAPS = 64"):
        ops.lanczos3_taps(56 * 11, 56)  # an 11x downscale needs 68 taps
    ops.lanczos3_taps(56 * 10, 56)  # 10x is within the limit
    with pytest.raises(ValueError, match="PZ_OBS_MAX_EXTENT"):
        ops.lanczos3_taps(ops.PZ_OBS_MAX_EXTENT + 1, 4096)
    for bad in [(0, 56), (56, 0), (-3, 56), (37.5, 56)]:
        with pytest.raises(ValueError, match="positive integers"):
            ops.lanczos3_taps(*bad)


def test_resize_entry_point_refuses_bad_arguments_before_launch():
    """host memory is enough: the checks return before anything is launched or dereferenced"""
    import pizero_native

    L = pizero_native.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    fr, sc, out, tab = base, base + 8192, base + 40000, base + 50000
    n, H, W, S = 1, 8, 8, 4
    need = n * 3 * H * S * 4

    def call(**kw):
        a = dict(frames=fr, cl=1, n=n, H=H, W=W, S=S, hf=tab, hc=tab, hw=tab, ht=8, vf=tab, vc=tab, vw=tab, vt=8,
                 lut=tab, scratch=sc, sb=need, out=out)
        a.update(kw)
        return L.pz_image_resize_norm(a["frames"], a["cl"], a["n"], a["H"], a["W"], a["S"], a["hf"], a["hc"], a["hw"],
                                      a["ht"], a["vf"], a["vc"], a["vw"], a["vt"], a["lut"], a["scratch"], a["sb"],
                                      a["out"], None)

    cases = [("null frames", dict(frames=None), b"null pointer"), ("null table", dict(vw=None), b"null tap table"),
             ("layout flag", dict(cl=2), b"channels_last"), ("n = 0", dict(n=0), b"must be positive"),
             ("S < 0", dict(S=-4), b"must be positive"), ("extent", dict(W=16385), b"limited to 16384"),
             ("too many taps (h)", dict(ht=65), b"limit of 64"), ("too many taps (v)", dict(vt=200), b"limit of 64"),
             ("no taps", dict(vt=0), b"tap counts"), ("misaligned scratch", dict(scratch=sc + 2), b"misaligned"),
             ("small scratch", dict(sb=need - 4), b"scratch has"), ("out inside scratch", dict(out=sc + 64), b"overlap"),
             ("frames inside out", dict(frames=out + 16), b"overlap")]
    for label, kw, msg in cases:
        assert call(**kw) == 1, f"{label} was not refused"
        err = L.pz_last_error()
        assert err.startswith(b"image_resize_norm") and msg in err, (label, err)


@pytest.mark.parametrize("fn", ["pz_proprio_normalize", "pz_action_denormalize"])
def test_norm_entry_points_refuse_bad_arguments_before_launch(fn):
    import pizero_native

    L = pizero_native.lib()
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    x, y, a, b = base, base + 1024, base + 2048, base + 2112

    def call(x=x, y=y, rows=4, D=7, n_pass=1, a=a, b=b, mode=0):
        if fn == "pz_proprio_normalize":
            return L.pz_proprio_normalize(x, y, rows, D, a, b, mode, None)
        return L.pz_action_denormalize(x, y, rows, D, n_pass, a, b, mode, None)

    cases = [("null x", dict(x=None)), ("null stats", dict(b=None)), ("rows = 0", dict(rows=0)), ("D = 0", dict(D=0)),
             ("mode", dict(mode=2)), ("misaligned", dict(y=y + 2))]
    if fn == "pz_action_denormalize":
        cases += [("n_pass < 0", dict(n_pass=-1)), ("n_pass > D", dict(n_pass=8))]
    for label, kw in cases:
        assert call(**kw) == 1, f"{fn}: {label} was not refused"
        assert L.pz_last_error().startswith(fn[3:].encode()), (label, L.pz_last_error())


def test_bridge_statistics_fixture():
    path = os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")
    assert os.path.getsize(path) < 1 << 20
    from src.agent.env_adapter.base import load_dataset_statistics

    s = load_dataset_statistics(path)
    for node in ("proprio", "action"):
        for k in ("p01", "p99", "mean", "std"):
            assert len(s[node][k]) == 7


def test_base_env_adapter_matches_reference_outputs():
    from src.agent.env_adapter.base import BaseEnvAdapter

    g = load_golden("obs_norm")
    s = _bridge_stats()
    ad = BaseEnvAdapter()
    p, a = s["proprio"], s["action"]
    x, y = g["proprio_raw"], g["action_norm"]
    sets = {"bridge": (x, y, np.array(p["p01"]), np.array(p["p99"]), np.array(p["mean"]), np.array(p["std"]),
                       np.array(a["p01"]), np.array(a["p99"]), np.array(a["mean"]), np.array(a["std"])),
            "synth": (g["synth/x"], g["synth/a"], g["synth/lo"], g["synth/hi"], g["synth/mean"], g["synth/std"],
                      g["synth/lo"], g["synth/hi"], g["synth/mean"], g["synth/std"])}
    for tag, (xi, yi, plo, phi, pm, ps, alo, ahi, am, as_) in sets.items():
        got = {"normalize_bound": ad.normalize_bound(xi, plo, phi),
               "normalize_gaussian": ad.normalize_gaussian(xi, pm, ps),
               "denormalize_bound": ad.denormalize_bound(yi, alo, ahi),
               "denormalize_gaussian": ad.denormalize_gaussian(yi, am, as_)}
        ref = {"normalize_bound": R.normalize_bound(xi, plo, phi), "normalize_gaussian": R.normalize_gaussian(xi, pm, ps),
               "denormalize_bound": R.denormalize_bound(yi, alo, ahi),
               "denormalize_gaussian": R.denormalize_gaussian(yi, am, as_)}
        for k, v in got.items():
            want = g[f"{tag}/{k}"]
            assert v.dtype == np.float64 and v.shape == want.shape
            # the same fp64 formulas up to the association of the products: a few ulps
            assert np.allclose(v, want, rtol=1e-14, atol=1e-15), (tag, k, np.abs(v - want).max())
            assert np.allclose(ref[k], want, rtol=1e-14, atol=1e-15), (tag, k)
    nb = g["bridge/normalize_bound"]
    assert (nb == 1).any() and (nb == -1).any() and (np.abs(nb) < 1).any()  # the clip is hit on both sides
    # the rollout-level helpers: the gripper (last action dimension) passes through
    out = ad.denormalize_action(y, s, "bound")
    assert np.array_equal(out[:, -1], y[:, -1])
    assert np.allclose(out[:, :-1], g["bridge/denormalize_bound"][:, :-1], rtol=1e-14, atol=1e-15)
    assert np.allclose(ad.normalize_proprio(x, s, "gaussian"), g["bridge/normalize_gaussian"], rtol=1e-14, atol=1e-15)
    with pytest.raises(ValueError):
        ad.normalize_proprio(x, s, "minmax")


def test_eval_agent_and_graph_surface():
    import inspect

    from pizero_native.graph import InferenceGraph, ObservationGraph
    from src.agent.eval import EvalAgent

    assert list(inspect.signature(EvalAgent.act).parameters)[:6] == ["self", "frames", "input_ids", "attention_mask",
                                                                     "raw_proprio", "noise"]
    assert list(inspect.signature(ObservationGraph.__init__).parameters) == ["self", "model", "bsz", "frame_hw", "stats",
                                                                             "channels_last", "clip"]
    assert ObservationGraph.replay is InferenceGraph.replay and ObservationGraph.capture is InferenceGraph.capture
    assert EvalAgent.STATS_KEY == "env.adapter.dataset_statistics_path"
