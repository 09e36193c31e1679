"""fp64 numpy restatement of the observation front end / action back end (csrc/pz_obs.hip), for the tests.

Resize: tf.image.resize(method="lanczos3", antialias=True) as a dense matrix per axis, written from the formulas
alone (no table sharing with pizero_native.ops.lanczos3_taps, which is checked against this).  For an axis
n_in -> n_out: scale = n_in / n_out, ks = max(scale, 1), support = 3 ks; output i is centred on c = (i + 0.5) scale and
its taps are the input indices x in [max(floor(c - support + 0.5), 0), min(floor(c + support + 0.5), n_in)) with
weights L3((x + 0.5 - c) / ks) normalised to sum 1, L3(t) = sinc(t) sinc(t / 3) on |t| < 3 and 0 elsewhere.
"""

from __future__ import annotations

import math

import numpy as np


def lanczos3(t):
    if abs(t) >= 3.0:
        return 0.0
    if t == 0.0:
        return 1.0
    a = math.pi * t
    return (math.sin(a) / a) * (math.sin(a / 3.0) / (a / 3.0))


def axis_matrix(n_in, n_out):
    """[n_out, n_in] fp64: row i holds output i's normalised weights (zero outside its window)"""
    scale = n_in / n_out
    ks = max(scale, 1.0)
    support = 3.0 * ks
    M = np.zeros((n_out, n_in), np.float64)
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(int(math.floor(c - support + 0.5)), 0)
        hi = min(int(math.floor(c + support + 0.5)), n_in)
        w = np.array([lanczos3((x + 0.5 - c) / ks) for x in range(lo, hi)], np.float64)
        M[i, lo:hi] = w / w.sum()
    return M


def resize(frames, S, channels_last=True):
    """uint8 frames [n, H, W, 3] (or [n, 3, H, W]) -> (v fp64 [n, 3, S, S] unrounded, codes uint8 [n, 3, S, S]):
    codes = clip(round-half-to-even(v), 0, 255), what tf.round + the cast back to uint8 give."""
    x = np.asarray(frames)
    assert x.dtype == np.uint8 and x.ndim == 4
    if channels_last:
        x = x.transpose(0, 3, 1, 2)
    x = x.astype(np.float64)
    Mv, Mh = axis_matrix(x.shape[2], S), axis_matrix(x.shape[3], S)
    v = np.einsum("oy,ncyx,px->ncop", Mv, x, Mh, optimize=True)
    codes = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return v, codes


def pixel_norm(codes):
    """the model's pixel normalisation of uint8 codes, fp64: (q / 255 - 0.5) / 0.5"""
    return (np.asarray(codes).astype(np.float64) / 255.0 - 0.5) / 0.5


# the four normalisation formulas (reference env_adapter/base.py:8-49), fp64
def normalize_bound(x, lo, hi):
    x, lo, hi = (np.asarray(a, np.float64) for a in (x, lo, hi))
    return np.clip(2.0 * (x - lo) / (hi - lo + 1e-8) - 1.0, -1.0, 1.0)


def denormalize_bound(a, lo, hi):
    a, lo, hi = (np.asarray(t, np.float64) for t in (a, lo, hi))
    return (a + 1.0) / 2.0 * (hi - lo) + lo


def normalize_gaussian(x, mean, std):
    x, mean, std = (np.asarray(a, np.float64) for a in (x, mean, std))
    return (x - mean) / (std + 1e-8)


def denormalize_gaussian(a, mean, std):
    a, mean, std = (np.asarray(t, np.float64) for t in (a, mean, std))
    return a * (std + 1e-8) + mean


def denormalize_action(a, stats, kind, n_pass=1):
    """all but the trailing n_pass dimensions, which pass through"""
    a = np.asarray(a, np.float64)
    k = a.shape[-1] - n_pass
    s = stats["action"]
    if kind == "bound":
        head = denormalize_bound(a[..., :k], np.asarray(s["p01"])[:k], np.asarray(s["p99"])[:k])
    else:
        head = denormalize_gaussian(a[..., :k], np.asarray(s["mean"])[:k], np.asarray(s["std"])[:k])
    return np.concatenate([head, a[..., k:]], axis=-1)


def normalize_proprio(x, stats, kind):
    s = stats["proprio"]
    if kind == "bound":
        return normalize_bound(x, s["p01"], s["p99"])
    return normalize_gaussian(x, s["mean"], s["std"])


def low_frequency_frame(h, w, seed):
    """mid-range, low-frequency uint8 [h, w, 3]: three sinusoids of period >= 19 px and amplitude <= 60 around a
    level in 96..128 plus +-6 noise -- stays far from 0 / 255, where a resize that rounds and clips between its two
    passes (PIL) would part from one that does not."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3), np.float64)
    for c in range(3):
        level = r.uniform(96, 128)
        acc = np.full((h, w), level)
        amps = r.uniform(5, 20, 3)  # sum <= 60
        for a in amps:
            period = r.uniform(19, 80)
            ang = r.uniform(0, 2 * math.pi)
            ph = r.uniform(0, 2 * math.pi)
            acc += a * np.sin(2 * math.pi * (xx * math.cos(ang) + yy * math.sin(ang)) / period + ph)
        img[..., c] = acc + r.uniform(-6, 6, (h, w))
    assert img.min() >= 0 and img.max() <= 255
    return np.rint(img).astype(np.uint8)


def checkerboard(n, h, w, square=3):
    """0 / 255 checkerboard of ``square``-pixel squares, uint8 [n, h, w, 3]: the Lanczos overshoot reaches the clip
    on both sides"""
    yy, xx = np.mgrid[0:h, 0:w]
    b = (((yy // square) + (xx // square)) % 2 * 255).astype(np.uint8)
    return np.broadcast_to(b[None, :, :, None], (n, h, w, 3)).copy()
