"""Training-image augmentation: the host side of ops.image_augment.

The reference augments every training frame in its TensorFlow data pipeline (src/agent/dataset.py:38-70 through
dlimp/augmentations.py:65-133).  Here the kernels are pure functions; this module parses the reference's
``image_augment_kwargs`` structure and draws each frame's parameters on the host from a counter-based generator
keyed on (seed, cnt_batch, rank) -- nothing else, so a resumed run draws what the uninterrupted run draws, ranks
differ, and neither torch's nor numpy's global generator is touched.  TF's own random stream is not reproduced.
"""

from __future__ import annotations

import math

import numpy as np

from ._lib import PZ_AUG_BRIGHTNESS, PZ_AUG_CONTRAST, PZ_AUG_CROP, PZ_AUG_HUE, PZ_AUG_SATURATION

# the one op order the kernel implements (the reference's own); a spec may use any subset of it
ORDER = ("random_resized_crop", "random_brightness", "random_contrast", "random_saturation", "random_hue")
OP_BITS = dict(zip(ORDER, (PZ_AUG_CROP, PZ_AUG_BRIGHTNESS, PZ_AUG_CONTRAST, PZ_AUG_SATURATION, PZ_AUG_HUE)))
# ops of dlimp's AUGMENT_OPS that are not implemented
UNSUPPORTED = ("random_flip_left_right", "random_flip_up_down", "random_rot90")
CROP_DRAWS = ("shared", "independent")

# the reference's settings (src/agent/dataset.py:39-69): the primary camera, and the wrist camera without the crop
REFERENCE_PRIMARY = {
    "random_resized_crop": {"scale": [0.8, 1.0], "ratio": [0.9, 1.1]},
    "random_brightness": [0.1],
    "random_contrast": [0.9, 1.1],
    "random_saturation": [0.9, 1.1],
    "random_hue": [0.05],
    "augment_order": list(ORDER),
}
REFERENCE_WRIST = {k: v for k, v in REFERENCE_PRIMARY.items() if k != "random_resized_crop"}
REFERENCE_WRIST["augment_order"] = list(ORDER[1:])

# column of each value in a parameter row, and the row that changes nothing
BOX, BRIGHTNESS, CONTRAST, SATURATION, HUE = slice(0, 4), 4, 5, 6, 7
IDENTITY_ROW = (0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0)


def _args(op, value, names):
    """the op's arguments from a dict of keywords or a positional sequence, as augment_image accepts them"""
    if hasattr(value, "items"):
        extra = sorted(set(value) - set(names))
        if extra or len(value) != len(names):
            raise ValueError(f"image_augment_kwargs: {op} takes {list(names)}, got {sorted(value)}")
        vals = [value[k] for k in names]
    else:
        vals = list(value)
        if len(vals) != len(names):
            raise ValueError(f"image_augment_kwargs: {op} takes {list(names)}, got {len(vals)} positional values")
    return vals


def _pair(op, name, v, lo_min, hi_max=None):
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"image_augment_kwargs: {op} {name} must be a [lower, upper] pair, got {v!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo_min <= lo <= hi and (hi_max is None or hi <= hi_max)):
        bound = f"{lo_min} <= lower <= upper" + (f" <= {hi_max}" if hi_max is not None else "")
        raise ValueError(f"image_augment_kwargs: {op} {name} needs {bound}, got {v!r}")
    return lo, hi


def parse_spec(kwargs):
    """One ``augment_image`` kwargs dict -> {"mask": int, "crop": (scale_lo, scale_hi, ratio_lo, ratio_hi) | None,
    "brightness": max_delta | None, "contrast": (lower, upper) | None, "saturation": (lower, upper) | None,
    "hue": max_delta | None}.  Raises ValueError (naming the key or the op) for an ``augment_order`` that is not a
    subset of ORDER in ORDER's order, and for the flips and random_rot90."""
    if not hasattr(kwargs, "items"):
        raise ValueError("image_augment_kwargs: expected a dict with an 'augment_order' key, got "
                         f"{type(kwargs).__name__}")
    if "augment_order" not in kwargs:
        raise ValueError("image_augment_kwargs must contain an 'augment_order' key")
    order = list(kwargs["augment_order"])
    for op in order:
        if op in UNSUPPORTED:
            raise ValueError(f"image_augment_kwargs: {op} is not supported (only {', '.join(ORDER)})")
        if op not in ORDER:
            raise ValueError(f"image_augment_kwargs: unknown op {op!r} in augment_order")
    if [op for op in ORDER if op in order] != order:
        raise ValueError(f"image_augment_kwargs: augment_order {order} is not supported: the ops run in the fixed "
                         f"order {list(ORDER)}, each at most once (any subset of it)")
    for k in kwargs:
        if k != "augment_order" and k not in order:
            raise ValueError(f"image_augment_kwargs: {k!r} has arguments but is not in augment_order")
    spec = {"mask": 0, "crop": None, "brightness": None, "contrast": None, "saturation": None, "hue": None}
    for op in order:
        if op not in kwargs:
            raise ValueError(f"image_augment_kwargs: {op} is in augment_order but has no arguments")
        spec["mask"] |= OP_BITS[op]
        if op == "random_resized_crop":
            scale, ratio = _args(op, kwargs[op], ("scale", "ratio"))
            s = _pair(op, "scale", scale, 0.0, 1.0)
            r = _pair(op, "ratio", ratio, 0.0)
            if s[0] <= 0.0 or r[0] <= 0.0:
                raise ValueError(f"image_augment_kwargs: {op} scale and ratio must be positive")
            spec["crop"] = (*s, *r)
        elif op in ("random_brightness", "random_hue"):
            (d,) = _args(op, kwargs[op], ("max_delta",))
            d = float(d)
            top = 0.5 if op == "random_hue" else math.inf
            if not 0.0 <= d <= top:
                raise ValueError(f"image_augment_kwargs: {op} max_delta must be in [0, {top}], got {d}")
            spec["brightness" if op == "random_brightness" else "hue"] = d
        else:
            lo, hi = _args(op, kwargs[op], ("lower", "upper"))
            spec["contrast" if op == "random_contrast" else "saturation"] = _pair(op, "lower/upper", (lo, hi), 0.0)
    return spec


def parse_kwargs(kwargs):
    """``image_augment_kwargs`` -> a list of specs, one per image slot: one dict applies to every frame, a list or
    tuple of dicts gives one per slot of a multi-image model (frame i uses slot i % len)."""
    if hasattr(kwargs, "items") or isinstance(kwargs, (str, bytes)) or not hasattr(kwargs, "__len__"):
        return [parse_spec(kwargs)]
    if len(kwargs) == 0:
        raise ValueError("image_augment_kwargs: an empty list of per-slot dicts")
    return [parse_spec(k) for k in kwargs]


def generator(seed, cnt_batch, rank, stream=0):
    """Philox keyed on the seed, with (cnt_batch, rank) in the two high counter words: the draws of one micro-batch
    advance the low word only, so no two (seed, cnt_batch, rank) share any part of a stream.  ``stream`` (a 64-bit
    constant, 0 for the image augmentation) goes into the key's high word: another consumer of the same seed draws
    from a stream of its own."""
    m = (1 << 64) - 1
    if cnt_batch < 0 or rank < 0:
        raise ValueError("draw_params: cnt_batch and rank must be non-negative")
    return np.random.Generator(np.random.Philox(key=[int(seed) & m, ((int(seed) >> 64) ^ int(stream)) & m],
                                                counter=[0, 0, int(cnt_batch) & m, int(rank) & m]))


PREFIX_STREAM = 0x7072656669785F64  # "prefix_d": the action-prefix delays' stream
# the episode sampler's epoch permutations (pizero_native.episodes): training and validation
EPISODE_STREAM = 0x657069736F646573  # "episodes"
EPISODE_VAL_STREAM = 0x657069735F76616C  # "epis_val"


def draw_prefix_len(bsz, max_delay, seed, cnt_batch, rank=0):
    """int64 [bsz] numpy: one delay d ~ U{0..max_delay} per sample of micro-batch ``cnt_batch``, from the
    generator above under PREFIX_STREAM -- a function of (seed, cnt_batch, rank) alone, so ranks differ and neither
    the augmentation's draws nor torch's generator are touched.  TrainAgent passes the number of micro-batches consumed
    (``micro_batches_seen``, which a resume restores), so a resumed run continues the draws."""
    bsz, max_delay = int(bsz), int(max_delay)
    if bsz < 1 or max_delay < 0:
        raise ValueError(f"draw_prefix_len: bsz must be positive and max_delay non-negative, got {bsz}, {max_delay}")
    return generator(seed, cnt_batch, rank, stream=PREFIX_STREAM).integers(0, max_delay + 1, size=bsz)


def draw_params(specs, n_frames, seed, cnt_batch, rank=0, crop_draws="shared"):
    """(params float32 [n_frames, 8], mask int32 [n_frames]) for ops.image_augment.  ``specs`` is parse_kwargs'
    list (or the kwargs themselves); frame i uses specs[i % len(specs)].  Every frame consumes eight uniforms u in
    [0, 1) whatever its spec (scale, ratio, row offset, column offset, brightness, contrast, saturation, hue), so a
    frame's draws do not depend on the other slots' settings:

      deltas  -max + 2 max u  in [-max, max);   factors  lower + (upper - lower) u  in [lower, upper)
      crop    scale uniform, ratio log-uniform, new_h = clip(sqrt(scale / ratio), 0, 1), new_w = clip(sqrt(scale
              ratio), 0, 1), offsets u (1 - new) in [0, 1 - new); box = (off_y, off_x, off_y + new_h, off_x + new_w)

    crop_draws "shared" (default) reproduces the reference: its random_resized_crop hands the SAME seed to all four
    stateless_uniform calls, so one u per frame drives scale, ratio and both offsets.  "independent" draws four."""
    if crop_draws not in CROP_DRAWS:
        raise ValueError(f"image_augment_crop_draws must be one of {list(CROP_DRAWS)}, got {crop_draws!r}")
    if not (isinstance(specs, list) and specs and all(isinstance(s, dict) and "mask" in s for s in specs)):
        specs = parse_kwargs(specs)
    n = int(n_frames)
    if n < 1:
        raise ValueError(f"draw_params: n_frames must be positive, got {n_frames}")
    u = generator(seed, cnt_batch, rank).random((n, 8))
    if crop_draws == "shared":
        u[:, 1:4] = u[:, 0:1]
    params = np.tile(np.asarray(IDENTITY_ROW, np.float64), (n, 1))
    mask = np.zeros(n, np.int32)
    for slot, sp in enumerate(specs):
        rows = slice(slot, n, len(specs))
        ur = u[rows]
        mask[rows] = sp["mask"]
        if sp["crop"] is not None:
            s_lo, s_hi, r_lo, r_hi = sp["crop"]
            scale = s_lo + (s_hi - s_lo) * ur[:, 0]
            ratio = np.exp(math.log(r_lo) + (math.log(r_hi) - math.log(r_lo)) * ur[:, 1])
            new_h = np.clip(np.sqrt(scale / ratio), 0.0, 1.0)
            new_w = np.clip(np.sqrt(scale * ratio), 0.0, 1.0)
            off_y, off_x = ur[:, 2] * (1.0 - new_h), ur[:, 3] * (1.0 - new_w)
            # off + new < 1 in exact arithmetic; the minimum keeps the rounded box inside the image too
            params[rows, 0:4] = np.stack([off_y, off_x, np.minimum(off_y + new_h, 1.0),
                                          np.minimum(off_x + new_w, 1.0)], axis=1)
        if sp["brightness"] is not None:
            params[rows, BRIGHTNESS] = -sp["brightness"] + 2.0 * sp["brightness"] * ur[:, 4]
        for col, key, k in ((CONTRAST, "contrast", 5), (SATURATION, "saturation", 6)):
            if sp[key] is not None:
                lo, hi = sp[key]
                params[rows, col] = lo + (hi - lo) * ur[:, k]
        if sp["hue"] is not None:
            params[rows, HUE] = -sp["hue"] + 2.0 * sp["hue"] * ur[:, 7]
    return params.astype(np.float32), mask
