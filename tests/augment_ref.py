"""Restatement of the training-image augmentation in numpy, fp64 by default.

The semantics of the TF ops the reference's pipeline calls (dlimp/augmentations.py:65-133), applied to one frame of
uint8 codes [3, S, S]; TensorFlow is not installed, so nothing here is pinned to TF's own outputs.

  x = q / 255
  crop        tf.image.crop_and_resize, bilinear, crop size = image size, box (y1, x1, y2, x2) in [0, 1]:
              in_y = y1 (S-1) + y (y2-y1)(S-1)/(S-1); rows floor / ceil of in_y; interpolate in x on both, then in y
  brightness  x + delta
  contrast    (x - m_c) f + m_c, m_c the mean of channel c over the frame as it is at that point
  saturation  hexcone RGB -> HSV, s = clip(s f, 0, 1), HSV -> RGB
  hue         RGB -> HSV, h = (h + delta) mod 1, HSV -> RGB
  clip(x, 0, 1) after every op;  q' = min(floor(255.5 x), 255)

Order fixed; ``mask`` (bits 1, 2, 4, 8, 16 in that order) picks the subset.  ``dtype`` lets a test evaluate the same
chain in float32.
"""

import numpy as np

CROP, BRIGHTNESS, CONTRAST, SATURATION, HUE, ALL = 1, 2, 4, 8, 16, 31
IDENTITY = (0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0)


def rgb_to_hsv(rgb):
    """[3, ...] -> (h, s, v), h in [0, 1) (hexcone; h = 0 where the chroma is 0)"""
    r, g, b = rgb
    t = rgb.dtype.type
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    rng = mx - mn
    safe = np.where(rng > 0, rng, t(1))
    s = np.where(mx > 0, rng / np.where(mx > 0, mx, t(1)), t(0))
    h = np.where(r == mx, (g - b) / safe / t(6),
                 np.where(g == mx, (b - r) / safe / t(6) + t(2) / t(6), (r - g) / safe / t(6) + t(4) / t(6)))
    h = np.where(rng > 0, h, t(0))
    h = np.where(h < 0, h + t(1), h)
    return h, s, mx


def hsv_to_rgb(h, s, v):
    t = v.dtype.type
    dh = h * t(6)
    dr = np.clip(np.abs(dh - t(3)) - t(1), 0, 1)
    dg = np.clip(t(2) - np.abs(dh - t(2)), 0, 1)
    db = np.clip(t(2) - np.abs(dh - t(4)), 0, 1)
    oms = t(1) - s
    return np.stack([(oms + s * dr) * v, (oms + s * dg) * v, (oms + s * db) * v])


def crop_and_resize(x, box):
    """x [3, S, S], box (y1, x1, y2, x2): a sample outside the image contributes 0 (TF's extrapolation value), which
    a box inside [0, 1] reaches only with weight ~0 through rounding"""
    S = x.shape[-1]
    t = x.dtype.type
    y1, x1, y2, x2 = (np.float64(b) for b in box)
    e = np.float64(S - 1)
    i = np.arange(S, dtype=np.float64)
    if S > 1:
        in_y, in_x = y1 * e + i * ((y2 - y1) * e / e), x1 * e + i * ((x2 - x1) * e / e)
    else:
        in_y, in_x = 0.5 * (y1 + y2) * e + 0 * i, 0.5 * (x1 + x2) * e + 0 * i
    top, left = np.floor(in_y).astype(np.int64), np.floor(in_x).astype(np.int64)
    bot, right = np.ceil(in_y).astype(np.int64), np.ceil(in_x).astype(np.int64)
    ly, lx = (in_y - np.floor(in_y)).astype(x.dtype), (in_x - np.floor(in_x)).astype(x.dtype)

    def take(rows, cols):
        ok = ((rows >= 0) & (rows < S))[:, None] & ((cols >= 0) & (cols < S))[None, :]
        g = x[:, np.clip(rows, 0, S - 1)[:, None], np.clip(cols, 0, S - 1)[None, :]]
        return np.where(ok[None], g, t(0))

    tl, tr, bl, br = take(top, left), take(top, right), take(bot, left), take(bot, right)
    tp = tl + (tr - tl) * lx[None, None, :]
    bt = bl + (br - bl) * lx[None, None, :]
    return tp + (bt - tp) * ly[None, :, None]


def augment_frame(q, row, mask=ALL, dtype=np.float64):
    """q uint8 [3, S, S], row = 8 parameters -> the unquantised result x in [0, 1], [3, S, S] of ``dtype``"""
    t = np.dtype(dtype).type
    row = np.asarray(row, np.float32)  # the kernel sees fp32 parameters
    x = q.astype(dtype) / t(255)
    clip = lambda a: np.clip(a, t(0), t(1))  # noqa: E731
    if mask & CROP:
        x = clip(crop_and_resize(x, row[:4]))
    if mask & BRIGHTNESS:
        x = clip(x + t(row[4]))
    if mask & CONTRAST:
        m = x.mean(axis=(1, 2), keepdims=True, dtype=dtype)
        x = clip((x - m) * t(row[5]) + m)
    if mask & SATURATION:
        h, s, v = rgb_to_hsv(x)
        x = clip(hsv_to_rgb(h, clip(s * t(row[6])), v))
    if mask & HUE:
        h, s, v = rgb_to_hsv(x)
        h = h + t(row[7])
        x = clip(hsv_to_rgb(h - np.floor(h), s, v))
    return x


def quantise(x):
    """convert_image_dtype(float -> uint8, saturate=True): min(floor(255.5 x), 255)"""
    return np.minimum(np.floor(x * x.dtype.type(255.5)), 255).astype(np.uint8)


def augment(frames, params, mask, dtype=np.float64):
    """frames uint8 [n, 3, S, S], params [n, 8], mask [n] -> x [n, 3, S, S] (unquantised)"""
    return np.stack([augment_frame(f, p, int(m), dtype) for f, p, m in zip(frames, params, mask)])


def host_augment_codes(frames, params, mask):
    """what a host pipeline would do with this restatement: the augmented uint8 codes (tools/augment_bench.py)"""
    return quantise(augment(frames, params, mask))
