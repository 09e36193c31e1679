"""numpy float32 restatement of the compensated and stochastic bf16 weight updates (csrc/pz_optim.hip:
pz_adamw8bit_r, pz_adamw_r), independent of the kernels.

The 8-bit-state path wraps oracle/adamw8bit.py: ``step_8bit`` / ``step_32bit`` give the new moments, codes and absmax
(none of which depend on the weights), and the few lines that produce the fp32 result ``pv`` BEFORE it is rounded --
which those functions do not return -- are restated here.  The fp32-moment path restates ``adamw_kernel``'s expression
(csrc/pz_misc.hip: decay multiply, moments, step) with every operation rounded on its own, as pz_adamw_r computes it.
Then ``store`` turns pv into the bf16 weight:

  mode 1, compensated   the update started from w = p + c;  p' = rne(pv), c' = rne(pv - p'), 0 if pv is not finite
  mode 2, stochastic    p' = top 16 bits of (bits(pv) + r), rne(pv) if pv's exponent field is all ones;
                        r = (splitmix64(key + (i >> 2)) >> (16 (i & 3))) & 0xffff, i = the element's arena index

All weights / compensation words are float32 arrays holding bf16 values.  ``stall_weights`` / ``master_step`` are the
experiment of the issue: weights too large for an lr = 5e-5 step to survive round-to-nearest.
"""

import numpy as np

from oracle import adamw8bit as O8

f = np.float32
NEAREST, COMPENSATED, STOCHASTIC = 0, 1, 2
M64 = (1 << 64) - 1


def splitmix64(z):
    """uint64 array -> uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def splitmix64_int(z):
    """the same hash on a python int (the host side of the step key: key = splitmix64(seed + step))"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def step_key(seed, t):
    return splitmix64_int((int(seed) + int(t)) & M64)


def draws(key, idx):
    """16-bit draws of the elements with arena indices idx (int64 array, >= 0)"""
    idx = np.asarray(idx, dtype=np.int64)
    with np.errstate(over="ignore"):
        h = splitmix64(np.uint64(key) + (idx >> 2).astype(np.uint64))
    return ((h >> (np.uint64(16) * (idx & 3).astype(np.uint64))) & np.uint64(0xFFFF)).astype(np.uint32)


def store(pv, mode, key=0, idx=None):
    """fp32 result -> (bf16 weight as float32, compensation word as float32 or None)"""
    pv = np.asarray(pv, dtype=f)
    if mode == NEAREST:
        return O8.bf16_round(pv), None
    if mode == COMPENSATED:
        p = O8.bf16_round(pv)
        with np.errstate(invalid="ignore"):
            c = O8.bf16_round(pv - p)
        return p, np.where(np.isfinite(pv), c, f(0)).astype(f)
    assert mode == STOCHASTIC
    bits = pv.view(np.uint32)
    special = (bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    up = ((bits.astype(np.uint64) + draws(key, idx).astype(np.uint64)) & np.uint64(0xFFFF0000)).astype(np.uint32)
    return np.where(special, O8.bf16_round(pv).view(np.uint32), up).view(f), None


def _start(p, comp, mode):
    p = np.asarray(p, dtype=f)
    return p + np.asarray(comp, dtype=f) if mode == COMPENSATED else p


def pv_bnb(w, m, v, lr, b1, b2, eps, wd, t):
    """the lines of oracle step_8bit / step_32bit between the moment update and the rounding: m, v are the NEW moments"""
    c1f = f(1.0 - b1 ** t)
    c2f = f(np.sqrt(1.0 - b2 ** t))
    step = f(-lr) * c2f / c1f
    pn = w.astype(f) + step * (m / (np.sqrt(v) + f(eps) * c2f))
    if wd > 0:
        pn = pn * f(1.0 - lr * wd)
    return pn


def step_8bit_r(p, comp, g, c1, c2, absmax1, absmax2, qmap1, qmap2, lr, b1, b2, eps, wd, t, gscale, mode, key=0,
                idx=None):
    """one tensor with 8-bit state: (p, comp, c1, c2, absmax1, absmax2)"""
    w = _start(p, comp, mode)
    blk = np.arange(w.size) // O8.BLOCK
    gg = g.astype(f) * f(gscale)
    m = f(b1) * (qmap1[c1].astype(f) * absmax1[blk].astype(f)) + f(1.0 - b1) * gg
    v = f(b2) * (qmap2[c2].astype(f) * absmax2[blk].astype(f)) + f(1.0 - b2) * (gg * gg)
    _, n1, n2, a1, a2 = O8.step_8bit(w, g, c1, c2, absmax1, absmax2, qmap1, qmap2, lr, b1, b2, eps, wd, t, gscale)
    pn, cn = store(pv_bnb(w, m, v, lr, b1, b2, eps, wd, t), mode, key, idx)
    return pn, cn, n1, n2, a1, a2


def step_32bit_r(p, comp, g, m, v, lr, b1, b2, eps, wd, t, gscale, mode, key=0, idx=None):
    """one tensor below min_8bit_size (fp32 moments, bnb's formula): (p, comp, m, v)"""
    w = _start(p, comp, mode)
    _, m, v = O8.step_32bit(w, g, m, v, lr, b1, b2, eps, wd, t, gscale)
    pn, cn = store(pv_bnb(w, m, v, lr, b1, b2, eps, wd, t), mode, key, idx)
    return pn, cn, m, v


def step_adamw_r(p, comp, g, m, v, lr, b1, b2, eps, wd, t, gscale, mode, key=0, idx=None):
    """fp32-moment AdamW in adamw_kernel's order, each operation rounded to float32: (p, comp, m, v)"""
    w = _start(p, comp, mode)
    lr, b1f, b2f = f(lr), f(b1), f(b2)
    bc1, bc2 = f(1 - b1 ** t), f(1 - b2 ** t)
    gr = g.astype(f) * f(gscale)
    pv = w * (f(1) - lr * f(wd))
    m = b1f * m.astype(f) + (f(1) - b1f) * gr
    v = b2f * v.astype(f) + ((f(1) - b2f) * gr) * gr
    pv = pv - ((lr / bc1) * m) / (np.sqrt(v) / np.sqrt(bc2) + f(eps))
    pn, cn = store(pv, mode, key, idx)
    return pn, cn, m, v


# ------------------------------------------------------------------------------------------ the stall experiment --
STALL_N, STALL_LR, STALL_STEPS = 4096, 5e-5, 64


def stall_weights(n=STALL_N, seed=0):
    """bf16 weights (as float32) with magnitude in [2^-6 + 2^-12, 2^-4) and random sign: an lr = 5e-5 step is below
    half an ulp (2^-14 = 6.1e-5 from 2^-6 up) of every one of them"""
    rng = np.random.default_rng(seed)
    lo, hi = 2.0 ** -6 + 2.0 ** -12, 2.0 ** -4
    # lo and hi - 2^-12 (the largest bf16 below hi) are bf16 values, so the clip only undoes a rounding up to hi
    mag = np.clip(O8.bf16_round((lo + (hi - lo) * rng.random(n)).astype(f)), f(lo), f(hi - 2.0 ** -12))
    assert (mag == O8.bf16_round(mag)).all() and (mag >= f(lo)).all() and (mag < f(hi)).all()
    return (mag * np.where(rng.random(n) < 0.5, f(-1), f(1))).astype(f)


def ulp_bf16(x):
    """the bf16 ulp (2^-7 of the binade) at |x|"""
    return np.exp2(np.floor(np.log2(np.abs(x).astype(np.float64))) - 7)


def err_ulps(p, master):
    """|p - master| in bf16 ulps taken at the larger binade of the two"""
    p, master = np.asarray(p, np.float64), np.asarray(master, np.float64)
    return np.abs(p - master) / np.maximum(ulp_bf16(p), ulp_bf16(master))


def comp_bound(steps):
    """half an ulp for the final rounding + per step at most one bf16 rounding of c (relative 2^-9 of at most half an
    ulp), doubled for slack"""
    return 0.5 + steps * 2.0 ** -9


def run_stall(step_fn, mode, steps=STALL_STEPS, seed=0, lr=STALL_LR, n=STALL_N, base=0, sl=slice(None), rng_seed=0):
    """``steps`` steps of constant gradient +1 on stall_weights()[sl] with one of the fp32-moment step functions
    (step_32bit_r / step_adamw_r); the same expression on unrounded fp32 weights is the master.  Returns
    (p0, p, comp, master)."""
    p0 = stall_weights(n, seed)[sl]
    k = p0.size
    idx = base + np.arange(n, dtype=np.int64)[sl]
    g = np.ones(k, f)
    p, comp = p0.copy(), np.zeros(k, f)
    m, v = np.zeros(k, f), np.zeros(k, f)
    master, mm, mv = p0.copy(), np.zeros(k, f), np.zeros(k, f)
    for t in range(1, steps + 1):
        p, c, m, v = step_fn(p, comp, g, m, v, lr, 0.9, 0.999, 1e-8, 0.0, t, 1.0, mode, step_key(rng_seed, t), idx)
        comp = c if c is not None else comp
        master, mm, mv = master_step(step_fn, master, g, mm, mv, lr, t)
    return p0, p, comp, master


def master_step(step_fn, master, g, m, v, lr, t):
    """one step of the same float32 expression on fp32 weights that are never rounded to bf16"""
    w = np.asarray(master, f)
    if step_fn is step_adamw_r:
        lrf = f(lr)
        bc1, bc2 = f(1 - 0.9 ** t), f(1 - 0.999 ** t)
        m = f(0.9) * m + (f(1) - f(0.9)) * g
        v = f(0.999) * v + ((f(1) - f(0.999)) * g) * g
        return w - ((lrf / bc1) * m) / (np.sqrt(v) / np.sqrt(bc2) + f(1e-8)), m, v
    _, m, v = O8.step_32bit(w, g, m, v, lr, 0.9, 0.999, 1e-8, 0.0, t, 1.0)
    return pv_bnb(w, m, v, lr, 0.9, 0.999, 1e-8, 0.0, t), m, v
