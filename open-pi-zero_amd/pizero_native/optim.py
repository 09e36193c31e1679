"""Fused flat AdamW + gradient-norm clipping over the parameter arena.

Replaces the reference's two bitsandbytes AdamW8bit optimizers and
``torch.nn.utils.clip_grad_norm_`` (train.py:171-198, 371-379).  Parameters
are views of one flat arena, so a param group collapses to a few contiguous
runs: one ``pz_adamw`` launch per run instead of one kernel chain per tensor.
Update rule = torch.optim.AdamW (decoupled weight decay, bias correction);
moments are fp32 (the reference's 8-bit blockwise states are not reproduced:
bitsandbytes is absent here, parity for the optimizer is pinned against
torch.optim.AdamW instead -- SURVEY 8(c)).

``state_bits=8`` (``AdamW8bit``) keeps the reference's blockwise 8-bit state instead
(bnb.optim.AdamW8bit, train.py:171-175,194-198): uint8 codes of m / v into the signed / unsigned
dynamic-tree maps with one fp32 absmax per 256 elements of a tensor, fp32 state for tensors below
4096 elements, bnb's update formula -- one ``pz_adamw8bit`` launch per contiguous run, 10 B of HBM
traffic per element instead of 22, and 5.2 GB of state for the 2.6 B trained elements instead of
20.9 GB.  The algorithm is restated from the published bitsandbytes one (oracle/adamw8bit.py, which
the GPU tests hold the kernel bit-exact against); bitsandbytes itself is absent, so parity with it
is unpinned.

Checkpoints: ``state_dict()`` has torch.optim.AdamW's layout (per-parameter
``step`` / ``exp_avg`` / ``exp_avg_sq``, param_groups with integer ids) for 32-bit state and
bnb's (``state1`` / ``state2`` / ``absmax1`` / ``absmax2`` / ``qmap1`` / ``qmap2`` / ``step``)
for 8-bit state; ``load_state_dict`` accepts either layout in either mode (8-bit codes are
dequantised, fp32 moments quantised).  State tensors are views of the flat buffers (torch.save
stores each buffer once).  The global gradient norm is reduced without atomics (fixed
partial-sum order), so clipping -- and training -- is bitwise reproducible.

``rounding``.  The weights are bf16 only, and with ``"nearest"`` (the default: exactly the kernels
and the state of before) a step smaller than half an ulp of a weight is rounded away in full -- at lr 5e-5 that is
every weight with |p| >= 2^-6.  ``"compensated"`` keeps a second bf16 word per weight (one flat buffer per run,
+2 B per trained element) that carries what the rounding dropped into the next step; ``"stochastic"`` needs no
state and rounds up or down with the probability that makes the stored weight unbiased.  Its draws are a pure
function of (``seed``, the group's step, the element's index in the arena storage), so they do not depend on how
parameters fall into runs or optimizers and are identical on every data-parallel rank.  In compensated mode every
parameter's state gains ``"comp"`` (a bf16 view shaped like the parameter); ``rounding`` and ``seed`` are in the
param_groups of the two new modes.  ``load_state_dict`` keeps the optimizer's own ``rounding``: a state without
``"comp"`` starts it from zeros, a ``"comp"`` loaded into another mode is dropped; ``seed`` is taken from the
loaded state (as the other hyperparameters are) when both sides have one.  Writes to the weights from outside
the optimizer -- ``model.load_state_dict`` after construction, ``FlatAverage.swapped()`` -- leave the
compensation word describing the weight it was computed for: stale by less than half an ulp of that weight,
which is harmless (it is the size of one rounding), not an error that grows.
"""

from __future__ import annotations

import os

import torch
from torch.autograd.graph import increment_version

from . import ops
from ._lib import PZ_SUMSQ_PARTS

_CHECK_FINITE = os.environ.get("PZ_CHECK_FINITE", "0") == "1"  # debug: check the updated weights (engine._chk)
BLOCK8 = 256  # elements per absmax block (bnb blockwise 2-state optimizers)
MIN_8BIT_SIZE = 4096  # bnb Optimizer8bit min_8bit_size: smaller tensors keep fp32 state
ROUNDINGS = ("nearest", "compensated", "stochastic")  # FusedAdamW(rounding=...): how pv becomes the bf16 weight


def create_dynamic_map(signed=True, max_exponent_bits=7, total_bits=8):
    """bitsandbytes' dynamic (tree) quantisation map: 256 sorted float32 values, built with the same
    float32 torch arithmetic as bnb's functional.create_dynamic_map (float32 linspace, float32 means and
    scale products), so the entries match bnb's saved qmap1 / qmap2 to the bit."""
    data = []
    nsb = total_bits - 1
    for i in range(max_exponent_bits):
        n = 2 ** (i + nsb - max_exponent_bits) + 1 if signed else 2 ** (i + nsb - max_exponent_bits + 1) + 1
        b = torch.linspace(0.1, 1, n)
        means = (b[:-1] + b[1:]) / 2.0
        sc = 10 ** (-(max_exponent_bits - 1) + i)
        data += (sc * means).tolist()
        if signed:
            data += (-sc * means).tolist()
    data += [0.0, 1.0]
    data += [0.0] * (2 ** total_bits - len(data))
    return torch.tensor(sorted(data), dtype=torch.float32)


def _quantize_nearest(x, qmap):
    """uint8 codes of the nearest map entries (state conversion on load; the kernel's own
    requantisation uses the bnb binary search)."""
    i = torch.searchsorted(qmap, x.contiguous()).clamp(1, qmap.numel() - 1)
    lo, hi = qmap[i - 1], qmap[i]
    return torch.where((x - lo).abs() <= (hi - x).abs(), i - 1, i).to(torch.uint8)


def contiguous_runs(params):
    """Merge parameters whose storage is adjacent (gaps < 16 B of arena padding)."""
    ps = sorted([p for p in params], key=lambda p: p.data_ptr())
    runs = []
    for p in ps:
        if runs:
            last = runs[-1]
            end = last["ptr"] + last["n"] * p.element_size()
            gap = p.data_ptr() - end
            if 0 <= gap < 16 and p.untyped_storage().data_ptr() == last["base"].untyped_storage().data_ptr():
                last["n"] = (p.data_ptr() - last["ptr"]) // p.element_size() + p.numel()
                last["params"].append(p)
                continue
        runs.append({"ptr": p.data_ptr(), "n": p.numel(), "params": [p], "base": p})
    out = []
    for r in runs:
        b = r["base"]
        st = b.untyped_storage()
        full = torch.empty(0, dtype=b.dtype, device=b.device).set_(st)
        off = (r["ptr"] - st.data_ptr()) // b.element_size()
        out.append((full[off : off + r["n"]], r["params"], off))
    return out


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, state_bits=32,
                 rounding="nearest", seed=0):
        if state_bits not in (32, 8):
            raise ValueError("state_bits must be 32 or 8")
        if rounding not in ROUNDINGS:
            raise ValueError(f"rounding must be one of {', '.join(ROUNDINGS)}, got {rounding!r}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.state_bits = state_bits
        self.rounding = rounding
        self.seed = int(seed)
        if rounding != "nearest":  # the nearest-mode param_groups (and state dict) keep exactly their keys
            for group in self.param_groups:
                group["rounding"], group["seed"] = rounding, int(seed)
        self._runs = None
        self._gscale = None
        self._parts = None

    def _prepare(self):
        if self._runs is not None:
            return
        self._runs = []
        dev = None
        for group in self.param_groups:
            runs = []
            for flat, plist, off in contiguous_runs(group["params"]):
                dev = flat.device
                r = dict(flat=flat, params=plist, off=off)  # off: the run's element offset in the arena storage
                if self.rounding == "compensated":
                    r["comp"] = torch.zeros(flat.numel(), device=dev, dtype=flat.dtype)
                if self.state_bits == 32:
                    r["m"] = torch.zeros(flat.numel(), device=dev, dtype=torch.float32)
                    r["v"] = torch.zeros_like(r["m"])
                else:
                    self._prepare_8bit(r)
                runs.append(r)
            self._runs.append(runs)
        if self.state_bits == 8 and dev is not None:
            self._qmap1 = create_dynamic_map(True).to(dev)
            self._qmap2 = create_dynamic_map(False).to(dev)

    @staticmethod
    def _prepare_8bit(r):
        """Segment table of one run: {offset, numel, first block, fp32-state offset or -1} per tensor."""
        flat = r["flat"]
        base, es = flat.data_ptr(), flat.element_size()
        rows, blocks, n32, info = [], 0, 0, {}
        for p in sorted(r["params"], key=lambda q: q.data_ptr()):
            o = (p.data_ptr() - base) // es
            if o % 4:  # pz_adamw8bit loads 4 codes / 4 bf16 elements per access from a segment start
                raise ValueError(f"FusedAdamW(state_bits=8): parameter segment at element offset {o} is not "
                                 "4-element aligned (arena parameters are 8-aligned; pass arena views)")
            nb = (p.numel() + BLOCK8 - 1) // BLOCK8
            if p.numel() >= MIN_8BIT_SIZE:
                rows.append([o, p.numel(), blocks, -1])
                info[p] = ("8", o, blocks, nb)
            else:
                rows.append([o, p.numel(), blocks, n32])
                info[p] = ("32", o, n32, nb)
                n32 += p.numel()
            blocks += nb
        dev = flat.device
        r["seg"] = torch.tensor(rows, dtype=torch.int64).to(dev)
        r["nseg"], r["nblocks"], r["info"] = len(rows), blocks, info
        r["s1"] = torch.zeros(flat.numel() + 4, device=dev, dtype=torch.uint8)
        r["s2"] = torch.zeros_like(r["s1"])
        r["absmax1"] = torch.zeros(blocks, device=dev, dtype=torch.float32)
        r["absmax2"] = torch.zeros_like(r["absmax1"])
        r["m32"] = torch.zeros(max(n32, 1), device=dev, dtype=torch.float32)
        r["v32"] = torch.zeros_like(r["m32"])

    def state_bytes(self):
        """Device bytes of optimizer state (reported by bench.py)."""
        self._prepare()
        keys = ("m", "v") if self.state_bits == 32 else ("s1", "s2", "absmax1", "absmax2", "m32", "v32")
        if self.rounding == "compensated":
            keys += ("comp",)
        return sum(r[k].numel() * r[k].element_size() for runs in self._runs for r in runs for k in keys)

    def _moment_views(self):
        """param -> (exp_avg view, exp_avg_sq view) into the flat fp32 moment buffers (32-bit state)."""
        self._prepare()
        out = {}
        for runs in self._runs:
            for r in runs:
                base, es = r["flat"].data_ptr(), r["flat"].element_size()
                for p in r["params"]:
                    o = (p.data_ptr() - base) // es
                    out[p] = (r["m"][o:o + p.numel()].view(p.shape), r["v"][o:o + p.numel()].view(p.shape))
        return out

    def _state8_views(self):
        """param -> bnb-layout state views (8-bit state)."""
        self._prepare()
        out = {}
        for runs in self._runs:
            for r in runs:
                for p, (kind, o, b, nb) in r["info"].items():
                    if kind == "8":
                        out[p] = {"state1": r["s1"][o:o + p.numel()].view(p.shape),
                                  "state2": r["s2"][o:o + p.numel()].view(p.shape),
                                  "absmax1": r["absmax1"][b:b + nb], "absmax2": r["absmax2"][b:b + nb]}
                    else:
                        out[p] = {"state1": r["m32"][b:b + p.numel()].view(p.shape),
                                  "state2": r["v32"][b:b + p.numel()].view(p.shape)}
        return out

    def _comp_views(self):
        """param -> its compensation words, a bf16 view shaped like the parameter (compensated mode)."""
        self._prepare()
        out = {}
        for runs in self._runs:
            for r in runs:
                base, es = r["flat"].data_ptr(), r["flat"].element_size()
                for p in r["params"]:
                    o = (p.data_ptr() - base) // es
                    out[p] = r["comp"][o:o + p.numel()].view(p.shape)
        return out

    def _n_runs(self):
        self._prepare()
        return sum(len(runs) for runs in self._runs)

    def _flat_grad(self, run):
        """Gradient run as a flat view (grads are arena views laid out like the params)."""
        p0 = run["params"][0]
        g0 = p0.grad
        if g0 is None:
            return None
        st = g0.untyped_storage()
        full = torch.empty(0, dtype=g0.dtype, device=g0.device).set_(st)
        off = (g0.data_ptr() - st.data_ptr()) // g0.element_size()
        flat = full[off : off + run["flat"].numel()]
        # verify the layout assumption once per gradient layout: the key holds EVERY parameter's gradient pointer
        # (None for a missing one), so a grad set to None or replaced by a non-arena tensor anywhere in the run
        # changes it and is re-checked; comparing the pointer list costs ~0.2 us per tensor
        key = [p.grad.data_ptr() if p.grad is not None else None for p in run["params"]]
        if run.get("gkey") != key:
            base_p, base_g = run["flat"].data_ptr(), flat.data_ptr()
            for p in run["params"]:
                if p.grad is None or p.grad.data_ptr() - base_g != p.data_ptr() - base_p:
                    raise RuntimeError("FusedAdamW: gradients are not arena views; use the native PiZero backward")
            run["gkey"] = key
        return flat

    def clip_grad_norm_(self, max_norm):
        """clip_grad_norm_ over every param of this optimizer; coefficient applied inside step().
        Returns the total norm as a device tensor (no host sync)."""
        return clip_grad_norm_([self], max_norm)

    def set_grad_scale(self, coef):
        self._gscale = coef

    @torch.no_grad()
    def step(self, closure=None):
        self._prepare()
        for group, runs in zip(self.param_groups, self._runs):
            b1, b2 = group["betas"]
            group["step"] = group.get("step", 0) + 1
            t = group["step"]
            for r in runs:
                g = self._flat_grad(r)
                if g is None:
                    continue
                if self.rounding != "nearest":
                    self._step_rounded(group, r, g, t)
                elif self.state_bits == 32:
                    ops.adamw(r["flat"], g, r["m"], r["v"], group["lr"], b1, b2, group["eps"],
                              group["weight_decay"], 1 - b1 ** t, 1 - b2 ** t, self._gscale)
                else:
                    ops.adamw8bit(r, g, self._qmap1, self._qmap2, group["lr"], b1, b2, group["eps"],
                                  group["weight_decay"], t, self._gscale)
                # the kernels write through raw pointers: bump the parameters' (shared arena) version
                # counter so weight-derived caches (the fp8 inference codes) see the change
                increment_version(r["params"][0])
                if _CHECK_FINITE:
                    from .engine import check_finite

                    check_finite(f"FusedAdamW.step (group lr {group['lr']:g})", param=r["flat"])
        self._gscale = None

    def _step_rounded(self, group, r, g, t):
        """One run's step with the compensated / stochastic weight store (pz_adamw_r / pz_adamw8bit_r)."""
        b1, b2 = group["betas"]
        kw = dict(mode=ops.ROUND_COMPENSATED, rng_key=0, rng_base=r["off"])
        if self.rounding == "stochastic":
            kw.update(mode=ops.ROUND_STOCHASTIC,
                      rng_key=ops.splitmix64((int(group.get("seed", self.seed)) + t) & (2 ** 64 - 1)))
        if self.state_bits == 32:
            ops.adamw_r(r["flat"], r.get("comp"), g, r["m"], r["v"], group["lr"], b1, b2, group["eps"],
                        group["weight_decay"], 1 - b1 ** t, 1 - b2 ** t, self._gscale, **kw)
        else:
            ops.adamw8bit_r(r, g, self._qmap1, self._qmap2, group["lr"], b1, b2, group["eps"],
                            group["weight_decay"], t, self._gscale, comp=r.get("comp"), **kw)

    def zero_grad(self, set_to_none: bool = True):
        for group in self.param_groups:
            for p in group["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    # ------------------------------------------------------------ checkpoints --
    def state_dict(self):
        """32-bit: torch.optim.AdamW layout {i: {step, exp_avg, exp_avg_sq}}; 8-bit: bnb's layout
        {i: {step, state1, state2, absmax1, absmax2, qmap1, qmap2}} (fp32 state1/state2 for small
        tensors); param_groups with integer ids.  Compensated rounding: every parameter's state also has "comp";
        compensated / stochastic: the param_groups also have "rounding" and "seed"."""
        self._prepare()
        views = self._moment_views() if self.state_bits == 32 else self._state8_views()
        comp = self._comp_views() if self.rounding == "compensated" else None
        state, groups, i = {}, [], 0
        for group in self.param_groups:
            ids = []
            step = group.get("step", 0)
            for p in group["params"]:
                if step > 0:
                    if self.state_bits == 32:
                        m, v = views[p]
                        state[i] = {"step": torch.tensor(float(step)), "exp_avg": m, "exp_avg_sq": v}
                    else:
                        st = dict(views[p])
                        st["step"] = step
                        if "absmax1" in st:
                            st["qmap1"], st["qmap2"] = self._qmap1, self._qmap2
                        state[i] = st
                    if comp is not None:
                        state[i]["comp"] = comp[p]
                ids.append(i)
                i += 1
            g = {k: v for k, v in group.items() if k != "params"}
            g["params"] = ids
            groups.append(g)
        return {"state": state, "param_groups": groups}

    def _same_qmaps(self, s):
        """True if a saved 8-bit state's maps equal this optimizer's (else its codes are dequantised with
        the SAVED maps and requantised into ours)."""
        for k, q in (("qmap1", self._qmap1), ("qmap2", self._qmap2)):
            if k in s and not torch.equal(s[k].to(q.device, torch.float32).reshape(-1), q):
                return False
        return True

    @staticmethod
    def _fp32_moments(s, p, dev):
        """(m, v) fp32 on dev from a saved per-parameter state of either layout."""
        if "exp_avg" in s:
            return s["exp_avg"].to(dev, torch.float32), s["exp_avg_sq"].to(dev, torch.float32)
        s1, s2 = s["state1"].to(dev), s["state2"].to(dev)
        if s1.dtype != torch.uint8:
            return s1.to(torch.float32), s2.to(torch.float32)
        blk = torch.arange(p.numel(), device=dev) // BLOCK8
        q1, q2 = s["qmap1"].to(dev, torch.float32), s["qmap2"].to(dev, torch.float32)
        m = q1[s1.reshape(-1).long()] * s["absmax1"].to(dev, torch.float32)[blk]
        v = q2[s2.reshape(-1).long()] * s["absmax2"].to(dev, torch.float32)[blk]
        return m.view(p.shape), v.view(p.shape)

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts the torch.optim.AdamW layout or bnb's AdamW8bit layout, in either state mode:
        moments are copied (fp32 <- fp32, codes <- codes) or converted (dequantised / quantised
        with a per-block absmax).  The rounding mode stays this optimizer's: "comp" is copied in compensated mode
        (zeros where the state has none) and ignored in the others."""
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        self._prepare()
        views = self._moment_views() if self.state_bits == 32 else self._state8_views()
        comp = self._comp_views() if self.rounding == "compensated" else None
        st = state_dict["state"]
        for group, sg in zip(self.param_groups, saved):
            if len(sg["params"]) != len(group["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of "
                                 "optimizer's group")
            step = sg.get("step", None)
            for pid, p in zip(sg["params"], group["params"]):
                s = st.get(pid)
                dst = views[p]
                if comp is not None:
                    if s is not None and "comp" in s:
                        comp[p].copy_(s["comp"].to(comp[p].device, comp[p].dtype).reshape(comp[p].shape))
                    else:
                        comp[p].zero_()
                if s is None:
                    for x in (dst if isinstance(dst, tuple) else dst.values()):
                        x.zero_()
                    continue
                if step is None and "step" in s:
                    step = int(float(s["step"]))
                if self.state_bits == 32:
                    m, v = self._fp32_moments(s, p, dst[0].device)
                    dst[0].copy_(m)
                    dst[1].copy_(v)
                    continue
                if "absmax1" not in dst:  # small tensor: fp32 state
                    m, v = self._fp32_moments(s, p, dst["state1"].device)
                    dst["state1"].copy_(m)
                    dst["state2"].copy_(v)
                elif ("absmax1" in s and s["state1"].dtype == torch.uint8
                      and self._same_qmaps(s)):  # same 8-bit layout and maps: codes copied as they are
                    for k in ("state1", "state2", "absmax1", "absmax2"):
                        dst[k].copy_(s[k].to(dst[k].device).reshape(dst[k].shape))
                else:  # fp32 moments -> codes with a per-block absmax
                    m, v = self._fp32_moments(s, p, dst["state1"].device)
                    for x, k, q in ((m, "1", self._qmap1), (v, "2", self._qmap2)):
                        xf = x.reshape(-1)
                        nb = dst["absmax" + k].numel()
                        pad = torch.zeros(nb * BLOCK8 - xf.numel(), device=xf.device)
                        am = torch.cat([xf, pad]).abs().view(nb, BLOCK8).amax(1)
                        dst["absmax" + k].copy_(am)
                        blk = torch.arange(xf.numel(), device=xf.device) // BLOCK8
                        nrm = torch.where(am[blk] > 0, xf / am[blk].clamp_min(1e-38), torch.zeros_like(xf))
                        dst["state" + k].copy_(_quantize_nearest(nrm, q).view(p.shape))
            for k, val in sg.items():
                if k == "params" or k == "rounding" or (k == "seed" and self.rounding == "nearest"):
                    continue  # the rounding mode is this optimizer's own
                group[k] = val
            group["step"] = int(step or 0)


def AdamW8bit(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, **_):
    """Drop-in for ``bnb.optim.AdamW8bit`` (train.py:171-175): FusedAdamW with 8-bit blockwise state."""
    return FusedAdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, state_bits=8)


def clip_grad_norm_(optimizers, max_norm):
    """Joint clip over several FusedAdamW optimizers (train.py:371-374 clips the union; same norm and
    coefficient as torch.nn.utils.clip_grad_norm_, total_norm + 1e-6).  No atomics: every run writes
    PZ_SUMSQ_PARTS partials and one kernel sums them in a fixed order.  Returns the norm (device)."""
    opts = list(optimizers)
    n = sum(o._n_runs() for o in opts)
    dev = opts[0]._runs[0][0]["flat"].device
    o0 = opts[0]
    if o0._parts is None or o0._parts.numel() != n * PZ_SUMSQ_PARTS or o0._parts.device != dev:
        o0._parts = torch.empty(n * PZ_SUMSQ_PARTS, device=dev, dtype=torch.float32)
    parts = o0._parts
    k = 0
    for o in opts:
        for runs in o._runs:
            for r in runs:
                sl = parts[k * PZ_SUMSQ_PARTS:(k + 1) * PZ_SUMSQ_PARTS]
                g = o._flat_grad(r)
                if g is None:
                    sl.zero_()
                else:
                    ops.sumsq(g, sl)
                k += 1
    coef = torch.empty(1, device=dev, dtype=torch.float32)
    norm = torch.empty(1, device=dev, dtype=torch.float32)
    ops.clip_coef(parts, coef, norm, max_norm)
    for o in opts:
        o.set_grad_scale(coef)
    return norm
