"""8-bit AdamW step over a Pi0-sized parameter arena (SigLIP 27 layers + Gemma 18 + the action expert 18: 2.7 B
bf16 parameters in ~800 tensors, one contiguous run), HIP-event timed, with the algorithmic bytes (10 B / element:
p and g read, p written, two 1-byte state codes read and written) and the rate.

    python tools/optim_bench.py [--iters 10] [--rounding nearest|compensated|stochastic|all]

``--rounding`` picks FusedAdamW's weight store; compensated moves 14 B / element (the compensation word
is read and written too).  ``all`` times the three modes against each other (profiles/optim/rounding_bench.txt): one
optimizer per mode over the same weights and gradients, their steps alternating in one process, every step timed by
its own pair of HIP events after ``--warmup`` untimed rounds; the median, minimum, maximum and spread of each mode
are printed with its ratio to nearest, and the last line is one JSON object with every figure.
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-pi-zero_amd"))

import torch  # noqa: E402

BYTES = {"nearest": 10, "compensated": 14, "stochastic": 10}  # HBM traffic per element


def shapes():
    out = []
    for _ in range(27):  # SigLIP So400m/14 layer
        out += [(1152, 1152)] * 3 + [(1152,)] * 3 + [(1152, 1152), (1152,), (4304, 1152), (4304,), (1152, 4304),
                                                     (1152,), (1152,), (1152,), (1152,), (1152,)]
    for _ in range(18):  # Gemma-2B layer
        out += [(2048, 2048), (256, 2048), (256, 2048), (2048, 2048), (16384, 2048), (16384, 2048), (2048, 16384),
                (2048,), (2048,)]
    for _ in range(18):  # action expert layer
        out += [(2048, 1024), (256, 1024), (256, 1024), (1024, 2048), (4096, 1024), (4096, 1024), (1024, 4096),
                (1024,), (1024,)]
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounding", default="nearest", choices=["nearest", "compensated", "stochastic", "all"])
    a = ap.parse_args()
    from pizero_native.optim import FusedAdamW

    sh = shapes()
    n = [int(torch.tensor(s).prod()) for s in sh]
    pad = [(k + 7) // 8 * 8 for k in n]
    total = sum(pad)
    dev = "cuda"
    w = (torch.rand(total, device=dev) * 0.2 - 0.1).to(torch.bfloat16)
    gbuf = (torch.randn(total, device=dev) * 1e-3).to(torch.bfloat16)
    params, o = [], 0
    for s, k, kp in zip(sh, n, pad):
        p = torch.nn.Parameter(w[o:o + k].view(s))
        p.grad = gbuf[o:o + k].view(s)
        params.append(p)
        o += kp
    elems = sum(n)
    if a.rounding != "all":
        opt = FusedAdamW(params, lr=1e-4, weight_decay=0.01, state_bits=8, rounding=a.rounding)
        for _ in range(a.warmup):
            opt.step()
        torch.cuda.synchronize()
        e0, e1 = timed(lambda: [opt.step() for _ in range(a.iters)])
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        b = BYTES[a.rounding]
        print(f"adamw8 step ({a.rounding}): {len(sh)} tensors, {elems / 1e9:.3f} B elements: {ms:.3f} ms, "
              f"{elems * b / ms / 1e9:.2f} TB/s of {b} B / element", flush=True)
        return
    modes = ["nearest", "compensated", "stochastic"]
    opts = {m: FusedAdamW(params, lr=1e-4, weight_decay=0.01, state_bits=8, rounding=m) for m in modes}
    for _ in range(a.warmup):
        for m in modes:
            opts[m].step()
    torch.cuda.synchronize()
    ev = {m: [] for m in modes}
    for _ in range(a.iters):
        for m in modes:
            ev[m].append(timed(opts[m].step))
    torch.cuda.synchronize()
    print(f"{len(sh)} tensors, {elems / 1e9:.3f} B elements, 8-bit state, {a.iters} timed steps per mode, alternating, "
          f"after {a.warmup} warm-up rounds", flush=True)
    out = {"elements": elems, "iters": a.iters}
    for m in modes:
        ms = [e0.elapsed_time(e1) for e0, e1 in ev[m]]
        med, lo, hi = statistics.median(ms), min(ms), max(ms)
        out[m] = {"median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                  "tb_per_s": round(elems * BYTES[m] / med / 1e9, 3)}
    for m in modes:
        r = out[m]
        r["ratio_to_nearest"] = round(r["median_ms"] / out["nearest"]["median_ms"], 4)
        print(f"{m:<12} median {r['median_ms']:8.3f} ms   min {r['min_ms']:8.3f}   max {r['max_ms']:8.3f}   spread "
              f"{(r['max_ms'] - r['min_ms']) / r['median_ms'] * 100:5.1f} %   {r['tb_per_s']:6.2f} TB/s of "
              f"{BYTES[m]} B / element   x{r['ratio_to_nearest']:.3f} of nearest", flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
