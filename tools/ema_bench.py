"""Timing of the weight-averaging kernels at the real arena size (profiles/ema/).

    python tools/ema_bench.py [--n 3240000000] [--reps 20] [--warmup 3] [--w 0.01]

Runs ``pz_avg_lerp`` (ops.avg_lerp) over two flat bf16 buffers of the arena's size (3.24 B elements: 2 reads + 1 write
of 2 bytes = 6 B of HBM traffic per element) and, alternating with it in the same process and on the same buffers,
PyTorch-ROCm's own ``avg.lerp_(p, w)`` -- what one would use without writing a kernel.  Every repetition is timed by
its own pair of HIP events after ``--warmup`` untimed rounds; the median, the minimum and the maximum (the spread) of
each are printed with the bandwidth and its share of the 6.29 TB/s float4-copy figure of the MI355X.  ``pz_avg_swap``
(8 B per element) is timed the same way, alone.  The last line is one JSON object with every figure.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-pi-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

COPY_TBS = 6.29  # measured float4 copy bandwidth of the MI355X, TB/s


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def summary(name, ms, bytes_per_el, n):
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    gbs = n * bytes_per_el / (med * 1e-3) / 1e9
    print(f"{name:<22} median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   spread {(hi - lo) / med * 100:5.1f} %   "
          f"{gbs:8.1f} GB/s   {gbs / (COPY_TBS * 1e3) * 100:5.1f} % of {COPY_TBS} TB/s", flush=True)
    return {"median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "gb_per_s": round(gbs, 1),
            "share_of_copy": round(gbs / (COPY_TBS * 1e3), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_240_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--w", type=float, default=1 - 0.99)
    a = ap.parse_args()
    from pizero_native import ops

    n = a.n
    avg = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    p = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    ops.fill_uniform(avg, 1, 0.0, 1.0)
    ops.fill_uniform(p, 2, 0.0, 1.0)
    torch.cuda.synchronize()
    print(f"n = {n} bf16 elements ({n * 2 / 1e9:.2f} GB per buffer), w = {a.w}, {a.reps} timed repetitions each, "
          f"alternating, after {a.warmup} warm-up rounds", flush=True)
    ours = lambda: ops.avg_lerp(avg, p, a.w)  # noqa: E731
    theirs = lambda: avg.lerp_(p, a.w)  # noqa: E731
    swap = lambda: ops.avg_swap(avg, p)  # noqa: E731
    for _ in range(a.warmup):
        ours()
        theirs()
    torch.cuda.synchronize()
    ev = {"ours": [], "torch": [], "swap": []}
    for _ in range(a.reps):
        ev["ours"].append(timed(ours))
        ev["torch"].append(timed(theirs))
    torch.cuda.synchronize()
    swap()
    for _ in range(a.reps):
        ev["swap"].append(timed(swap))
    torch.cuda.synchronize()
    ms = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
    out = {"n": n, "w": a.w, "reps": a.reps,
           "pz_avg_lerp": summary("pz_avg_lerp", ms["ours"], 6, n),
           "torch_lerp_": summary("torch lerp_", ms["torch"], 6, n),
           "pz_avg_swap": summary("pz_avg_swap", ms["swap"], 8, n)}
    out["lerp_ratio_ours_over_torch"] = round(out["pz_avg_lerp"]["median_ms"] / out["torch_lerp_"]["median_ms"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
