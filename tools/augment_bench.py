"""Cost of the on-device image augmentation beside today's normalisation (profiles/augment/).

    python tools/augment_bench.py [--frames 256] [--size 224] [--reps 50] [--warmup 5] [--host-reps 1] [--out FILE]

One micro-batch of uint8 frames [n, 3, S, S] on the device (noise: the kernels' time does not depend on the content).
HIP-event times of
  (a) norm     TrainAgent.preprocess_batch's normalisation expression, ((x.float() / 255 - 0.5) / 0.5).to(bf16);
  (b) augment  ops.image_augment with all five ops (parameters drawn by pizero_native.augment.draw_params from the
               reference's primary-camera settings, already on the device -- the upload of 9 KiB is not the kernel);
  (b') draw    host wall time of draw_params for the micro-batch (what (b) costs the host besides the two launches);
alternating repetition by repetition in one process, medians of ``--reps`` after ``--warmup``; and
  (c) numpy    host wall time of the fp64 numpy restatement (tests/augment_ref.py) on the same frames and parameters:
               what a host-side augmentation of this micro-batch would cost, ``--host-reps`` runs.
The text goes to stdout and to ``--out``, then one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-pi-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment", "augment_bench.txt"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from pizero_native import augment as A
    from pizero_native import ops
    from tests import augment_ref as R

    if not torch.cuda.is_available():
        raise SystemExit("augment_bench measures on the GPU: no device found")
    n, S = a.frames, a.size
    host = np.random.default_rng(0).integers(0, 256, (n, 3, S, S), dtype=np.uint8)
    frames = torch.from_numpy(host).cuda()
    specs = A.parse_kwargs(A.REFERENCE_PRIMARY)
    params, mask = A.draw_params(specs, n, seed=0, cnt_batch=0, rank=0)
    d_params, d_mask = torch.from_numpy(params).cuda(), torch.from_numpy(mask).cuda()
    out = torch.empty(n, 3, S, S, device="cuda", dtype=torch.bfloat16)
    scratch = torch.empty(ops.image_augment_scratch_numel(n, S), device="cuda", dtype=torch.float32)

    def norm():
        return ((frames.to(torch.float32) / 255.0 - 0.5) / 0.5).to(torch.bfloat16)

    def augment():
        return ops.image_augment(frames, d_params, d_mask, out=out, scratch=scratch)

    paths = {"norm": norm, "augment": augment}
    ms = {k: [] for k in paths}
    draw_ms = []
    for rep in range(a.warmup + a.reps):
        for k, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        A.draw_params(specs, n, seed=0, cnt_batch=rep, rank=0)
        if rep >= a.warmup:
            draw_ms.append((time.perf_counter() - t0) * 1e3)
    host_ms = []
    codes = None
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        codes = R.host_augment_codes(host, params, mask)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    # the two agree up to the code boundaries (tests/test_augment_gpu.py holds every pixel to 0.01 of one)
    lut = ops.pixel_code_lut("cuda").float()
    got = torch.searchsorted(lut, augment().float().contiguous()).clamp_(0, 255).cpu().numpy()
    differ = float((got != codes).mean())
    worst = int(np.abs(got.astype(np.int32) - codes.astype(np.int32)).max())

    mb = n * 3 * S * S
    res = {"frames": n, "size": S, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "norm_ms": round(statistics.median(ms["norm"]), 4), "augment_ms": round(statistics.median(ms["augment"]), 4),
           "norm_min_max_ms": [round(min(ms["norm"]), 4), round(max(ms["norm"]), 4)],
           "augment_min_max_ms": [round(min(ms["augment"]), 4), round(max(ms["augment"]), 4)],
           "draw_params_ms": round(statistics.median(draw_ms), 4),
           "numpy_host_ms": round(statistics.median(host_ms), 1), "host_reps": a.host_reps,
           "host_cpus": os.cpu_count(), "codes_differing_share": differ, "codes_max_abs_diff": worst}
    # bytes the augmentation has to move at least: the frames twice when the contrast is on (one read per pass;
    # the bilinear gather's four texels per channel overlap between neighbouring lanes) and the bf16 output once
    res["augment_min_bytes"] = mb * 2 + mb * 2
    res["augment_gbps_of_min_bytes"] = round(res["augment_min_bytes"] / (res["augment_ms"] * 1e-3) / 1e9, 1)
    lines = [
        f"{n} uint8 frames [3, {S}, {S}] on {res['device']}; HIP-event medians of {a.reps} repetitions after "
        f"{a.warmup} warm-up, the two device paths alternating in one process",
        f"(a) norm     ((x.float() / 255 - 0.5) / 0.5).to(bf16)          {res['norm_ms']:9.4f} ms   "
        f"(min {res['norm_min_max_ms'][0]:.4f}, max {res['norm_min_max_ms'][1]:.4f})",
        f"(b) augment  ops.image_augment, crop + 4 colour ops, 2 launches {res['augment_ms']:9.4f} ms   "
        f"(min {res['augment_min_max_ms'][0]:.4f}, max {res['augment_min_max_ms'][1]:.4f})   "
        f"{res['augment_min_bytes'] / 1e6:.0f} MB least traffic -> {res['augment_gbps_of_min_bytes']:.0f} GB/s of it",
        f"(b') draw    augment.draw_params on the host                    {res['draw_params_ms']:9.4f} ms   (host wall)",
        f"(c) numpy    fp64 restatement of the same chain on the host    {res['numpy_host_ms']:9.1f} ms   "
        f"(host wall, median of {a.host_reps}; {res['host_cpus']} CPUs visible, numpy single-threaded here)",
        f"(b) / (a) = {res['augment_ms'] / res['norm_ms']:.2f};  "
        f"(c) / (b) = {res['numpy_host_ms'] / res['augment_ms']:.0f};  "
        f"codes of (b) and (c) differ in {100 * differ:.4f} % of the values, by at most {worst}",
    ]
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n" + json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
