"""Wall time from "raw camera frame in host memory" to "actions in host memory" (profiles/obs_path_ab.txt).

    python tools/obs_bench.py [--steps 200] [--warmup 20] [--hw 480 640]
    python tools/obs_bench.py --only-act --steps 50            # the program to put under a kernel trace
    python tools/obs_bench.py --split <dir or kernel_trace.csv>  # front-end / back-end share from that trace

B = 1 at the real dims (config/train/bridge.yaml; synthetic weights: a latency does not depend on their values), one
uint8 H x W x 3 frame, raw proprio and a tokenised prompt per control step.  Two paths, alternating step by step in one
process so that both see the same machine state:

  (a) host   PIL.Image.resize(LANCZOS) to the model's size, host pixel and proprio normalisation (BaseEnvAdapter),
             EvalAgent.infer_chunk with the graph, host denormalisation of the chunk -- the path before EvalAgent.act;
  (b) act    EvalAgent.act: the raw frame, proprio and prefix count are copied to the graph's static buffers, one
             replay does resize + normalisations + chunk + denormalisation, the result is copied back.

Every step is timed by the host clock between a device synchronise before the frame is touched and the arrival of the
actions in host memory (a blocking copy).  Median, minimum, maximum and the 5th / 95th percentiles of ``--steps`` steps
after ``--warmup`` untimed ones are printed, then one JSON line.  ``--split`` reads a ``rocprofv3 --kernel-trace`` CSV of
an ``--only-act`` run (taken separately: tracing slows the host) and prints, per act step, the kernel time of the
front end (resize, proprio normalisation) and back end (action denormalisation) beside the whole step's.
"""

from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-pi-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FRONT = ("resize_h_kernel", "resize_v_kernel", "proprio_norm_kernel")
BACK = ("action_denorm_kernel",)


def split(path):
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"),
                                                                 recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {path}")
    rows = [r for r in csv.DictReader(open(files[-1])) if r.get("Start_Timestamp") and r.get("End_Timestamp")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731  (us)
    has = lambda r, names: any(n in r["Kernel_Name"] for n in names)  # noqa: E731
    starts = [i for i, r in enumerate(rows) if "resize_h_kernel" in r["Kernel_Name"]]
    steps = []
    for i in starts:
        j = next((k for k in range(i, len(rows)) if has(rows[k], BACK)), None)
        if j is None:
            break
        seg = rows[i:j + 1]
        steps.append(dict(kernels=len(seg), front=sum(dur(r) for r in seg if has(r, FRONT)),
                          back=sum(dur(r) for r in seg if has(r, BACK)), busy=sum(map(dur, seg)),
                          wall=(int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])) / 1e3,
                          parts={n: sum(dur(r) for r in seg if n in r["Kernel_Name"]) for n in FRONT + BACK}))
    if not steps:
        raise SystemExit("no act step (resize_h_kernel .. action_denorm_kernel) in the trace")
    steps = steps[len(steps) // 2:]  # the later half: replays, after warm-up and capture
    med = lambda k: statistics.median(s[k] for s in steps)  # noqa: E731
    out = {"trace": os.path.relpath(files[-1], ROOT) if files[-1].startswith(ROOT) else files[-1],
           "steps": len(steps), "kernels_per_step": int(med("kernels")),
           "front_us": round(med("front"), 2), "back_us": round(med("back"), 2),
           "busy_us": round(med("busy"), 1), "wall_us": round(med("wall"), 1),
           "parts_us": {n: round(statistics.median(s["parts"][n] for s in steps), 2) for n in FRONT + BACK}}
    out["front_share_of_wall"] = round(out["front_us"] / out["wall_us"], 5)
    out["back_share_of_wall"] = round(out["back_us"] / out["wall_us"], 5)
    print(f"kernel trace of {out['steps']} act steps ({out['kernels_per_step']} kernels each), medians per step:")
    print(f"  first kernel start .. last kernel end {out['wall_us']:9.1f} us   kernel time {out['busy_us']:9.1f} us")
    print(f"  front end {out['front_us']:7.2f} us ({out['front_share_of_wall'] * 100:.3f} % of the step)   "
          f"back end {out['back_us']:6.2f} us ({out['back_share_of_wall'] * 100:.3f} %)")
    for n, v in out["parts_us"].items():
        print(f"    {n:22s} {v:7.2f} us")
    print(json.dumps(out), flush=True)


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def summary(name, ms):
    med = statistics.median(ms)
    s = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
         "p05_ms": round(pct(ms, 0.05), 4), "p95_ms": round(pct(ms, 0.95), 4)}
    print(f"{name:<10} median {med:8.3f} ms   min {s['min_ms']:8.3f}   p05 {s['p05_ms']:8.3f}   p95 {s['p95_ms']:8.3f}   "
          f"max {s['max_ms']:8.3f}   ({len(ms)} steps)", flush=True)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hw", type=int, nargs=2, default=[480, 640])
    ap.add_argument("--stats", default=os.path.join(ROOT, "tests", "golden", "bridge_statistics.json"))
    ap.add_argument("--only-act", action="store_true")
    ap.add_argument("--split", default=None)
    a = ap.parse_args()
    if a.split:
        return split(a.split)

    import numpy as np
    import torch
    from PIL import Image

    from pizero_native import ops
    from src.agent.env_adapter.base import BaseEnvAdapter, load_dataset_statistics
    from src.agent.eval import EvalAgent
    from src.agent.train import SyntheticBridgeDataset
    from src.utils.config import load_config

    if not torch.cuda.is_available():
        raise SystemExit("obs_bench measures on the GPU: no device found")
    cfg = load_config(os.path.join(ROOT, "open-pi-zero_amd", "config", "train", "bridge.yaml"),
                      {"env.adapter.dataset_statistics_path": a.stats})
    ag = EvalAgent(cfg, use_graph=True)
    ar = ag.model._arena
    for i, name in enumerate(ar.order):  # synthetic weights, U(+-1/sqrt(fan_in)); vectors zero (Gemma norm = identity)
        v = ar.view(name)
        if v.dim() >= 2:
            ops.fill_uniform(v, 1000 + i, 0.0, float(v.shape[-1]) ** -0.5)
        else:
            v.zero_()
    torch.cuda.synchronize()
    stats = load_dataset_statistics(a.stats)
    ad = BaseEnvAdapter()
    S = int(cfg.vision.config.image_size)
    h, w = a.hw
    b = next(iter(SyntheticBridgeDataset(cfg, 1, seed=1)))
    ids, am = b["input_ids"], b["attention_mask"]
    r = np.random.default_rng(0)
    n_frames = 8  # a few different frames and proprio vectors, cycled
    frames = [r.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n_frames)]
    lo, hi = np.array(stats["proprio"]["p01"]), np.array(stats["proprio"]["p99"])
    props = [(lo + (hi - lo) * r.uniform(0, 1, lo.shape)).astype(np.float32)[None, None] for _ in range(n_frames)]
    noise = torch.randn(1, ag.model.horizon_steps, ag.model.action_dim, device=ag.device)

    def host_path(frame, prop):
        small = np.array(Image.fromarray(frame).resize((S, S), Image.LANCZOS))
        pix = torch.from_numpy(small).permute(2, 0, 1)[None]
        pix = (pix.to(torch.float32) / 255.0 - 0.5) / 0.5
        pn = torch.from_numpy(ad.normalize_proprio(prop, stats, "bound").astype(np.float32))
        chunk = ag.infer_chunk(ids, am, pix, pn, noise=noise).float().cpu().numpy()
        return ad.denormalize_action(chunk, stats, "bound")

    def act_path(frame, prop):
        return ag.act(frame[None], ids, am, prop, noise=noise).cpu().numpy()

    paths = {"act": act_path} if a.only_act else {"host": host_path, "act": act_path}
    ms = {k: [] for k in paths}
    last = {}
    for step in range(a.warmup + a.steps):
        f, p = frames[step % n_frames], props[step % n_frames]
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn(f, p)
            dt = (time.perf_counter() - t0) * 1e3
            if step >= a.warmup:
                ms[k].append(dt)
    print(f"B = 1, {h}x{w} uint8 frame -> {S}x{S}, {a.steps} timed steps per path after {a.warmup} warm-up steps, "
          f"paths alternating; device {torch.cuda.get_device_name(0)}, host {os.cpu_count()} CPUs visible, "
          f"torch threads {torch.get_num_threads()}", flush=True)
    out = {"hw": [h, w], "S": S, "steps": a.steps, "device": torch.cuda.get_device_name(0)}
    for k in paths:
        out[k] = summary({"host": "(a) host", "act": "(b) act"}[k], ms[k])
    if "host" in out:
        d = float(np.abs(last["host"] - last["act"]).max())
        out["act_over_host"] = round(out["act"]["median_ms"] / out["host"]["median_ms"], 4)
        out["last_step_max_abs_diff"] = d
        print(f"(b) / (a) = {out['act_over_host']:.4f}; last step: max |actions(a) - actions(b)| = {d:.3e} "
              "(PIL rounds between its passes: the two resizes differ by up to 1 code on smooth images, more on noise)",
              flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
