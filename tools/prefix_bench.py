"""What action-prefix conditioning costs: EvalAgent.act with and without a committed prefix, and a training
micro-batch with and without prefix lengths (profiles/prefix/prefix_bench.txt).

    python tools/prefix_bench.py [--steps 200] [--warmup 20] [--hw 480 640]     # inference
    python tools/prefix_bench.py --train [--micro-batch 64] [--steps 5]         # one training micro-batch

Inference: B = 1 at the real dims (config/train/bridge.yaml; synthetic weights), one uint8 frame, raw proprio and a
tokenised prompt per control step, as tools/obs_bench.py measures ``act``.  Three paths alternate step by step in one
process so that all see the same machine state:

  plain    EvalAgent.act without prev_actions: the graph without the option (what tools/obs_bench.py --only-act times)
  delay0   act(prev_actions=, delay=0) through the prefix-capable graph: the two extra launches outside the denoise
           loop (pz_action_normalize, pz_action_prefix_init), the prefix forms of the clamp and the denormalisation,
           and the prefix forms of pz_action_in / pz_action_out inside the loop; nothing committed
  delay2   the same graph with the first two actions committed

Each step is timed by the host clock from a device synchronise to the arrival of the actions in host memory; median,
minimum, maximum and the 5th / 95th percentiles of ``--steps`` steps are printed, then one JSON line.

Training (``--train``): forward + backward of one micro-batch at the real dims, without prefix lengths and with
d ~ U{0..3} per sample, alternating, device-synchronised wall time per call.
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


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def summary(name, ms):
    med = statistics.median(ms)
    s = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
         "p05_ms": round(pct(ms, 0.05), 4), "p95_ms": round(pct(ms, 0.95), 4)}
    print(f"{name:<10} median {med:9.3f} ms   min {s['min_ms']:9.3f}   p05 {s['p05_ms']:9.3f}   p95 {s['p95_ms']:9.3f}   "
          f"max {s['max_ms']:9.3f}   ({len(ms)} steps)", flush=True)
    return s


def synthetic_weights(model):
    import torch

    from pizero_native import ops

    ar = model._arena
    for i, name in enumerate(ar.order):  # U(+-1/sqrt(fan_in)); vectors zero (Gemma norm = identity)
        v = ar.view(name)
        if v.dim() >= 2:
            ops.fill_uniform(v, 1000 + i, 0.0, float(v.shape[-1]) ** -0.5)
        else:
            v.zero_()
    torch.cuda.synchronize()


def infer(a):
    import numpy as np
    import torch

    from src.agent.env_adapter.base import load_dataset_statistics
    from src.agent.eval import EvalAgent
    from src.agent.train import SyntheticBridgeDataset
    from src.utils.config import load_config

    cfg = load_config(os.path.join(ROOT, "open-pi-zero_amd", "config", "train", "bridge.yaml"),
                      {"env.adapter.dataset_statistics_path": a.stats})
    ag = EvalAgent(cfg, use_graph=True)
    synthetic_weights(ag.model)
    stats = load_dataset_statistics(a.stats)
    h, w = a.hw
    H, A = ag.model.horizon_steps, ag.model.action_dim
    b = next(iter(SyntheticBridgeDataset(cfg, 1, seed=1)))
    ids, am = b["input_ids"], b["attention_mask"]
    r = np.random.default_rng(0)
    n_frames = 8
    frames = [r.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n_frames)]
    lo, hi = np.array(stats["proprio"]["p01"]), np.array(stats["proprio"]["p99"])
    props = [(lo + (hi - lo) * r.uniform(0, 1, lo.shape)).astype(np.float32)[None, None] for _ in range(n_frames)]
    alo, ahi = np.array(stats["action"]["p01"]), np.array(stats["action"]["p99"])
    prevs = [torch.from_numpy((alo + (ahi - alo) * r.uniform(0, 1, (1, H, A))).astype(np.float32))
             for _ in range(n_frames)]
    noise = torch.randn(1, H, A, device=ag.device)
    paths = {
        "plain": lambda f, p, pv: ag.act(f[None], ids, am, p, noise=noise).cpu().numpy(),
        "delay0": lambda f, p, pv: ag.act(f[None], ids, am, p, noise=noise, prev_actions=pv, delay=0).cpu().numpy(),
        "delay2": lambda f, p, pv: ag.act(f[None], ids, am, p, noise=noise, prev_actions=pv, delay=2).cpu().numpy(),
    }
    ms = {k: [] for k in paths}
    last = {}
    for step in range(a.warmup + a.steps):
        i = step % n_frames
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn(frames[i], props[i], prevs[i])
            dt = (time.perf_counter() - t0) * 1e3
            if step >= a.warmup:
                ms[k].append(dt)
    print(f"act, B = 1, {h}x{w} uint8 frame, chunk {H}, {a.steps} timed steps per path after {a.warmup} warm-up steps, "
          f"paths alternating; device {torch.cuda.get_device_name(0)}", flush=True)
    out = {"mode": "infer", "hw": [h, w], "steps": a.steps, "device": torch.cuda.get_device_name(0)}
    for k in paths:
        out[k] = summary(k, ms[k])
    for k in ("delay0", "delay2"):
        out[f"{k}_over_plain"] = round(out[k]["median_ms"] / out["plain"]["median_ms"], 5)
    out["delay0_equals_plain_bitwise"] = bool(np.array_equal(last["plain"], last["delay0"]))
    out["delay2_prefix_rows_are_prev"] = bool(np.array_equal(last["delay2"][0, :2], prevs[(a.warmup + a.steps - 1)
                                                                                          % n_frames][0, :2].numpy()))
    print(f"delay0 / plain = {out['delay0_over_plain']:.5f}, delay2 / plain = {out['delay2_over_plain']:.5f}; last step: "
          f"delay0 == plain bit for bit: {out['delay0_equals_plain_bitwise']}, delay2's first two rows are the "
          f"caller's: {out['delay2_prefix_rows_are_prev']}", flush=True)
    print(json.dumps(out), flush=True)


def train(a):
    import torch

    from pizero_native import augment as A
    from src.agent.train import SyntheticBridgeDataset
    from src.model.vla.pizero import PiZero
    from src.utils.config import load_config

    cfg = load_config(os.path.join(ROOT, "open-pi-zero_amd", "config", "train", "bridge.yaml"), {})
    m = PiZero(cfg, device="cuda", dtype=torch.bfloat16, init="none")
    m.tie_action_proprio_weights()
    m.freeze_unused_weights()
    synthetic_weights(m)
    B = a.micro_batch
    b = next(iter(SyntheticBridgeDataset(cfg, B, seed=1)))
    mask, vpos, ppos, apos = m.build_causal_mask_and_position_ids(b["attention_mask"].cuda(), torch.bfloat16)
    pix = ((b["pixel_values"].cuda().float() / 255 - 0.5) / 0.5).to(torch.bfloat16)
    t = torch.rand(B, device="cuda") * 0.99
    x0 = torch.randn(B, m.horizon_steps, m.action_dim, device="cuda")
    base = dict(input_ids=b["input_ids"].cuda(), pixel_values=pix, causal_mask=mask, vlm_position_ids=vpos,
                proprio_position_ids=ppos, action_position_ids=apos, proprios=b["proprio"].cuda(),
                actions=b["action"].cuda(), t=t, noise=x0)
    pl = torch.from_numpy(A.draw_prefix_len(B, 3, 0, 0, 0)).to(torch.int32)
    paths = {"D=0": {}, "D=3": {"prefix_len": pl}}
    ms = {k: [] for k in paths}
    losses = {}
    for step in range(a.warmup + a.steps):
        for k, kw in paths.items():
            m.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = m(**base, **kw)
            loss.backward()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            losses[k] = loss.item()
            if step >= a.warmup:
                ms[k].append(dt)
    print(f"training micro-batch {B} (forward + backward), {a.steps} timed calls per path after {a.warmup} warm-up, "
          f"alternating; device {torch.cuda.get_device_name(0)}", flush=True)
    out = {"mode": "train", "micro_batch": B, "steps": a.steps, "loss": losses}
    for k in paths:
        out[k] = summary(k, ms[k])
    out["D3_over_D0"] = round(out["D=3"]["median_ms"] / out["D=0"]["median_ms"], 5)
    print(f"D=3 / D=0 = {out['D3_over_D0']:.5f}; losses {losses}", flush=True)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--hw", type=int, nargs=2, default=[480, 640])
    ap.add_argument("--stats", default=os.path.join(ROOT, "tests", "golden", "bridge_statistics.json"))
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--micro-batch", type=int, default=64)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("prefix_bench measures on the GPU: no device found")
    a.steps = a.steps if a.steps is not None else (5 if a.train else 200)
    a.warmup = a.warmup if a.warmup is not None else (1 if a.train else 20)
    return train(a) if a.train else infer(a)


if __name__ == "__main__":
    main()
