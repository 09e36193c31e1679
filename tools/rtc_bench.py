"""What inference-time guidance toward the previous chunk costs, and what the few-row input-gradient kernel
buys (profiles/rtc/rtc_bench.txt).

    python tools/rtc_bench.py [--steps 100] [--warmup 10] [--hw 480 640] [--reps 200] [--rounds 9] [--out FILE]

One process on one GPU, real dims (config/train/bridge.yaml, synthetic weights), B = 1.

  (a) act      EvalAgent.act per control step, three paths alternating step by step: without prev_actions, with a hard
               prefix (delay 2), and guided (delay 1, overlap 4, beta from the config).  Host clock from a device
               synchronise to the arrival of the actions in host memory; median / min / p05 / p95 / max.
  (b) chunk    the guided chunk as one graph replay (InferenceGraph.enable_guidance) captured twice on the same model:
               with ops.linear_dgrad_rows and with every input gradient forced onto ops.linear_dgrad; replays
               alternate, HIP-event time per replay.  The unguided graph's replay time is printed beside them.
  (c) kernels  each of the expert's four input-gradient shapes at M = 5 rows (the tied group of one sample) on both
               kernels: ``--reps`` launches back to back between two HIP events, over a ring of weight copies larger
               than the Infinity Cache (the loop's 18 layers of expert weights do not fit it either), the two kernels
               alternating for ``--rounds`` rounds; median time per launch and the achieved GB/s of the bytes the
               product needs (W once, dy, dx, the saved g|u where it applies).
  (d) chunk-50 the same shapes at M = 51 rows (one sample of the chunk-50 geometry): above the kernel's 16 rows, so
               ops.linear_dgrad_rows declines and the engine runs ops.linear_dgrad; its time is recorded.
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

SHAPES = [("down_proj", 1024, 4096, True), ("gate|up", 8192, 1024, False), ("o_proj", 1024, 2048, False),
          ("q|k|v", 2560, 1024, False)]  # name, N, K, DGEGLU epilogue
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def summary(name, ms):
    med = statistics.median(ms)
    s = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
         "p05_ms": round(pct(ms, 0.05), 4), "p95_ms": round(pct(ms, 0.95), 4)}
    say(f"{name:<12} median {med:9.3f} ms   min {s['min_ms']:9.3f}   p05 {s['p05_ms']:9.3f}   p95 {s['p95_ms']:9.3f}   "
        f"max {s['max_ms']:9.3f}   ({len(ms)} samples)")
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


def bench_act(a, ag, cfg, out):
    import numpy as np
    import torch

    from src.agent.env_adapter.base import load_dataset_statistics
    from src.agent.train import SyntheticBridgeDataset

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
        "hard d=2": lambda f, p, pv: ag.act(f[None], ids, am, p, noise=noise, prev_actions=pv, delay=2).cpu().numpy(),
        "guided 1/4": lambda f, p, pv: ag.act(f[None], ids, am, p, noise=noise, prev_actions=pv, delay=1,
                                              overlap=H).cpu().numpy(),
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
    say(f"(a) act, B = 1, {h}x{w} uint8 frame, chunk {H}, {a.steps} timed steps per path after {a.warmup} warm-up, "
        f"paths alternating")
    out["act"] = {k: summary(k, ms[k]) for k in paths}
    out["act"]["guided_over_plain"] = round(out["act"]["guided 1/4"]["median_ms"] / out["act"]["plain"]["median_ms"], 4)
    i = (a.warmup + a.steps - 1) % n_frames
    out["act"]["guided_row0_is_prev"] = bool(np.array_equal(last["guided 1/4"][0, :1], prevs[i][0, :1].numpy()))
    say(f"guided / plain = {out['act']['guided_over_plain']:.4f}; the guided chunk's row 0 is the caller's: "
        f"{out['act']['guided_row0_is_prev']}; finite: {bool(np.isfinite(last['guided 1/4']).all())}")


def bench_chunk(a, ag, out):
    import torch

    from pizero_native.graph import InferenceGraph
    from src.agent.chunking import guidance_coef, soft_mask

    m = ag.model
    eng = m._engine()
    H, A, steps = m.horizon_steps, m.action_dim, m.num_inference_steps
    g = torch.Generator("cuda").manual_seed(3)
    target = torch.rand(1, H, A, device="cuda", generator=g) * 2 - 1
    w = torch.from_numpy(soft_mask(H, 1, H))[None]
    coef = torch.from_numpy(guidance_coef(steps, 5.0))
    graphs = {}
    for name, rows in (("dgrad_rows", True), ("linear_dgrad", False), ("unguided", None)):
        ig = InferenceGraph(m, 1)
        ig.static["noise"].copy_(torch.randn(1, H, A, device="cuda", generator=g))
        if rows is not None:
            ig.enable_guidance()
            ig.static["guide_target"].copy_(target)
            ig.static["guide_w"].copy_(w)
            ig.static["guide_coef"].copy_(coef)
            eng.dgrad_rows = rows
        try:
            ig.capture()
        finally:
            eng.dgrad_rows = True
        graphs[name] = ig
    ms = {k: [] for k in graphs}
    res = {}
    for step in range(a.warmup + a.steps):
        for k, ig in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res[k] = ig.replay()
            e1.record()
            e1.synchronize()
            if step >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    say()
    say(f"(b) one chunk as one graph replay (zero image and prompt, B = 1), HIP events, {a.steps} replays per graph "
        f"after {a.warmup}, alternating")
    out["chunk"] = {k: summary(k, ms[k]) for k in graphs}
    d = (res["dgrad_rows"].float() - res["linear_dgrad"].float()).abs().max().item()
    out["chunk"]["rows_over_gemm"] = round(out["chunk"]["dgrad_rows"]["median_ms"] /
                                           out["chunk"]["linear_dgrad"]["median_ms"], 4)
    out["chunk"]["max_abs_diff"] = d
    say(f"dgrad_rows / linear_dgrad = {out['chunk']['rows_over_gemm']:.4f}; max |difference| of the two chunks {d:.3e}")


def bench_kernels(a, M, out, key, both=True):
    import torch

    from pizero_native import ops

    BF16 = torch.bfloat16
    res = {}
    for name, N, K, geglu in SHAPES:
        wbytes = N * K * 2
        copies = max(2, (640 << 20) // wbytes)
        g = torch.Generator("cuda").manual_seed(N + K)
        Ws = [(torch.randn(N, K, device="cuda", generator=g) * N ** -0.5).to(BF16) for _ in range(copies)]
        dy = torch.randn(M, N, device="cuda", generator=g).to(BF16)
        gu = torch.randn(M, 2 * K, device="cuda", generator=g).to(BF16) if geglu else None
        dx = torch.empty(M, 2 * K if geglu else K, device="cuda", dtype=BF16)
        kw = dict(epi=ops.PZ_EPI_DGEGLU, aux=gu) if geglu else {}
        need = wbytes + M * N * 2 + dx.numel() * 2 + (gu.numel() * 2 if geglu else 0)
        fns = {"linear_dgrad": lambda W: ops.linear_dgrad(dy, W, dx, **kw)}
        if both:
            fns["dgrad_rows"] = lambda W: ops.linear_dgrad_rows(dy, W, dx, **kw)
            assert ops.linear_dgrad_rows(dy, Ws[0], dx, **kw) is True
        else:
            assert ops.linear_dgrad_rows(dy, Ws[0], dx, **kw) is False
        us = {k: [] for k in fns}
        for rnd in range(a.rounds + 1):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.reps):
                    fn(Ws[i % copies])
                e1.record()
                e1.synchronize()
                if rnd:  # round 0 warms up
                    us[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        row = {"N": N, "K": K, "dgeglu": geglu, "bytes": need}
        for k in fns:
            t = statistics.median(us[k])
            row[k] = {"median_us": round(t, 3), "min_us": round(min(us[k]), 3), "max_us": round(max(us[k]), 3),
                      "GBps": round(need / t / 1e3, 1)}
        line = f"{name:<10} {N:>5} -> {K:<5}" + "".join(
            f"   {k} {row[k]['median_us']:8.2f} us (min {row[k]['min_us']:.2f}, max {row[k]['max_us']:.2f}) "
            f"{row[k]['GBps']:7.1f} GB/s" for k in fns)
        if both:
            row["speedup"] = round(row["linear_dgrad"]["median_us"] / row["dgrad_rows"]["median_us"], 3)
            line += f"   linear_dgrad / dgrad_rows = {row['speedup']:.2f}"
        say(line)
        res[name] = row
        del Ws
        torch.cuda.empty_cache()
    out[key] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--hw", type=int, nargs=2, default=[480, 640])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--stats", default=os.path.join(ROOT, "tests", "golden", "bridge_statistics.json"))
    ap.add_argument("--skip-model", action="store_true", help="kernels only: (c) and (d)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtc", "rtc_bench.txt"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rtc_bench measures on the GPU: no device found")
    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "reps": a.reps, "rounds": a.rounds}
    say(f"rtc_bench on {out['device']}")
    if not a.skip_model:
        from src.agent.eval import EvalAgent
        from src.utils.config import load_config

        cfg = load_config(os.path.join(ROOT, "open-pi-zero_amd", "config", "train", "bridge.yaml"),
                          {"env.adapter.dataset_statistics_path": a.stats})
        ag = EvalAgent(cfg, use_graph=True)
        synthetic_weights(ag.model)
        bench_act(a, ag, cfg, out)
        bench_chunk(a, ag, out)
        del ag
        torch.cuda.empty_cache()
    say()
    say(f"(c) input-gradient GEMMs at M = 5, {a.reps} launches per sample over a ring of weight copies (> 256 MiB), "
        f"{a.rounds} rounds, the two kernels alternating; GB/s of the bytes the product needs")
    bench_kernels(a, 5, out, "kernels_m5")
    say()
    say("(d) the same shapes at M = 51 (chunk 50, one sample): ops.linear_dgrad_rows declines, ops.linear_dgrad runs")
    bench_kernels(a, 51, out, "kernels_m51", both=False)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
