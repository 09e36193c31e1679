"""Timing driver of the 4-bit base weights (quantize: True); writes profiles/q4/q4_bench.txt.

    python tools/q4_bench.py [--reps 40] [--micro-batches 16,64] [--steps 5] [--out profiles/q4/q4_bench.txt]

1. pz_q4_dequant at the real sites (vlm gate|up 2 x 16384 x 2048 in one launch, q|k|v 2560 x 2048 in one launch, SigLIP
   fc1 4304 x 1152) against a device-to-device copy of the same bf16 output: the two alternate in one process over
   rotating destination buffers, medians of event times.  The copy moves 4 B per weight, the kernel 2.5 B + scales.
2. One LoRA training micro-batch (forward + backward, rank 32) at the bridge dims with and without quantize, the two
   models alternating in one process: median time, peak memory of a step above the resident weights, resident bytes of
   the weights, and the share of the micro-batch spent dequantising (every site's launch twice, timed by itself).
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

SITES = [("vlm gate|up", [16384 * 2048, 16384 * 2048]), ("vlm q|k|v", [2048 * 2048, 256 * 2048, 256 * 2048]),
         ("siglip fc1", [4304 * 1152])]


def _time(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def bench_sites(reps, qtype, say):
    from pizero_native.quant4 import Q4Store

    dev = "cuda"
    store = Q4Store(qtype, dev)
    for name, sizes in SITES:
        total = sum(sizes)
        names = []
        for i, n in enumerate(sizes):
            w = (torch.randn(n, device=dev) * 0.02).to(torch.bfloat16)
            store.quantize(f"{name}.{i}", w)
            names.append(f"{name}.{i}")
            del w
        nbuf = max(2, min(8, (1 << 30) // (2 * total)))  # rotate over ~1 GiB of destinations: no cache-resident output
        dsts = [torch.empty(total, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
        src = torch.empty(total, device=dev, dtype=torch.bfloat16).normal_()
        k = [0]

        def deq():
            k[0] += 1
            store.dequant(names, dsts[k[0] % nbuf])

        def copy():
            k[0] += 1
            dsts[k[0] % nbuf].copy_(src)

        for _ in range(3):
            deq(), copy()
        td, tc = [], []
        for _ in range(reps):  # alternate
            td += _time(deq, 1)
            tc += _time(copy, 1)
        md, mc = statistics.median(td), statistics.median(tc)
        moved = total * 2.5 + total / 64
        say(json.dumps({"site": name, "weights": total, "launches": 1, "dequant_us": round(md * 1e3, 1),
                        "copy_us": round(mc * 1e3, 1), "dequant_TBps": round(moved / md / 1e9, 3),
                        "copy_TBps": round(total * 4 / mc / 1e9, 3), "dequant_over_copy": round(md / mc, 3),
                        "min_dequant_us": round(min(td) * 1e3, 1), "min_copy_us": round(min(tc) * 1e3, 1)}))
        del dsts, src


def build(d, rank, quantize, qtype):
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.model.vla.pizero import PiZero
    from tests.golden.make_golden_lora import lora_cfg

    cfg = lora_cfg(d, rank)
    if quantize:
        cfg.vision.use_quantize = cfg.vision_projector.use_quantize = True
        for mixes in (cfg.mixture, cfg.joint.config.mixture):
            mixes["vlm"].use_quantize = True
        cfg.quantize_type = qtype
    m = PiZero(cfg, device="cuda", dtype=torch.bfloat16, init="none")
    m.tie_action_proprio_weights()
    m.freeze_unused_weights()
    m.freeze_non_lora_weights_in_vlm()
    for name in m._arena.order:
        v = m._arena.view(name)
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    m.quantize_base_()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return m


def micro_batch(m, gi):
    m.zero_grad(set_to_none=True)
    loss = m(input_ids=gi["input_ids"], pixel_values=gi["pixel_values"], causal_mask=gi["causal_mask"],
             vlm_position_ids=gi["vpos"], proprio_position_ids=gi["ppos"], action_position_ids=gi["apos"],
             proprios=gi["proprios"], actions=gi["actions32"], t=gi["t32"], noise=gi["x0"])
    loss.backward()
    return loss


def bench_train(mbs, steps, rank, qtype, say):
    from oracle import pizero_oracle as O
    from tests.pizero_gpu_helpers import gpu_inputs

    d = O.FULL_DIMS
    base0 = torch.cuda.memory_allocated()
    models = {}
    for q in (False, True):
        before = torch.cuda.memory_allocated()
        models[q] = build(d, rank, q, qtype)
        say(json.dumps({"model": "qlora" if q else "lora", "rank": rank,
                        "resident_weights_GB": round((torch.cuda.memory_allocated() - before) / 1e9, 3)}))
    mq = models[True]
    # the dequantisation work of one micro-batch by itself: every site twice (forward, input gradient)
    eng = mq._engine()
    sites = [[f"{pre}{pr}.weight" for pr in projs] for pre, projs in mq._vlm_linear_sites()]

    def all_sites():
        for _ in range(2):
            for s in sites:
                eng._q4_dequant(s[0], s[-1])

    all_sites()
    deq_ms = statistics.median(_time(all_sites, 5))
    for mb in mbs:
        gi = {q: gpu_inputs(m, d, 16, repeat=max(1, mb // 16)) for q, m in models.items()}
        times, peaks = {False: [], True: []}, {False: 0, True: 0}
        for q, m in models.items():  # warm-up (allocations, the scratch, the gradient arena)
            micro_batch(m, gi[q])
        torch.cuda.synchronize()
        for _ in range(steps):  # alternate
            for q, m in models.items():
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                times[q] += _time(lambda: micro_batch(m, gi[q]), 1)
                peaks[q] = max(peaks[q], torch.cuda.max_memory_allocated() - base)
        tl, tq = statistics.median(times[False]), statistics.median(times[True])
        say(json.dumps({"micro_batch": mb, "lora_ms": round(tl, 2), "qlora_ms": round(tq, 2),
                        "qlora_over_lora": round(tq / tl, 4), "dequant_ms_per_micro_batch": round(deq_ms, 3),
                        "dequant_share": round(deq_ms / tq, 4),
                        "step_peak_above_resident_GB": {"lora": round(peaks[False] / 1e9, 3),
                                                        "qlora": round(peaks[True] / 1e9, 3)},
                        "spread_ms": {"lora": [round(min(times[False]), 2), round(max(times[False]), 2)],
                                      "qlora": [round(min(times[True]), 2), round(max(times[True]), 2)]}}))
        del gi
    for q, m in models.items():
        g = m._arena.grad
        say(json.dumps({"model": "qlora" if q else "lora", "param_arena_GB": round(m._arena.data.numel() * 2 / 1e9, 3),
                        "grad_arena_GB": round((g.numel() if g is not None else 0) * 2 / 1e9, 3),
                        "packed_GB": round(m._q4.nbytes() / 1e9, 3) if q else 0.0,
                        "scratch_GB": round(m._engine()._q4_buf.numel() * 2 / 1e9, 3) if q else 0.0}))
    say(json.dumps({"total_allocated_GB_both_models": round((torch.cuda.memory_allocated() - base0) / 1e9, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--micro-batches", default="16,64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--quantize-type", default="fp4")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q4", "q4_bench.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        say(f"# tools/q4_bench.py on {torch.cuda.get_device_name(0)}: quantize_type {a.quantize_type}, medians of "
            f"{a.reps} alternating runs (sites) / {a.steps} alternating micro-batches (training, LoRA rank {a.rank})")
        bench_sites(a.reps, a.quantize_type, say)
        if not a.skip_train:
            bench_train([int(x) for x in a.micro_batches.split(",")], a.steps, a.rank, a.quantize_type, say)


if __name__ == "__main__":
    main()
