"""Timing / profiling driver of LoRA fine-tuning at bridge dims (profiles/lora/).

    python tools/lora_bench.py [--ranks 0,32,64] [--steps 2] [--micro-batch 256] [--accum 4] [--chunks 50]

For each rank (0 = full fine-tuning, the bench.py workload) prints one JSON line: samples/s and ms of a training step
at the bench shape (micro-batch 256 x 4 accumulations: forward + backward, gradient clipping, 8-bit AdamW on the
action expert and on the trained VLM parameters -- every VLM weight, or the adapters alone), the loss per step, and,
for a LoRA model, the time of one merged-weight refresh and the hipGraph-replayed action chunk at B = 1 (config C4: the
same kernels on merged weights).  Under ``rocprofv3 --kernel-trace --stats -- python tools/lora_bench.py --ranks 32
--steps 1 --no-warmup --chunks 0`` the per-kernel summary holds one LoRA step: the adapter GEMMs (N or K of 32..192),
lora_wgrad_kernel / lora_wgrad_reduce_kernel and the rank-extended gemm8p_x_kernel launches.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-pi-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def build(d, rank):
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.model.vla.pizero import PiZero
    from tests.golden.make_golden import ref_cfg
    from tests.golden.make_golden_lora import lora_cfg

    m = PiZero(lora_cfg(d, rank) if rank else ref_cfg(d), device="cuda", dtype=torch.bfloat16, init="none")
    m.tie_action_proprio_weights()
    m.freeze_unused_weights()
    if rank:
        m.freeze_non_lora_weights_in_vlm()
    for name in m._arena.order:
        v = m._arena.view(name)
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    torch.cuda.synchronize()
    return m


def train_step(m, gi, opts, accum):
    from pizero_native.optim import clip_grad_norm_

    m.zero_grad(set_to_none=True)
    total = 0.0
    for _ in range(accum):
        loss = m(input_ids=gi["input_ids"], pixel_values=gi["pixel_values"], causal_mask=gi["causal_mask"],
                 vlm_position_ids=gi["vpos"], proprio_position_ids=gi["ppos"], action_position_ids=gi["apos"],
                 proprios=gi["proprios"], actions=gi["actions32"], t=gi["t32"], noise=gi["x0"]) / accum
        loss.backward()
        total = total + loss.detach()
    clip_grad_norm_(opts, 1.0)
    for o in opts:
        o.step()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="0,32,64")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--micro-batch", type=int, default=256)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--chunks", type=int, default=50)
    ap.add_argument("--no-warmup", action="store_true")
    a = ap.parse_args()
    from oracle import pizero_oracle as O
    from pizero_native.graph import InferenceGraph
    from pizero_native.optim import FusedAdamW
    from tests.pizero_gpu_helpers import gpu_inputs

    d = O.FULL_DIMS
    for rank in [int(r) for r in a.ranks.split(",")]:
        m = build(d, rank)
        out = {"lora_r": rank, "micro_batch": a.micro_batch, "accum": a.accum}
        vlm = m.lora_trainable_vlm_parameters if rank else m.trainable_vlm_parameters
        out["trained_vlm_params_B"] = round(sum(p.numel() for p in vlm) / 1e9, 4)
        opts = [FusedAdamW(m.action_expert_parameters, lr=5e-5, state_bits=8), FusedAdamW(vlm, lr=5e-5, state_bits=8)]
        gi = gpu_inputs(m, d, 16, repeat=a.micro_batch // 16)
        if not a.no_warmup:
            train_step(m, gi, opts, a.accum)
        torch.cuda.synchronize()
        losses = []
        t0 = time.perf_counter()
        for _ in range(a.steps):
            losses.append(train_step(m, gi, opts, a.accum))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / max(1, a.steps)
        out["step_ms"] = round(dt * 1e3, 1)
        out["samples_per_s"] = round(a.micro_batch * a.accum / dt, 2)
        out["loss_per_step"] = [float(x) for x in losses]
        del gi, opts
        m.zero_grad(set_to_none=True)
        m._arena.grad = None
        torch.cuda.empty_cache()
        if a.chunks:
            eng = m._engine()
            if rank:
                eng.lora_refresh()
                torch.cuda.synchronize()
                eng._merged_ver = None  # time one full rebuild
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.lora_refresh()
                e1.record()
                torch.cuda.synchronize()
                out["merge_refresh_ms"] = round(e0.elapsed_time(e1), 3)
            g1 = gpu_inputs(m, d, 2, select=[0])
            ig = InferenceGraph(m, 1, clip=True)
            ig.load(g1["input_ids"], g1["pixel_values"], m.block_prefix_counts(g1["itp"], g1["amask"]), g1["vpos"],
                    g1["ppos"], g1["apos"], g1["proprios"].float(), g1["noise"])
            ig.capture()
            ig.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.chunks):
                ig.replay()
            e1.record()
            torch.cuda.synchronize()
            out["chunk_ms_graph_b1"] = round(e0.elapsed_time(e1) / a.chunks, 3)
            del ig
        print(json.dumps(out), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
