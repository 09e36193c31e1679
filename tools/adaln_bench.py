"""Timing / profiling driver of the adaLN and adaLN-Zero action expert at bridge dims (profiles/adaln/).

    python tools/adaln_bench.py --mode adaLN-Zero [--train-steps 3] [--chunks 50] [--micro-batch 64]

Prints one JSON line: ms per training step (forward + backward, micro-batch 64, synthetic fixture inputs) and ms
per hipGraph-replayed action chunk at B = 1 (``--mode none``: the default expert, i.e. config C4, on the same box).
Under ``rocprofv3 --kernel-trace --stats -- python tools/adaln_bench.py --train-steps 1 --chunks 1 --no-warmup``
the per-kernel summary holds one training step and one chunk.

    python tools/adaln_bench.py --kernels

times every pz_adaln.hip kernel ALONE (nothing else on the device, 200 back-to-back launches between two events) at the
training shape (micro-batch 64 x 5 expert rows x 1024) and the chunk shape (5 rows) and prints us per launch and the
achieved GB/s of the bytes the launch must move.
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


def build(d, mode):
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.model.vla.pizero import PiZero
    from tests.golden.make_golden import ref_cfg
    from tests.golden.make_golden_adaln import adaptive_cfg

    cfg = ref_cfg(d) if mode is None else adaptive_cfg(d, mode)
    m = PiZero(cfg, device="cuda", dtype=torch.bfloat16, init="none")
    m.tie_action_proprio_weights()
    m.freeze_unused_weights()
    for name in m._arena.order:
        v = m._arena.view(name)
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    torch.cuda.synchronize()
    return m


def time_kernels(iters=200):
    from pizero_native import ops

    D, rps = 1024, 5
    rows = []
    for B in (64, 1):
        R = B * rps
        bf = lambda *sh: torch.randn(*sh, device="cuda").to(torch.bfloat16)  # noqa: E731
        x, y, dh, out, out2 = bf(R, D), bf(R, D), bf(R, D), bf(R, D), bf(R, D)
        mod = torch.randn(B, 3 * D, device="cuda")
        dmod = torch.zeros_like(mod)
        rstd = torch.rand(R, device="cuda") + 0.5
        bz = bf(D)
        gate, gamma, beta = (0, bz), (D, bz), 2 * D
        row, mrow = 2 * R * D, 4 * B * D  # bytes of one bf16 [R, D] tensor / one fp32 [B, D] slot
        cases = {
            "adaln_fwd norm": (lambda: ops.adaln_fwd(x, mod, rps, 1e-6, gamma=gamma, beta=beta, h=out, rstd=rstd),
                               2 * row + 2 * mrow),
            "adaln_fwd gate": (lambda: ops.adaln_fwd(x, mod, rps, 1e-6, y=y, gate=gate, xm=out), 3 * row + mrow),
            "adaln_fwd gate+norm": (lambda: ops.adaln_fwd(x, mod, rps, 1e-6, y=y, gate=gate, xm=out, gamma=gamma,
                                                          beta=beta, h=out2, rstd=rstd), 4 * row + 3 * mrow),
            "adaln_norm_bwd": (lambda: ops.adaln_norm_bwd(dh, x, rstd, mod, gamma, out, dmod, beta, rps, dres=y),
                               4 * row + 3 * mrow),
            "adaln_gate_bwd": (lambda: ops.adaln_gate_bwd(dh, y, mod, gate, out, dmod, rps), 3 * row + 2 * mrow),
        }
        for name, (fn, nbytes) in cases.items():
            for _ in range(10):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / iters * 1e3
            rows.append({"kernel": name, "rows": R, "D": D, "us_per_launch": round(us, 2), "bytes": nbytes,
                         "GBps": round(nbytes / us / 1e3, 1)})
    for r in rows:
        print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="time each pz_adaln.hip kernel alone and exit")
    ap.add_argument("--mode", default="adaLN-Zero", choices=("none", "adaLN", "adaLN-Zero"))
    ap.add_argument("--train-steps", type=int, default=3)
    ap.add_argument("--chunks", type=int, default=50)
    ap.add_argument("--micro-batch", type=int, default=64)
    ap.add_argument("--no-warmup", action="store_true")
    a = ap.parse_args()
    if a.kernels:
        return time_kernels()
    from oracle import pizero_oracle as O
    from pizero_native.graph import InferenceGraph
    from tests.pizero_gpu_helpers import gpu_inputs, run_infer, run_loss

    d = O.FULL_DIMS
    mode = None if a.mode == "none" else a.mode
    m = build(d, mode)
    out = {"mode": a.mode, "micro_batch": a.micro_batch}
    if a.train_steps:
        gi = gpu_inputs(m, d, 16, repeat=a.micro_batch // 16)
        if not a.no_warmup:
            run_loss(m, gi)
        t0 = time.perf_counter()
        for _ in range(a.train_steps):
            loss = run_loss(m, gi)
        out["train_step_ms"] = (time.perf_counter() - t0) / a.train_steps * 1e3
        out["loss"] = float(loss)
        del gi
        m.zero_grad(set_to_none=True)
    if a.chunks:
        g1 = gpu_inputs(m, d, 2, select=[0])
        if a.no_warmup:
            run_infer(m, g1)
            torch.cuda.synchronize()
        else:
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
            out["chunk_ms_graph_b1"] = e0.elapsed_time(e1) / a.chunks
    print(json.dumps(out))


if __name__ == "__main__":
    main()
