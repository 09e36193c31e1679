"""Timing / memory driver of several flow draws per observation (flow_samples_per_observation) at bridge
dims, synthetic batches, 64 observations (profiles/draws/).

    python tools/draws_bench.py [--draws 1,2,4,8,16] [--reps 10] [--rounds 2] [--parent-root ab_old]
                                [--out profiles/draws/draws_bench.txt] [--no-profile]

The driver itself never opens the GPU: every measurement is a child process of its own, one at a time.
  * timing: per round, a child on the parent commit's tree (``--parent-root``: a checkout of it with its library built,
    e.g. ``git archive HEAD^ | tar -x -C ab_old`` + its build_native.py) and a child on this tree, alternating.  A
    child builds the model, freezes the VLM as TrainAgent does (train_vlm: False) and times one micro-batch
    (zero_grad + forward + backward) with device events, 2 warm-up, ``--reps`` times per setting, then
    torch.cuda.max_memory_allocated of one micro-batch.  This tree: 64 observations with S draws each (S = 1: t of
    shape [B], today's step).  Parent: the replicated batch of 64 * S samples (every observation S times, sample
    b * S + s carrying draw s -- the same (t, x0), so the losses are comparable), for every S it holds; the first
    batch that runs out of memory ends the parent's list.
  * kernels: one ``rocprofv3 --kernel-trace --stats`` run of its own, one micro-batch of 64 observations x 8 draws; the
    rows of the new kernel instantiations are reported.
"""

from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS = 64


def _paths(root):
    for p in (root, os.path.join(root, "open-pi-zero_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _build(root):
    _paths(root)
    import torch
    from oracle import pizero_oracle as O
    from tests.pizero_gpu_helpers import build_gpu_model

    m = build_gpu_model(O.FULL_DIMS)
    for p in m.trainable_vlm_parameters:  # TrainAgent, train_vlm: False
        p.requires_grad = False
    assert not m._vlm_needs_grad()
    torch.cuda.synchronize()
    return m, O.FULL_DIMS


def _draws(gi, S):
    """t [64, S] and x0 [64, S, H, A] on the device: draw 0 the fixture's, the rest from a fixed generator"""
    import torch

    B, H, A = gi["actions32"].shape
    g = torch.Generator().manual_seed(1234)
    t = torch.rand(B, S, generator=g) * 0.96 + 0.02
    x0 = torch.randn(B, S, H, A, generator=g)
    t, x0 = t.cuda(), x0.cuda()
    t[:, 0], x0[:, 0] = gi["t32"], gi["x0"]
    return t, x0


def _micro_batch(m, gi, t, x0):
    m.zero_grad(set_to_none=True)
    loss = m(input_ids=gi["input_ids"], pixel_values=gi["pixel_values"], causal_mask=gi["causal_mask"],
             vlm_position_ids=gi["vpos"], proprio_position_ids=gi["ppos"], action_position_ids=gi["apos"],
             proprios=gi["proprios"], actions=gi["actions32"], t=t, noise=x0)
    loss.backward()
    return loss


def _measure(m, gi, t, x0, reps):
    import torch

    for _ in range(2):
        _micro_batch(m, gi, t, x0)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _micro_batch(m, gi, t, x0)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    loss = _micro_batch(m, gi, t, x0)
    torch.cuda.synchronize()
    return {"ms": [round(x, 3) for x in ms], "peak_GiB": round(torch.cuda.max_memory_allocated() / 2**30, 3),
            "loss": float(loss)}


def worker_time(a):
    import torch
    from tests.pizero_gpu_helpers import gpu_inputs

    m, d = _build(a.root)
    gi = gpu_inputs(m, d, 16, repeat=OBS // 16)
    for S in [int(x) for x in a.draws.split(",")]:
        t, x0 = _draws(gi, S)
        B, H, A = gi["actions32"].shape
        rec = {"label": a.label, "S": S}
        try:
            if a.label == "parent":  # the replicated batch of 64 * S samples through today's pass
                g = gi if S == 1 else {k: v.repeat_interleave(S, dim=0) for k, v in gi.items()}
                rec.update(_measure(m, g, t.reshape(B * S), x0.reshape(B * S, H, A), a.reps), samples=B * S)
                del g
            elif S == 1:
                rec.update(_measure(m, gi, t[:, 0].contiguous(), x0[:, 0].contiguous(), a.reps), samples=B)
            else:
                rec.update(_measure(m, gi, t, x0, a.reps), samples=B * S)
        except torch.cuda.OutOfMemoryError:
            rec["skipped"] = "out of memory"
        print(json.dumps(rec), flush=True)
        m.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
        if "skipped" in rec:
            break


def worker_profile(a):
    import torch
    from tests.pizero_gpu_helpers import gpu_inputs

    m, d = _build(a.root)
    gi = gpu_inputs(m, d, 16, repeat=OBS // 16)
    _micro_batch(m, gi, *_draws(gi, 8))
    torch.cuda.synchronize()


def _child(args, root, prefix=()):
    cmd = [*prefix, sys.executable, os.path.abspath(__file__), "--root", root, *args]
    # a child that fails or runs out of time ends the whole driver: nothing more is started on the device after it
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "draws", "draws_bench.txt"))
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--worker", choices=["time", "profile"], default=None)
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    if a.worker:
        _paths(os.path.abspath(a.root))
        return {"time": worker_time, "profile": worker_profile}[a.worker](a)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def say(line=""):  # every line goes to the screen and the file as soon as it exists
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("several flow draws per observation (flow_samples_per_observation = S, train_vlm: False), bridge dims, synthetic "
        "batches, one MI355X")
    say(f"one micro-batch = zero_grad + forward + backward on {OBS} observations; device events, 2 warm-up, {a.reps} reps "
        f"per round, {a.rounds} rounds, parent and this tree alternating")
    say(f"this tree: {OBS} observations x S draws.  parent commit: the replicated batch of {OBS} * S samples, same (t, x0)")
    say()
    runs = []
    common = ["--worker", "time", "--draws", a.draws, "--reps", str(a.reps)]
    for rnd in range(a.rounds):
        if a.parent_root:
            runs += _child([*common, "--label", "parent"], os.path.abspath(a.parent_root))
            print(f"(round {rnd + 1}: parent measured)", flush=True)
        runs += _child([*common, "--label", "this"], HERE)
        print(f"(round {rnd + 1}: this tree measured)", flush=True)
    med = {}
    for S in [int(x) for x in a.draws.split(",")]:
        say(f"S = {S} ({OBS * S} pairs)")
        for label, name in (("this", f"this tree, {OBS} observations x {S} draws"),
                            ("parent", f"parent commit, {OBS * S} samples (replicated)")):
            rs = [r for r in runs if r["label"] == label and r["S"] == S]
            if not rs:
                if label == "parent" and a.parent_root:
                    say(f"  {name:46s} not run: a smaller replicated batch already ran out of memory")
                continue
            if any("skipped" in r for r in rs):
                say(f"  {name:46s} not held: {rs[0].get('skipped') or 'out of memory'}")
                continue
            ms = [t for r in rs for t in r["ms"]]
            med[(label, S)] = statistics.median(ms)
            per = ", ".join(f"{statistics.median(r['ms']):.2f}" for r in rs)
            say(f"  {name:46s} {med[(label, S)]:9.2f} ms median of {len(ms)} (per round: {per}; min {min(ms):.2f}, max "
                f"{max(ms):.2f}); peak memory {max(r['peak_GiB'] for r in rs):.2f} GiB; loss {rs[0]['loss']:.6f}")
        if ("this", S) in med and ("parent", S) in med:
            say(f"  {S} draws vs the parent's replicated batch: {med[('parent', S)] / med[('this', S)]:.2f}x faster "
                f"({med[('parent', S)] - med[('this', S)]:.2f} ms less)")
        if ("this", S) in med and ("this", 1) in med and S > 1:
            say(f"  {S} draws vs 1 draw on this tree: {med[('this', S)] / med[('this', 1)]:.2f}x the time for {S}x the "
                f"supervision")
        say()
    if not a.no_profile:
        with tempfile.TemporaryDirectory() as tmp:
            _child(["--worker", "profile"], HERE, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format",
                                                          "csv", "-d", tmp, "-o", "draws", "--"])
            rows = []
            for f in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
                rows += list(csv.DictReader(open(f)))
        say(f"rocprofv3 --kernel-trace --stats, one run of its own: model build + ONE micro-batch of {OBS} observations x 8 "
            "draws (18 layers: 18 calls per kernel)")
        tot = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
        for r in rows:
            n = r["Name"]
            if "expert_attn" in n or "decode_attn" in n:
                say(f"  {n[:100]:100s} calls {r['Calls']:>4s}  total {float(r['TotalDurationNs']) / 1e3:9.1f} us  avg "
                    f"{float(r['AverageNs']) / 1e3:8.2f} us  {100 * float(r['TotalDurationNs']) / tot:5.2f} % of all kernel "
                    f"time in the run")
        say()
    out.close()


if __name__ == "__main__":
    main()
