"""Timing / memory driver of the frozen-VLM training pass (train_vlm: False) at bridge dims, synthetic
batches (profiles/frozen_vlm/).

    python tools/frozen_vlm_bench.py [--micro-batches 64,256] [--reps 20] [--rounds 2] [--parent-root ab_old]
                                     [--probe 512,1024] [--out profiles/frozen_vlm/frozen_vlm_bench.txt]

The driver itself never opens the GPU: every measurement is a child process of its own, one at a time.
  * timing: per round, a child on the parent commit's tree (``--parent-root``: a checkout of it with its library
    built, e.g. ``git archive HEAD^ | tar -x -C ab_old`` + its build_native.py) and a child on this tree, alternating.
    A child builds the model, freezes the VLM as TrainAgent does and times one micro-batch (zero_grad + forward +
    backward) with device events, warmed, ``--reps`` times per setting, the settings of ``Engine.vlm_forward_only``
    (False, True) alternating inside the loop; then torch.cuda.max_memory_allocated of one micro-batch per setting.
    The parent's tree has no such switch: its one figure is today's full pass.  Reported per micro-batch: the
    median over all rounds, and the spread of the parent's own repeated runs (its per-round medians and min / max).
  * ``--probe``: the largest of the given power-of-two micro-batches that the new pass holds (one micro-batch each,
    in order, stopping at the first out-of-memory error).
  * kernels: one ``rocprofv3 --kernel-trace --stats`` run of one micro-batch 64 of the new pass; the rows of the two
    new kernels (the decode_attn kernels instantiated with the log-sum-exp, expert_attn_bwd_*) are reported.
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


def _micro_batch(m, gi):
    m.zero_grad(set_to_none=True)
    loss = m(input_ids=gi["input_ids"], pixel_values=gi["pixel_values"], causal_mask=gi["causal_mask"],
             vlm_position_ids=gi["vpos"], proprio_position_ids=gi["ppos"], action_position_ids=gi["apos"],
             proprios=gi["proprios"], actions=gi["actions32"], t=gi["t32"], noise=gi["x0"])
    loss.backward()
    return loss


def worker_time(a):
    import torch
    from tests.pizero_gpu_helpers import gpu_inputs

    m, d = _build(a.root)
    eng = m._engine()
    settings = [s == "True" for s in a.settings.split(",")]
    for mb in [int(x) for x in a.micro_batches.split(",")]:
        gi = gpu_inputs(m, d, 16, repeat=mb // 16)
        live = []
        for s in settings:
            # the full pass keeps ~0.84 GB of activations per sample (13.3 GiB at 16, measured): leave it out where
            # it cannot fit rather than run into the allocator's limit
            torch.cuda.empty_cache()
            free, _ = torch.cuda.mem_get_info()
            if not s and free < mb * 0.95e9:
                print(json.dumps({"label": a.label, "mb": mb, "vlm_forward_only": s,
                                  "skipped": f"needs ~{mb * 0.95:.0f} GB, {free / 1e9:.0f} GB free"}), flush=True)
                continue
            live.append(s)
            eng.vlm_forward_only = s
            for _ in range(2):
                _micro_batch(m, gi)
        torch.cuda.synchronize()
        times = {s: [] for s in live}
        for _ in range(a.reps):
            for s in live:
                eng.vlm_forward_only = s
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss = _micro_batch(m, gi)
                e1.record()
                torch.cuda.synchronize()
                times[s].append(e0.elapsed_time(e1))
        for s in live:
            eng.vlm_forward_only = s
            m.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            loss = _micro_batch(m, gi)
            torch.cuda.synchronize()
            print(json.dumps({"label": a.label, "mb": mb, "vlm_forward_only": s, "ms": [round(t, 3) for t in times[s]],
                              "peak_GiB": round(torch.cuda.max_memory_allocated() / 2**30, 3),
                              "loss": float(loss)}), flush=True)
        del gi
        m.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()


def worker_probe(a):
    import torch
    from tests.pizero_gpu_helpers import gpu_inputs

    m, d = _build(a.root)
    held = None
    for mb in [int(x) for x in a.probe.split(",")]:
        try:
            gi = gpu_inputs(m, d, 16, repeat=mb // 16)
            torch.cuda.reset_peak_memory_stats()
            loss = _micro_batch(m, gi)
            torch.cuda.synchronize()
            held = mb
            print(json.dumps({"probe": mb, "held": True, "loss": float(loss),
                              "peak_GiB": round(torch.cuda.max_memory_allocated() / 2**30, 3)}), flush=True)
            del gi
            m.zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
        except torch.cuda.OutOfMemoryError:
            print(json.dumps({"probe": mb, "held": False, "why": "out of memory"}), flush=True)
            break
        except (ValueError, RuntimeError) as e:  # a size limit refused on the host, before any launch
            print(json.dumps({"probe": mb, "held": False, "why": str(e)[:200]}), flush=True)
            break
    print(json.dumps({"largest_probed_micro_batch_held": held}), flush=True)


def worker_profile(a):
    import torch
    from tests.pizero_gpu_helpers import gpu_inputs

    m, d = _build(a.root)
    gi = gpu_inputs(m, d, 16, repeat=4)
    _micro_batch(m, gi)
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
    ap.add_argument("--micro-batches", default="64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--probe", default="512,1024")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "frozen_vlm", "frozen_vlm_bench.txt"))
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--worker", choices=["time", "probe", "profile"], default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--settings", default="False,True")
    a = ap.parse_args()
    if a.worker:
        _paths(os.path.abspath(a.root))
        return {"time": worker_time, "probe": worker_probe, "profile": worker_profile}[a.worker](a)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    class _Lines:  # every line goes to the screen and the file as soon as it exists
        def append(self, line):
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        def __iadd__(self, ls):
            for line in ls:
                self.append(line)
            return self

    lines = _Lines()
    lines += ["frozen-VLM training pass (train_vlm: False), bridge dims, synthetic batches, one MI355X",
             f"one micro-batch = zero_grad + forward + backward; device events, 2 warm-up, {a.reps} reps per round, "
             f"{a.rounds} rounds, parent and this tree alternating, the two settings alternating inside a round", ""]
    runs = []
    common = ["--worker", "time", "--micro-batches", a.micro_batches, "--reps", str(a.reps)]
    for _ in range(a.rounds):
        if a.parent_root:
            runs += _child([*common, "--label", "parent", "--settings", "False"], os.path.abspath(a.parent_root))
        runs += _child([*common, "--label", "this", "--settings", "False,True"], HERE)
    for mb in [int(x) for x in a.micro_batches.split(",")]:
        lines.append(f"micro-batch {mb}")
        med = {}
        for label, s in (("parent", False), ("this", False), ("this", True)):
            rs = [r for r in runs if r["label"] == label and r["mb"] == mb and r["vlm_forward_only"] == s]
            name = "parent commit (full pass)" if label == "parent" else f"vlm_forward_only = {s}"
            if not rs:
                continue
            if "skipped" in rs[0]:
                lines.append(f"  {name:32s} not run: {rs[0]['skipped']}")
                continue
            ms = [t for r in rs for t in r["ms"]]
            med[(label, s)] = statistics.median(ms)
            per = ", ".join(f"{statistics.median(r['ms']):.2f}" for r in rs)
            lines.append(f"  {name:32s} {med[(label, s)]:9.2f} ms median of {len(ms)} (per round: {per}; min "
                         f"{min(ms):.2f}, max {max(ms):.2f}); peak memory {max(r['peak_GiB'] for r in rs):.2f} GiB; "
                         f"loss {rs[0]['loss']:.6f}")
        new = med.get(("this", True))
        for key, name in ((("parent", False), "parent"), (("this", False), "vlm_forward_only = False")):
            if new and key in med:
                lines.append(f"  new pass vs {name}: {med[key] / new:.2f}x faster ({med[key] - new:.2f} ms less)")
        lines.append("")
    if a.probe:
        pr = _child(["--worker", "probe", "--probe", a.probe], HERE)
        lines.append(f"largest power-of-two micro-batch of the new pass, probed over {a.probe} (one micro-batch each):")
        lines += ["  " + json.dumps(r) for r in pr]
        lines.append("")
    if not a.no_profile:
        with tempfile.TemporaryDirectory() as tmp:
            _child(["--worker", "profile"], HERE, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format",
                                                          "csv", "-d", tmp, "-o", "frozen", "--"])
            rows = []
            for f in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
                rows += list(csv.DictReader(open(f)))
        lines.append("rocprofv3 --kernel-trace --stats, one run of its own: model build + ONE micro-batch 64 of the new pass "
                     "(18 layers: 18 calls per kernel)")
        tot = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
        for r in rows:
            n = r["Name"]
            if "expert_attn" in n or ("decode_attn" in n and ("true" in n or "Lb1" in n)):
                lines.append(f"  {n[:90]:90s} calls {r['Calls']:>4s}  total {float(r['TotalDurationNs']) / 1e3:9.1f} us  "
                             f"avg {float(r['AverageNs']) / 1e3:8.2f} us  {100 * float(r['TotalDurationNs']) / tot:5.2f} % "
                             f"of all kernel time in the run")
        lines.append("")
    out.close()


if __name__ == "__main__":
    main()
