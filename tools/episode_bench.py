"""Cost of assembling training micro-batches from an episode store (profiles/episodes/).

    python tools/episode_bench.py [--batch 256] [--size 224] [--reps 50] [--warmup 5] [--agent-batch 64]
                                  [--skip-full] [--bench-branch FILE] [--bench-parent FILE] [--out FILE]

One process on one GPU; every number is a median of ``--reps`` micro-batches after ``--warmup``.  A counter-generated
store (tools/make_episode_store.py's episodes) of ``--size`` x ``--size`` frames is written to a temporary directory.
  (a) device    frames_placement: device -- HIP-event time of one micro-batch's assembly: the upload of the rows and
                both launches (ops.episode_gather_rows, ops.episode_gather_frames), and the host wall time of next()
  (b) host      frames_placement: host -- what its pieces cost on their own: the worker's gather of B frames from the
                memory maps into a pinned buffer (host wall), the H2D copy of that buffer and the transposing launch
                (HIP events)
  (c) numpy     the same micro-batch assembled on the host with numpy (fancy indexing, the NHWC -> NCHW copy, the
                normalisation of the gathered rows) and the upload it then needs (host wall, synchronised)
  (d) steps     TrainAgent's micro-batch step (next batch, preprocess_batch, forward, backward, clip, both optimizers;
                one micro-batch per update), synchronised after every step, with three sources alternating step by
                step on the SAME agent: pre-generated SyntheticBridgeDataset batches handed over from host memory
                (frames at the store's size), the store with ``device`` placement, and with ``host`` placement -- at
                the tiny model (``--batch``) and, unless ``--skip-full``, at the full model (``--agent-batch``)
``--bench-branch`` / ``--bench-parent``: files holding bench.py's JSON line on this tree and on its parent commit;
both lines are recorded and the losses compared.  The text goes to stdout and to ``--out``, then one JSON line.
"""

from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-pi-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def med(xs):
    return round(statistics.median(xs), 4)


def make_store(path, size, episodes, tmin, tmax, **tok):
    import numpy as np

    from src.data.episode_store import EpisodeStore, EpisodeStoreWriter, synthetic_episode

    lengths = np.random.Generator(np.random.Philox(key=0)).integers(tmin, tmax + 1, episodes)
    with EpisodeStoreWriter(path) as w:
        for e in range(episodes):
            w.add_episode(**synthetic_episode(e, int(lengths[e]), size, size, **tok))
    return EpisodeStore(path)


def numpy_batch(store, stats, rows, window, horizon):
    """the micro-batch on the host, vectorised numpy: what a host-side pipeline would do per micro-batch"""
    import numpy as np

    e = store.episode_of[rows]
    s, en = store.episode_offsets[e], store.episode_offsets[e + 1]
    act_rows = np.minimum(rows[:, None] + np.arange(horizon)[None], en[:, None] - 1)
    obs_rows = np.maximum(rows[:, None] - window + 1 + np.arange(window)[None], s[:, None])
    f = np.float32

    def bound(x, st, n_pass):
        k = x.shape[-1] - n_pass
        p, q = np.asarray(st["p01"], f)[:k], np.asarray(st["p99"], f)[:k]
        out = x.copy()
        out[..., :k] = np.clip(f(2) * (x[..., :k] - p) / (q - p + f(1e-8)) - f(1), -1, 1)
        return out

    ids = store.input_ids[e].astype(np.int64)
    frames = store.read_frames(rows)  # [B, C, H, W, 3]
    B, C, H, W, _ = frames.shape
    return {"action": bound(store.action[act_rows], stats["action"], 1),
            "proprio": bound(store.proprio[obs_rows], stats["proprio"], 0),
            "action_pad_mask": (rows[:, None] + np.arange(horizon)[None] <= en[:, None] - 1).astype(np.uint8),
            "input_ids": ids, "attention_mask": (ids != store.pad_token_id).astype(np.int64),
            "pixel_values": np.ascontiguousarray(frames.transpose(0, 1, 4, 2, 3)).reshape(B * C, 3, H, W)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--agent-batch", type=int, default=64)
    ap.add_argument("--skip-full", action="store_true")
    ap.add_argument("--bench-branch", default=None)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episodes", "episode_bench.txt"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from pizero_native import ops
    from pizero_native.episodes import EpisodeBatches, from_config
    from src.agent.train import SyntheticBridgeDataset, TrainAgent
    from src.utils.config import load_config
    from tests.golden.make_golden import ref_cfg
    from tests.oracle_helpers import O

    if not torch.cuda.is_available():
        raise SystemExit("episode_bench measures on the GPU: no device found")
    if a.reps < 50:
        print("note: fewer than 50 repetitions", flush=True)
    B, S, n_all = a.batch, a.size, a.warmup + a.reps
    tmp = tempfile.mkdtemp(prefix="episode_bench_")
    res = {"batch": B, "size": S, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "host_cpus_visible": os.cpu_count()}
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    t0 = time.perf_counter()
    full = make_store(os.path.join(tmp, "full"), S, 48, 20, 40)
    say(f"store: {full.num_episodes} episodes, {full.num_transitions} frames [1, {S}, {S}, 3] "
        f"({full.num_transitions * full.frame_bytes / 1e6:.0f} MB, {len(full.shards)} shards), written in "
        f"{time.perf_counter() - t0:.1f} s; micro-batch {B}; medians of {a.reps} after {a.warmup} on {res['device']}")

    def ev():
        return torch.cuda.Event(enable_timing=True)

    # ---- (a) device placement --------------------------------------------------------------------------------------
    eb = EpisodeBatches(full, B, 1, 4, "cuda", frames_placement="device")
    dev_ms, wall_ms = [], []
    for k in range(n_all):
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        t0 = time.perf_counter()
        e0.record()
        next(eb)
        e1.record()
        t1 = time.perf_counter()
        e1.synchronize()
        if k >= a.warmup:
            dev_ms.append(e0.elapsed_time(e1))
            wall_ms.append((t1 - t0) * 1e3)
    frame_bytes = B * full.frame_bytes
    res.update(device_assembly_ms=med(dev_ms), device_next_host_wall_ms=med(wall_ms))
    # the frames launch alone, rows already on the device
    local = torch.from_numpy(np.searchsorted(eb.sampler.rows, eb.sampler.batch(0))).cuda()
    out = torch.empty(B, 3, S, S, device="cuda", dtype=torch.uint8)
    k_ms = []
    for k in range(n_all):
        e0, e1 = ev(), ev()
        e0.record()
        ops.call("pz_episode_gather_frames", eb.frames.data_ptr(), eb.frames.shape[0], 1, S, S, local.data_ptr(), B,
                 out.data_ptr(), ops._st())
        e1.record()
        e1.synchronize()
        if k >= a.warmup:
            k_ms.append(e0.elapsed_time(e1))
    res.update(frames_kernel_ms=med(k_ms), frames_kernel_gbps=round(2 * frame_bytes / (med(k_ms) * 1e-3) / 1e9, 1))
    say(f"(a) device   rows upload + both launches (HIP events)        {res['device_assembly_ms']:9.4f} ms   "
        f"next() on the host {res['device_next_host_wall_ms']:.4f} ms (wall, not synchronised)")
    say(f"             pz_episode_gather_frames alone                  {res['frames_kernel_ms']:9.4f} ms   "
        f"{2 * frame_bytes / 1e6:.0f} MB read + written -> {res['frames_kernel_gbps']:.0f} GB/s")

    # ---- (b) host placement, piece by piece ------------------------------------------------------------------------
    pinned = torch.empty((B, *full.frame_shape), dtype=torch.uint8).pin_memory()
    staging = torch.empty((B, *full.frame_shape), device="cuda", dtype=torch.uint8)
    g_ms, c_ms, t_ms = [], [], []
    for k in range(n_all):
        rows = eb.sampler.batch(k)
        t0 = time.perf_counter()
        full.read_frames(rows, out=pinned.numpy())
        t1 = time.perf_counter()
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        staging.copy_(pinned, non_blocking=True)
        e1.record()
        ops.episode_gather_frames(staging, None, out=out)
        e2.record()
        e2.synchronize()
        if k >= a.warmup:
            g_ms.append((t1 - t0) * 1e3)
            c_ms.append(e0.elapsed_time(e1))
            t_ms.append(e1.elapsed_time(e2))
    res.update(host_gather_ms=med(g_ms), host_h2d_ms=med(c_ms), host_transpose_ms=med(t_ms),
               host_h2d_gbps=round(frame_bytes / (med(c_ms) * 1e-3) / 1e9, 1))
    say(f"(b) host     worker's gather, memory maps -> pinned (wall)    {res['host_gather_ms']:9.4f} ms   "
        f"(page cache warm: the store was just written)")
    say(f"             H2D copy of the pinned buffer (HIP events)       {res['host_h2d_ms']:9.4f} ms   "
        f"{frame_bytes / 1e6:.0f} MB -> {res['host_h2d_gbps']:.0f} GB/s")
    say(f"             transposing launch, identity rows                {res['host_transpose_ms']:9.4f} ms")

    # ---- (c) numpy on the host + upload ----------------------------------------------------------------------------
    n_ms, u_ms = [], []
    for k in range(n_all):
        rows = eb.sampler.batch(k)
        t0 = time.perf_counter()
        hb = numpy_batch(full, full.statistics, rows, 1, 4)
        t1 = time.perf_counter()
        up = {key: torch.from_numpy(v).cuda() for key, v in hb.items()}
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if k >= a.warmup:
            n_ms.append((t1 - t0) * 1e3)
            u_ms.append((t2 - t1) * 1e3)
    got = next(iter(EpisodeBatches(full, B, 1, 4, "cuda", frames_placement="device")))
    rows0 = eb.sampler.batch(0)
    hb0 = numpy_batch(full, full.statistics, rows0, 1, 4)
    res.update(numpy_host_ms=med(n_ms), numpy_upload_ms=med(u_ms),
               numpy_equals_device=all(bool((torch.from_numpy(hb0[key]).cuda() == got[key]).all()) for key in hb0))
    say(f"(c) numpy    the same micro-batch with numpy on the host      {res['numpy_host_ms']:9.4f} ms   "
        f"+ pageable upload {res['numpy_upload_ms']:.4f} ms (wall, synchronised); equal to (a): "
        f"{res['numpy_equals_device']}")
    del up, eb

    # ---- (d) TrainAgent steps ----------------------------------------------------------------------------------------
    from pizero_native.optim import clip_grad_norm_

    def agent_steps(label, cfg, store, mb):
        cfg_dev = copy.deepcopy(cfg)
        cfg_dev["data"] = {"train": {"episode_store": store.path, "frames_placement": "device"}}
        torch.manual_seed(0)
        ag = TrainAgent(cfg_dev)
        cfg_host = copy.deepcopy(cfg)
        cfg_host["data"] = {"train": {"episode_store": store.path, "frames_placement": "host"}}
        it = iter(SyntheticBridgeDataset(cfg, mb, seed=0))
        synth = []
        for i in range(4):  # handed over from host memory, frames at the store's size
            b = next(it)
            b["pixel_values"] = torch.randint(0, 256, (mb, 3, S, S), dtype=torch.uint8,
                                              generator=torch.Generator().manual_seed(i))
            synth.append(b)

        def cycle():
            i = 0
            while True:
                yield synth[i % len(synth)]
                i += 1

        host_batches = from_config(cfg_host, "train", mb, 0, 1, ag.device)
        sources = {"synthetic": cycle(), "store_device": iter(ag.train_dataloader), "store_host": iter(host_batches)}
        ms = {k: [] for k in sources}
        ag.model_meta.train()
        try:
            for rep in range(n_all):
                for name, src in sources.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    inputs = ag.preprocess_batch(next(src))
                    loss = ag.model_meta(**inputs)
                    loss.backward()
                    clip_grad_norm_(ag.optimizers, ag.max_grad_norm)
                    for opt in ag.optimizers:
                        opt.step()
                        opt.zero_grad(set_to_none=True)
                    torch.cuda.synchronize()
                    if rep >= a.warmup:
                        ms[name].append((time.perf_counter() - t0) * 1e3)
        finally:
            host_batches.close()
        r = {k: med(v) for k, v in ms.items()}
        r["spread_synthetic_min_max"] = [round(min(ms["synthetic"]), 4), round(max(ms["synthetic"]), 4)]
        res[f"steps_{label}"] = {"micro_batch": mb, **r}
        say(f"(d) {label:<6} micro-batch {mb:3d}: synthetic from host memory {r['synthetic']:9.3f} ms   store, device "
            f"{r['store_device']:9.3f} ms ({r['store_device'] - r['synthetic']:+.3f})   store, host "
            f"{r['store_host']:9.3f} ms ({r['store_host'] - r['synthetic']:+.3f})   [synthetic min "
            f"{r['spread_synthetic_min_max'][0]:.3f}, max {r['spread_synthetic_min_max'][1]:.3f}]")
        del ag, host_batches, sources
        torch.cuda.empty_cache()

    d = O.TINY_DIMS
    tiny_cfg = ref_cfg(d)
    common = dict(action_lr=1e-4, vlm_lr=1e-4, action_weight_decay=0.0, vlm_weight_decay=0.0, max_grad_norm=1.0,
                  n_updates=10 ** 9, log_freq=10 ** 9, train_vlm=True, use_bf16=True, flow_sampling="beta",
                  load_pretrained_weights=False,
                  action_lr_scheduler=dict(first_cycle_steps=10 ** 7, min_lr=1e-8, warmup_steps=2),
                  vlm_lr_scheduler=dict(first_cycle_steps=10 ** 7, min_lr=1e-8, warmup_steps=2))
    tiny_cfg.update(common, global_batch_size=B, per_device_batch_size=B)
    tiny_store = make_store(os.path.join(tmp, "tiny"), S, 48, 20, 40, token_len=d["max_seq_len"],
                            image_tokens=d["num_image_tokens"], image_token_index=d["image_token_index"],
                            vocab_size=d["vocab_size"])
    agent_steps("tiny", tiny_cfg, tiny_store, B)
    if not a.skip_full:
        os.environ.setdefault("VLA_LOG_DIR", tmp)
        os.environ.setdefault("TRANSFORMERS_CACHE", tmp)
        mb = a.agent_batch
        cfg = load_config(os.path.join(ROOT, "open-pi-zero_amd", "config", "train", "bridge.yaml"),
                          {"log_dir": "", "global_batch_size": mb, "per_device_batch_size": mb, "n_updates": 10 ** 9})
        agent_steps("full", cfg, full, mb)

    # ---- bench.py on this tree and on its parent -------------------------------------------------------------------
    lines_json = {}
    for label, path in (("branch", a.bench_branch), ("parent", a.bench_parent)):
        if path and os.path.exists(path):
            for ln in open(path).read().splitlines():
                if ln.startswith("{") and '"metric"' in ln:
                    lines_json[label] = ln
    if lines_json:
        say("bench.py --gpus 1 (the new path is not entered), one run each:")
        for label, ln in lines_json.items():
            j = json.loads(ln)
            say(f"  {label}: {j.get('value'):.2f} {j.get('unit')}  ms_per_step {j.get('ms_per_step'):.1f}  "
                f"loss_per_step {j.get('loss_per_step')}")
            say(f"  {label} line: {ln}")
        if len(lines_json) == 2:
            jb, jp = (json.loads(lines_json[k]) for k in ("branch", "parent"))
            res["bench_losses_bit_equal"] = (jb.get("loss_per_step") is not None and all(
                jb.get(k) == jp.get(k) for k in ("loss_per_step", "grad_norm_per_step")))
            say(f"  loss_per_step and grad_norm_per_step bit-equal: {res['bench_losses_bit_equal']}")
    say("command: python tools/episode_bench.py " + " ".join(sys.argv[1:]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)
    import shutil

    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
