"""Golden fixtures of weight averaging and the validation metric, from the REFERENCE itself (build container only).

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_averaging.py

The reference's ``src/agent/model_averaging.py`` (ModelAveraging over torch.optim.swa_utils.AveragedModel) and
``src/utils/metric.py`` (get_action_accuracy) are imported at run time by file path; nothing of them is stored.

tests/golden/averaging.npz: ModelAveraging driven on the CPU over a one-parameter bf16 module of N = 4,099 elements
for 12 scripted updates (update u = 1..12: the live weights become ``live[u - 1]``, then maybe_initialize(u) and
maybe_update(u), as train.py:387-393 calls them).  The live weights are a random walk (steps of mixed size, some
elements frozen, some exactly zero) so successive snapshots differ by anything from 0 to many ulps.
  live              [12, N] uint16   bf16 bit patterns of the live weights of each update
  ema/avg, swa/avg  [12, N] uint16   the averaged weights after each update (zeros before the start)
  ema/n, swa/n      [12]    int64    n_averaged after each update (-1 before the start: state_dict() is {})
  ema/cfg, swa/cfg                   the schedule: EMA start 3, freq 2 (does not divide the start), decay 0.99;
                                     SWA start 2, freq 3, swa_device cpu (the reference's default: torch's per-op
                                     bf16 path avg + (p - avg) / (n + 1), not the lerp)

tests/golden/action_accuracy.npz: three (gt, pred) pairs [5, 4, 7] fp32, the bridge thresholds, the reference
function's outputs [3, 5] fp32.  Pair 2 has errors exactly on the thresholds (strict <).
"""

from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import REF, AttrDict  # noqa: E402

N = 4099
UPDATES = 12
EMA = dict(use_ema=True, ema_start=3, ema_freq=2, ema_decay=0.99, ema_device="cpu")
SWA = dict(use_swa=True, swa_start=2, swa_freq=3, swa_device="cpu")
THRESHOLDS = [0.05, 0.1, 0.2, 0.3, 0.5]


def _load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def live_walk():
    g = torch.Generator().manual_seed(20241)
    w = torch.randn(N, generator=g) * torch.exp2(torch.randint(-6, 3, (N,), generator=g).float())
    w[::17] = 0.0
    moving = torch.rand(N, generator=g) > 0.1  # a tenth of the elements never move
    out = []
    for _ in range(UPDATES):
        step = torch.randn(N, generator=g) * torch.exp2(torch.randint(-12, -2, (N,), generator=g).float())
        w = torch.where(moving, w + step, w)
        out.append(w.to(torch.bfloat16))
        w = out[-1].float()
    return out


class One(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(N, dtype=torch.bfloat16))


def drive(MA, cfg, live):
    model = One()
    ma = MA(model, AttrDict(cfg), "cpu")
    avg = np.zeros((UPDATES, N), np.uint16)
    n = np.full(UPDATES, -1, np.int64)
    for u in range(1, UPDATES + 1):
        with torch.no_grad():
            model.w.copy_(live[u - 1])
        ma.maybe_initialize(u)
        ma.maybe_update(u)
        sd = ma.state_dict()
        if sd:
            avg[u - 1] = bits(sd["state_dict"]["w"])
            n[u - 1] = int(sd["n_averaged"])
    return avg, n


def make_averaging():
    MA = _load("src/agent/model_averaging.py", "ref_model_averaging").ModelAveraging
    live = live_walk()
    res = {"live": np.stack([bits(x) for x in live])}
    for tag, cfg in (("ema", EMA), ("swa", SWA)):
        res[f"{tag}/avg"], res[f"{tag}/n"] = drive(MA, cfg, live)
        res[f"{tag}/cfg"] = np.array([f"{k}={v}" for k, v in cfg.items()])
        print(tag, "n_averaged", res[f"{tag}/n"].tolist())
    path = os.path.join(ROOT, "tests", "golden", "averaging.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


def make_accuracy():
    fn = _load("src/utils/metric.py", "ref_metric").get_action_accuracy
    g = torch.Generator().manual_seed(7)
    res = {"thresholds": np.array(THRESHOLDS, np.float64)}
    outs = []
    for i in range(3):
        gt = torch.rand(5, 4, 7, generator=g) * 2 - 1
        # per-row error scales from far below the smallest threshold to above the largest
        scale = torch.exp2(torch.randint(-7, 1, (5, 4, 1), generator=g).float())
        pred = gt + (torch.rand(5, 4, 7, generator=g) * 2 - 1) * scale
        if i == 2:  # errors exactly on a threshold: gt 0, pred = the float32 threshold
            gt[0] = 0.0
            pred[0] = 0.0
            for j, thr in enumerate(THRESHOLDS[:4]):
                pred[0, j, j] = thr
        res[f"gt{i}"], res[f"pred{i}"] = gt.numpy(), pred.numpy()
        outs.append(fn(gt, pred, THRESHOLDS).numpy())
    res["accuracy"] = np.stack(outs).astype(np.float32)
    print("accuracy", res["accuracy"])
    path = os.path.join(ROOT, "tests", "golden", "action_accuracy.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make_averaging()
    make_accuracy()
