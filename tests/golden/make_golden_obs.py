"""Golden fixture of the env adapter's normalisation, from the REFERENCE itself (build container only).

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_obs.py

The reference's ``src/agent/env_adapter/base.py`` (BaseEnvAdapter) is imported at run time by file path; nothing of it
is stored.  tests/golden/obs_norm.npz holds inputs and the reference methods' outputs only (fp64):

  proprio_raw   [64, 7]   raw proprio around the Bridge statistics' [p01, p99], a fifth of the range beyond each end
                          (so normalize_bound's clip is hit on both sides)
  action_norm   [64, 7]   normalised actions in [-1.25, 1.25]
  {bridge,synth}/normalize_bound, /denormalize_bound, /normalize_gaussian, /denormalize_gaussian
                          the four methods on those inputs with the Bridge statistics
                          (tests/golden/bridge_statistics.json, the reference's config/bridge_statistics.json) and with
                          a synthetic set (synth/lo, hi, mean, std: |values| <= 4, hi - lo >= 0.1), on synth/x, synth/a
"""

from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import REF  # noqa: E402


def _load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ad = _load("src/agent/env_adapter/base.py", "ref_env_adapter_base").BaseEnvAdapter()
    stats = json.load(open(os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")))
    r = np.random.default_rng(20250)
    res = {}
    p, a = stats["proprio"], stats["action"]
    lo, hi = np.array(p["p01"]), np.array(p["p99"])
    x = lo + (hi - lo) * r.uniform(-0.2, 1.2, (64, 7))
    y = r.uniform(-1.25, 1.25, (64, 7))
    res["proprio_raw"], res["action_norm"] = x, y
    res["bridge/normalize_bound"] = ad.normalize_bound(x, lo, hi)
    res["bridge/normalize_gaussian"] = ad.normalize_gaussian(x, np.array(p["mean"]), np.array(p["std"]))
    res["bridge/denormalize_bound"] = ad.denormalize_bound(y, np.array(a["p01"]), np.array(a["p99"]))
    res["bridge/denormalize_gaussian"] = ad.denormalize_gaussian(y, np.array(a["mean"]), np.array(a["std"]))
    slo = r.uniform(-4, 0, 7)
    shi = np.minimum(slo + r.uniform(0.1, 4, 7), 4.0)
    smean, sstd = r.uniform(-2, 2, 7), r.uniform(0.5, 2, 7)
    sx = slo + (shi - slo) * r.uniform(-0.2, 1.2, (64, 7))
    sx = np.clip(sx, -4, 4)
    res.update({"synth/lo": slo, "synth/hi": shi, "synth/mean": smean, "synth/std": sstd, "synth/x": sx, "synth/a": y})
    res["synth/normalize_bound"] = ad.normalize_bound(sx, slo, shi)
    res["synth/normalize_gaussian"] = ad.normalize_gaussian(sx, smean, sstd)
    res["synth/denormalize_bound"] = ad.denormalize_bound(y, slo, shi)
    res["synth/denormalize_gaussian"] = ad.denormalize_gaussian(y, smean, sstd)
    assert (np.abs(res["bridge/normalize_bound"]) == 1).any() and (np.abs(res["bridge/normalize_bound"]) < 1).any()
    path = os.path.join(ROOT, "tests", "golden", "obs_norm.npz")
    np.savez_compressed(path, **{k: np.asarray(v, np.float64) for k, v in res.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
