"""Weight averaging (EMA / SWA) and in-training evaluation: the parts that need no GPU.

ABI surface of pz_avg_lerp / pz_avg_swap and their host-side argument checks (which fail before any launch),
get_action_accuracy against the reference function's recorded outputs (tests/golden/action_accuracy.npz, written by
tests/golden/make_golden_averaging.py), ModelAveraging's constructor contract and the new bridge.yaml keys.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

from tests.conftest import PKG, ROOT
from tests.oracle_helpers import load_golden

NEW = ("pz_avg_lerp", "pz_avg_swap")


def test_abi_declares_exports_and_binds_the_entry_points():
    import pizero_native
    from pizero_native._lib import ABI_VERSION, SIGNATURES
    from tests.test_abi import declared_symbols

    syms = declared_symbols()
    L = pizero_native.lib()
    for s in NEW:
        assert s in syms, f"{s} not declared in include/pz_abi.h"
        assert hasattr(L, s), f"{s} not exported"
        assert s in SIGNATURES, f"{s} has no ctypes signature"
    i64, f32, vp = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert SIGNATURES["pz_avg_lerp"] == [vp, vp, i64, f32, vp]
    assert SIGNATURES["pz_avg_swap"] == [vp, vp, i64, vp]
    assert ABI_VERSION == 22 and L.pz_abi_version() == 22  # entry points added, no signature changed
    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    assert "#define PZ_ABI_VERSION 22" in hdr


def test_ops_wrappers_exist():
    from pizero_native import ops

    assert callable(ops.avg_lerp) and callable(ops.avg_swap)


def _bad_args():
    """(label, a, b, n): host memory is enough, the checks return before anything is launched or dereferenced"""
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    a, b = base, base + 2048
    return [("null a", None, b, 64), ("null b", a, None, 64), ("n = 0", a, b, 0), ("n < 0", a, b, -8),
            ("a off by 2 bytes", a + 2, b, 64), ("b off by 2 bytes", a, b + 2, 64),
            ("overlap: same", a, a, 64), ("overlap: b inside a", a, a + 64, 64), ("overlap: a inside b", a + 64, a, 64),
            ("overlap: last 16 bytes", a, a + 2048 - 16, 1024)], buf


@pytest.mark.parametrize("fn", NEW)
def test_error_path_without_gpu(fn):
    import pizero_native

    L = pizero_native.lib()
    cases, keep = _bad_args()
    for label, a, b, n in cases:
        args = (a, b, n, 0.25, None) if fn == "pz_avg_lerp" else (a, b, n, None)
        assert getattr(L, fn)(*args) == 1, f"{fn}: {label} was not refused"
        assert L.pz_last_error().startswith(fn[3:].encode()), (label, L.pz_last_error())
    del keep


def test_action_accuracy_matches_reference_outputs():
    from src.utils.metric import get_action_accuracy

    g = load_golden("action_accuracy")
    thr = [float(x) for x in g["thresholds"]]
    assert thr == [0.05, 0.1, 0.2, 0.3, 0.5]
    for i in range(3):
        gt, pred = torch.from_numpy(g[f"gt{i}"]), torch.from_numpy(g[f"pred{i}"])
        assert gt.shape == (5, 4, 7)
        out = get_action_accuracy(gt, pred, thr)
        assert out.dtype == torch.float32 and out.shape == (5,)
        assert np.array_equal(out.numpy(), g["accuracy"][i]), (i, out, g["accuracy"][i])
    # the fixture discriminates: not all 0 / all 1, and monotone in the threshold
    assert 0 < g["accuracy"].min() and g["accuracy"].max() < 1
    assert (np.diff(g["accuracy"], axis=1) >= 0).all()


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(8))


def test_model_averaging_constructor_contract():
    """both switches -> AssertionError; nothing is allocated before the start, so a CPU stub model is enough"""
    from src.agent.model_averaging import ModelAveraging

    with pytest.raises(AssertionError):
        ModelAveraging(_Stub(), dict(use_ema=True, use_swa=True, ema_start=0, swa_start=0, swa_freq=1), "cpu")
    m = _Stub()
    off = ModelAveraging(m, {}, "cpu")
    assert not off.use_ema and not off.use_swa and off.state_dict() == {} and off.get_model_module() is m
    off.maybe_initialize(0)
    off.maybe_update(0)
    assert off.model_avg is None
    with off.averaged_weights() as mm:  # a no-op before the start
        assert mm is m
    ema = ModelAveraging(m, dict(use_ema=True, ema_start=5), "cpu")
    assert (ema.ema_start, ema.ema_decay, ema.ema_freq) == (5, 0.99, 1)
    assert ema.model_avg is None and ema.state_dict() == {} and ema.get_model_module() is m
    ema.maybe_update(3)  # before the start: nothing happens (and nothing touches a GPU)
    assert ema.model_avg is None
    swa = ModelAveraging(m, dict(use_swa=True, swa_start=4, swa_freq=2), "cuda:0")  # swa_device defaults to cpu
    assert (swa.swa_start, swa.swa_freq) == (4, 2) and swa.model_avg is None
    with pytest.raises(KeyError):
        ModelAveraging(m, dict(use_swa=True), "cpu")  # swa_start / swa_freq have no default (as in the reference)


def test_train_agent_signature():
    import inspect

    from src.agent.train import TrainAgent

    assert list(inspect.signature(TrainAgent.__init__).parameters) == ["self", "cfg", "dataset", "val_dataset"]
    assert callable(TrainAgent.evaluate)


def test_bridge_config_resolves_averaging_and_eval_keys():
    from src.utils.config import load_config

    c = load_config(os.path.join(PKG, "config", "train", "bridge.yaml"))
    assert c.use_ema is False and c.use_swa is False
    assert c.save_model_start == 0 and c.ema_start == c.save_model_start
    assert c.ema_decay == 0.99 and c.ema_freq == 1 and c.ema_device == "cuda" and c.swa_device == "cpu"
    assert c.swa_start == 1550000 // 1024 * 5 and c.swa_freq == 1550000 // 1024 // 4
    assert c.eval_freq == 2000 and c.eval_size == 1024
    assert c.eval_thresholds == [0.05, 0.1, 0.2, 0.3, 0.5] and len(c.eval_thresholds) == 5
    c2 = load_config(os.path.join(PKG, "config", "train", "bridge.yaml"), {"save_model_start": 7})
    assert c2.ema_start == 7
