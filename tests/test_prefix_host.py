"""Action-prefix conditioning, the parts that need no GPU: the restatement against the oracle, the
host-side delay draws and the count a resume restores for them, the chunk-scheduling helper, the numpy normalisation twin and the refusals."""

import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.golden.make_golden import ref_cfg
from tests.oracle_helpers import O, oracle_run
from tests.prefix_ref import restatement_run


def test_restatement_without_a_prefix_is_the_oracle_bit_for_bit():
    d = O.TINY_DIMS
    want, _ = oracle_run(d, 3, True, want_grads=False)
    got, _ = restatement_run(d, 3, [0, 0, 0], want_grads=False)
    assert got["loss"] == want["loss"], (got["loss"], want["loss"])
    assert torch.equal(got["actions"], want["actions"])


def test_restatement_with_a_prefix():
    """the masked loss differs from the plain one; prefix rows of the chunk are the prefix, whatever its values (no
    clamp on them), and the d = 0 sample's chunk is the oracle's"""
    d = O.TINY_DIMS
    plain, inp = oracle_run(d, 3, True, want_grads=False)
    pf = np.array(inp["actions"], copy=True)
    pf[1, 0, :] = 1.5
    pf[2, :3, 2] = -1.5
    got, _ = restatement_run(d, 3, [0, 1, 3], prefix=pf, want_grads=False, clip=True)
    assert abs(got["loss"] - plain["loss"]) > 0.05 * plain["loss"]
    a = got["actions"].numpy()
    assert np.array_equal(a[1, :1], pf[1, :1]) and np.array_equal(a[2, :3], pf[2, :3])
    assert np.abs(a[1, 1:]).max() <= 1.0 and np.abs(a[2, 3:]).max() <= 1.0 and np.abs(a[0]).max() <= 1.0
    assert np.array_equal(a[0], np.clip(plain["actions"][0].numpy(), -1.0, 1.0))
    assert not np.array_equal(a[1, 1:], np.clip(plain["actions"][1, 1:].numpy(), -1.0, 1.0))


# ------------------------------------------------------------------------------------------------ the delay draws --
def test_draws_are_deterministic_in_range_and_keyed_on_seed_batch_and_rank():
    from pizero_native import augment as A

    D = 3
    a = A.draw_prefix_len(64, D, seed=42, cnt_batch=5, rank=0)
    assert a.shape == (64,) and a.dtype.kind == "i" and a.min() >= 0 and a.max() <= D
    assert set(a.tolist()) == set(range(D + 1))  # 64 draws of U{0..3}: every value appears
    assert np.array_equal(a, A.draw_prefix_len(64, D, seed=42, cnt_batch=5, rank=0))
    for other in (dict(seed=43, cnt_batch=5, rank=0), dict(seed=42, cnt_batch=6, rank=0),
                  dict(seed=42, cnt_batch=5, rank=1)):
        assert not np.array_equal(a, A.draw_prefix_len(64, D, **other)), other
    # a sample's draw does not depend on the batch size, D = 0 draws zeros, D = H - 1 stays below H
    assert np.array_equal(a[:8], A.draw_prefix_len(8, D, seed=42, cnt_batch=5, rank=0))
    assert not A.draw_prefix_len(16, 0, 1, 2, 3).any()
    assert A.draw_prefix_len(4096, 49, 0, 0).max() == 49
    with pytest.raises(ValueError, match="max_delay"):
        A.draw_prefix_len(4, -1, 0, 0)


def test_draws_leave_the_augmentation_stream_and_torch_alone():
    """a stream constant of their own: the image augmentation draws of the same (seed, cnt_batch, rank) are what they
    were, the delays are not a function of them, and neither torch's nor numpy's global generator is consumed"""
    from pizero_native import augment as A

    u_before = A.generator(7, 3, 1).random(8)
    st, ns = torch.get_rng_state(), np.random.get_state()[1].copy()
    d = A.draw_prefix_len(8, 3, seed=7, cnt_batch=3, rank=1)
    assert torch.equal(torch.get_rng_state(), st) and np.array_equal(np.random.get_state()[1], ns)
    assert np.array_equal(A.generator(7, 3, 1).random(8), u_before)
    assert np.array_equal(A.generator(7, 3, 1, stream=0).random(8), u_before)
    same_stream = A.generator(7, 3, 1).integers(0, 4, size=8)
    assert not np.array_equal(d, same_stream)
    p0, m0 = A.draw_params(A.REFERENCE_PRIMARY, 4, seed=7, cnt_batch=3, rank=1)
    A.draw_prefix_len(4, 3, seed=7, cnt_batch=3, rank=1)
    p1, m1 = A.draw_params(A.REFERENCE_PRIMARY, 4, seed=7, cnt_batch=3, rank=1)
    assert np.array_equal(p0, p1) and np.array_equal(m0, m1)


def test_load_checkpoint_restores_the_count_the_draws_are_keyed_on(tmp_path):
    """a checkpoint stores the index of its last micro-batch; load_checkpoint restores the number of micro-batches
    consumed (that index + 1), so the first resumed micro-batch draws what the uninterrupted run draws next and not the
    last draw again"""
    from pizero_native import augment as A
    from src.agent import train as T

    class Stub:
        def load_state_dict(self, sd, strict=True):
            pass

    path = tmp_path / "step.pt"
    torch.save({"cnt_update": 2, "cnt_batch": 3, "model": {}, "wandb_id": None}, path)
    a = T.TrainAgent.__new__(T.TrainAgent)
    a.cfg, a.model, a._averaging_enabled = ref_cfg(O.TINY_DIMS), Stub(), False
    a.action_prefix_max_delay, a.action_prefix_seed, a.rank = 3, 11, 0
    a.load_checkpoint(str(path))
    assert (a.cnt_update, a.cnt_batch, a.micro_batches_seen) == (2, 3, 4)
    ids = torch.zeros(16, 2, dtype=torch.int64)
    got = a._prefix_len({"input_ids": ids}).numpy()
    assert np.array_equal(got, A.draw_prefix_len(16, 3, 11, 4, 0))
    assert not np.array_equal(got, A.draw_prefix_len(16, 3, 11, 3, 0))


# ------------------------------------------------------------------------------------------- the chunk scheduler --
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_next_prefix(kind):
    from src.agent.chunking import next_prefix

    H, A = 6, 3
    prev = np.arange(H * A, dtype=np.float32).reshape(H, A) + 1
    if kind == "torch":
        prev = torch.from_numpy(prev)
    eq = (lambda a, b: torch.equal(a, b)) if kind == "torch" else np.array_equal
    p, d = next_prefix(prev, offset=2, delay=3)
    assert d == 3 and p.shape == prev.shape and eq(p[:3], prev[2:5]) and not p[3:].any()
    p, d = next_prefix(prev, offset=4, delay=3)  # offset + delay > H: only what is left of the previous chunk
    assert d == 2 and eq(p[:2], prev[4:6]) and not p[2:].any()
    p, d = next_prefix(prev, offset=6, delay=2)  # the previous chunk is used up
    assert d == 0 and not p.any()
    p, d = next_prefix(prev, offset=9, delay=2)
    assert d == 0 and not p.any()
    p, d = next_prefix(prev, offset=1, delay=0)
    assert d == 0 and not p.any()
    p, d = next_prefix(prev, offset=0, delay=5)
    assert d == 5 and eq(p[:5], prev[:5])
    assert type(p) is type(prev)
    with pytest.raises(ValueError, match="non-negative"):
        next_prefix(prev, -1, 2)
    with pytest.raises(ValueError, match=r"\[H, A\]"):
        next_prefix(prev[None], 0, 1)


# ------------------------------------------------------------------------------------------ normalisation twin --
@pytest.mark.parametrize("kind", ["bound", "gaussian"])
def test_normalize_action_inverts_denormalize_action(kind):
    import json

    from src.agent.env_adapter.base import BaseEnvAdapter

    stats = json.load(open(os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")))
    ad = BaseEnvAdapter()
    rng = np.random.default_rng(0)
    x = rng.uniform(-1.0, 1.0, size=(5, 4, 7))  # in range: the bound form's clip does not act
    x[..., -1] = rng.uniform(-3.0, 3.0, size=(5, 4))  # the gripper passes through both ways, whatever its value
    raw = ad.denormalize_action(x, stats, kind)
    back = ad.normalize_action(raw, stats, kind)
    assert back.shape == x.shape
    np.testing.assert_allclose(back[..., :-1], x[..., :-1], rtol=0, atol=1e-6)  # fp64; p99 - p01 ~ 0.05: eps 1e-8 / span
    assert np.array_equal(back[..., -1], x[..., -1]) and np.array_equal(raw[..., -1], x[..., -1])
    if kind == "bound":  # robot units outside [p01, p99] clip to [-1, 1]
        far = np.array(stats["action"]["p99"])[None, :] * 0 + 1e3
        out = ad.normalize_action(far, stats, "bound")
        assert np.array_equal(out[..., :-1], np.ones((1, 6))) and out[0, -1] == 1e3
    assert np.array_equal(ad.normalize_action(raw, stats, kind, n_pass=0)[..., :-1], back[..., :-1])
    with pytest.raises(ValueError, match="action_normalization_type"):
        ad.normalize_action(x, stats, "minmax")


# ------------------------------------------------------------------------------------------------- the refusals --
def _model(**kw):
    from src.model.vla.pizero import PiZero

    c = ref_cfg(O.TINY_DIMS)
    c.update(kw)
    return PiZero(c, init="none")


def test_prefix_len_refusals_name_their_keys():
    m = _model()
    H = O.TINY_DIMS["horizon_steps"]
    with pytest.raises(ValueError, match=r"prefix_len must lie in \[0, horizon_steps - 1\]"):
        m._prefix_len(torch.tensor([0, H, 1]), 3)
    with pytest.raises(ValueError, match="prefix_len must lie in"):
        m._prefix_len(torch.tensor([0, -1, 1]), 3)
    with pytest.raises(ValueError, match="prefix_len has 2 entries"):
        m._prefix_len(torch.tensor([0, 1]), 3)
    with pytest.raises(ValueError, match="prefix_len must be integers"):
        m._prefix_len(torch.tensor([0.0, 1.0, 2.0]), 3)
    z = torch.zeros(3, H, 7)
    with pytest.raises(NotImplementedError, match="infer_action_naive.*prefix"):
        m.infer_action_naive(None, None, None, None, None, None, None, prefix_actions=z,
                             prefix_len=torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="prefix_actions and prefix_len go together"):
        m.infer_action(None, None, None, None, None, None, None, None, noise=z, prefix_actions=z)


def test_adaln_with_a_prefix_is_refused_by_name():
    from pizero_native.engine import PREFIX_ADAPTIVE_MSG
    from src.model.vla.pizero import PiZero
    from tests.golden.make_golden_adaln import adaptive_cfg

    assert "action_expert_adaptive_mode" in PREFIX_ADAPTIVE_MSG and "action_prefix_max_delay" in PREFIX_ADAPTIVE_MSG
    m = PiZero(adaptive_cfg(O.TINY_DIMS, "adaLN"), init="none")
    with pytest.raises(NotImplementedError, match="action_expert_adaptive_mode"):
        m._prefix_len(torch.tensor([0, 1, 2]), 3)


def test_train_agent_prefix_lengths_per_micro_batch():
    """TrainAgent._prefix_len on an agent built without its GPU-bound constructor: the draw of (seed, cnt_batch, rank),
    the batch's own action_prefix_len in its place, its range check, and nothing drawn with the key at 0 (the
    constructor's refusals need a device: tests/test_prefix_gpu.py)"""
    from src.agent import train as T

    a = T.TrainAgent.__new__(T.TrainAgent)
    a.cfg = ref_cfg(O.TINY_DIMS)
    a.action_prefix_max_delay, a.action_prefix_seed, a.micro_batches_seen, a.rank = 3, 9, 4, 1
    a.cnt_batch = 3  # a resumed agent: the checkpoint's index trails the count of micro-batches consumed by one
    H = O.TINY_DIMS["horizon_steps"]
    ids = torch.zeros(5, 2, dtype=torch.int64)
    from pizero_native import augment as A

    got = a._prefix_len({"input_ids": ids})
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), A.draw_prefix_len(5, 3, 9, 4, 1))
    over = a._prefix_len({"input_ids": ids, "action_prefix_len": [0, 1, 2, 3, 0]})  # the batch's own lengths win
    assert over.tolist() == [0, 1, 2, 3, 0]
    with pytest.raises(ValueError, match="action_prefix_len"):
        a._prefix_len({"input_ids": ids, "action_prefix_len": [0, 1, 2, H, 0]})
    a.action_prefix_max_delay = 0
    st = torch.get_rng_state()
    assert a._prefix_len({"input_ids": ids}) is None and torch.equal(torch.get_rng_state(), st)


def test_abi_lists_the_prefix_entry_points():
    from pizero_native._lib import SIGNATURES

    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    for name in ("pz_flow_psi_prefix", "pz_concat_time_prefix", "pz_flow_loss_prefix", "pz_time_embed_rows_prefix",
                 "pz_action_in_prefix", "pz_action_out_prefix", "pz_euler_step_prefix", "pz_action_prefix_init",
                 "pz_clamp_prefix", "pz_action_normalize", "pz_action_denormalize_prefix"):
        assert name in SIGNATURES and f"int {name}(" in hdr, name


def test_null_prefix_len_is_an_argument_error():
    """the prefix entry points refuse a NULL prefix_len on the host, before any launch (no GPU needed)"""
    import pizero_native

    L = pizero_native.lib()
    one = 16  # any non-null address: the argument check fails first, nothing is dereferenced
    assert L.pz_flow_psi_prefix(one, one, one, None, one, 1, 4, 7, 0.001, None) == 1
    assert b"flow_psi_prefix" in L.pz_last_error()
    assert L.pz_action_prefix_init(one, one, None, 1, 4, 7, None) == 1
    assert L.pz_clamp_prefix(one, None, 1, 4, 7, -1.0, 1.0, None) == 1
    assert L.pz_action_denormalize_prefix(one, one, one, None, 1, 4, 7, 1, one, one, 0, None) == 1
    assert b"action_denormalize_prefix" in L.pz_last_error()
