"""EvalAgent.act (raw observation -> robot-unit actions in one graph replay) and the training-side resize, on the MI355X.

TINY_DIMS model with generator-defined weights (the agents leave an inference model's weights to the checkpoint).
act is held to EvalAgent.infer_chunk on host-prepared inputs: bit for bit before the denormalisation when the frames
are already at the model's resolution, within test_eval_agent_graph_matches_eager's atol = 1e-2 when they are resized
(a 1-code difference in a pixel is legitimate under the resize criterion of tests/test_obs_kernels_gpu.py); a graph
replay equals the eager launches of the same kernels bit for bit, and inputs of one replay do not leak into the next.
"""

import json
import os

import numpy as np
import pytest
import torch

from tests import obs_ref as R
from tests.conftest import ROOT
from tests.golden.make_golden import ref_cfg
from tests.oracle_helpers import O

pytestmark = pytest.mark.gpu

ATOL = 2e-5  # tests/test_obs_kernels_gpu.py: fp32 evaluation of the normalisation formulas


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bridge_stats():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")))


def _identity_proprio_stats():
    """Bridge action statistics; gaussian proprio statistics with mean 0 and std 1 - 1e-8, so that the proprio
    normalisation (x - 0) / (std + 1e-8) is the identity"""
    s = _bridge_stats()
    s["proprio"]["mean"] = [0.0] * 7
    s["proprio"]["std"] = [1.0 - 1e-8] * 7
    return s


def _cfg(stats_path=None, proprio="gaussian", action="bound"):
    c = ref_cfg(O.TINY_DIMS)
    c.update(dict(use_bf16=True, load_pretrained_weights=False))
    if stats_path is not None:
        c["env"] = dict(adapter=dict(dataset_statistics_path=str(stats_path), proprio_normalization_type=proprio,
                                     action_normalization_type=action))
    return c


def _agent(cfg, use_graph=True):
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.agent.eval import EvalAgent

    ag = EvalAgent(cfg, use_graph=use_graph)
    ar = ag.model._arena
    for name in ar.order:
        v = ar.view(name)
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    torch.cuda.synchronize()
    return ag


def _batch(cfg, B, seed):
    from src.agent.train import SyntheticBridgeDataset

    return next(iter(SyntheticBridgeDataset(cfg, B, seed=seed)))


@pytest.fixture(scope="module")
def stats_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("obs") / "stats.json"
    p.write_text(json.dumps(_identity_proprio_stats()))
    return p


@pytest.fixture(scope="module")
def agent(stats_file):
    return _agent(_cfg(stats_file))


def test_act_without_statistics_names_the_key():
    from src.agent.eval import EvalAgent

    ag = EvalAgent(_cfg(None))
    b = _batch(_cfg(None), 1, 0)
    with pytest.raises(ValueError, match="env.adapter.dataset_statistics_path"):
        ag.act(b["pixel_values"], b["input_ids"], b["attention_mask"], b["proprio"], channels_last=False)


def test_act_at_model_resolution_equals_infer_chunk(agent, stats_file):
    from src.agent.env_adapter.base import BaseEnvAdapter

    cfg = _cfg(stats_file)
    b = _batch(cfg, 2, seed=3)
    noise = torch.randn(2, 4, 7, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    pix = (b["pixel_values"].float() / 255 - 0.5) / 0.5  # host-normalised, as test_eval_agent_graph_matches_eager
    want_norm = agent.infer_chunk(b["input_ids"], b["attention_mask"], pix, b["proprio"], noise=noise).clone()
    out = agent.act(b["pixel_values"], b["input_ids"], b["attention_mask"], b["proprio"], noise=noise,
                    channels_last=False)
    g = agent.observation_graph(2, (56, 56), channels_last=False)
    assert out.shape == (2, 4, 7) and out.dtype == torch.float32
    assert float(want_norm.float().abs().max()) > 0
    # before the denormalisation: the very bits of infer_chunk (which returns the fp32 chunk rounded to bf16)
    assert torch.equal(g.out_norm.to(torch.bfloat16).view(torch.int16), want_norm.view(torch.int16))
    # after it: the host adapter on the same normalised chunk
    host = BaseEnvAdapter().denormalize_action(g.out_norm.double().cpu().numpy(), _bridge_stats(), "bound")
    err = np.abs(out.double().cpu().numpy() - host).max()
    print(f"act vs host denormalisation: max |d| = {err:.3e}")
    assert err <= ATOL
    assert torch.equal(out[..., -1], g.out_norm[..., -1])  # the gripper passes through
    # channels-last frames give the same result
    out_cl = agent.act(b["pixel_values"].permute(0, 2, 3, 1).contiguous().numpy(), b["input_ids"], b["attention_mask"],
                       b["proprio"], noise=noise)
    assert torch.equal(out_cl, out)


def test_act_on_resized_frames_matches_infer_chunk_on_the_restatement(agent, stats_file):
    cfg = _cfg(stats_file)
    b = _batch(cfg, 2, seed=5)
    r = np.random.default_rng(11)
    frames = np.stack([R.low_frequency_frame(131, 97, seed=s) for s in (1, 2)])
    frames = np.clip(frames.astype(np.int32) + r.integers(-40, 41, frames.shape), 0, 255).astype(np.uint8)
    noise = torch.randn(2, 4, 7, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    _, codes = R.resize(frames, 56)
    pix = torch.from_numpy(R.pixel_norm(codes)).float()
    want = agent.infer_chunk(b["input_ids"], b["attention_mask"], pix, b["proprio"], noise=noise).float().clone()
    agent.act(frames, b["input_ids"], b["attention_mask"], b["proprio"], noise=noise)
    got = agent.observation_graph(2, (131, 97)).out_norm
    err = float((got - want).abs().max())
    print(f"act on 131x97 frames vs infer_chunk on the restatement's codes: max |d| = {err:.3e}")
    assert torch.allclose(got, want, atol=1e-2)


def test_graph_replay_equals_eager_and_does_not_leak(agent, stats_file):
    cfg = _cfg(stats_file, proprio="bound", action="gaussian")
    (stats_file.parent / "bridge.json").write_text(json.dumps(_bridge_stats()))
    cfg["env"]["adapter"]["dataset_statistics_path"] = str(stats_file.parent / "bridge.json")
    gr = _agent(cfg, use_graph=True)
    eg = _agent(cfg, use_graph=False)
    r = np.random.default_rng(4)
    s = _bridge_stats()["proprio"]
    lo, hi = np.array(s["p01"]), np.array(s["p99"])
    outs = []
    for i in range(2):
        b = _batch(cfg, 2, seed=20 + i)
        frames = r.integers(0, 256, (2, 57, 55, 3), dtype=np.uint8)
        prop = torch.from_numpy(lo + (hi - lo) * r.uniform(-0.1, 1.1, (2, 1, 7))).float()
        noise = torch.randn(2, 4, 7, device="cuda", generator=torch.Generator("cuda").manual_seed(30 + i))
        a_graph = gr.act(frames, b["input_ids"], b["attention_mask"], prop, noise=noise).clone()
        a_eager = eg.act(frames, b["input_ids"], b["attention_mask"], prop, noise=noise).clone()
        assert torch.equal(a_graph.view(torch.int32), a_eager.view(torch.int32)), (i, (a_graph - a_eager).abs().max())
        outs.append(a_graph)
    assert gr.observation_graph(2, (57, 55)).graph is not None and eg.observation_graph(2, (57, 55)).graph is None
    assert not torch.equal(outs[0], outs[1])
    # the second observation again on a fresh eager agent state == its replay: nothing of the first one remains
    # (already shown per step above); and the first observation replayed after the second gives its first result
    b = _batch(cfg, 2, seed=20)
    r = np.random.default_rng(4)
    frames = r.integers(0, 256, (2, 57, 55, 3), dtype=np.uint8)
    prop = torch.from_numpy(lo + (hi - lo) * r.uniform(-0.1, 1.1, (2, 1, 7))).float()
    noise = torch.randn(2, 4, 7, device="cuda", generator=torch.Generator("cuda").manual_seed(30))
    again = gr.act(frames, b["input_ids"], b["attention_mask"], prop, noise=noise)
    assert torch.equal(again, outs[0])


def _train_cfg():
    c = ref_cfg(O.TINY_DIMS)
    c.update(dict(global_batch_size=4, per_device_batch_size=4, action_lr=1e-3, vlm_lr=1e-3,
                  action_weight_decay=0.0, vlm_weight_decay=0.0, max_grad_norm=1.0, n_updates=1, log_freq=1,
                  train_vlm=True, use_bf16=True, flow_sampling="beta", load_pretrained_weights=False,
                  action_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2),
                  vlm_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2)))
    return c


def test_preprocess_batch_resizes_frames_off_the_model_resolution():
    from pizero_native import ops
    from src.agent.train import TrainAgent

    c = _train_cfg()
    a = TrainAgent(c)
    b = _batch(c, 4, seed=7)
    native = b["pixel_values"]
    assert native.shape == (4, 3, 56, 56) and native.dtype == torch.uint8
    # at the model's size: the parent's torch expression, untouched
    same = a.preprocess_batch(b)["pixel_values"]
    want = ((native.cuda().to(torch.float32) / 255.0 - 0.5) / 0.5).to(torch.bfloat16)
    assert torch.equal(same.view(torch.int16), want.view(torch.int16))
    # off it: the resize kernel
    big = torch.randint(0, 256, (4, 3, 131, 97), dtype=torch.uint8, generator=torch.Generator().manual_seed(8))
    inputs = a.preprocess_batch(dict(b, pixel_values=big))
    pv = inputs["pixel_values"]
    assert pv.shape == (4, 3, 56, 56) and pv.dtype == torch.bfloat16
    assert torch.equal(pv.view(torch.int16), ops.image_resize_norm(big.cuda(), 56, channels_last=False).view(torch.int16))
    loss = a.model(**inputs)
    assert torch.isfinite(loss).all()
