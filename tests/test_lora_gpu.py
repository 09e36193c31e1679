"""End-to-end parity of LoRA fine-tuning (lora: True) against the reference fixture.

tests/golden/lora.npz (tests/golden/make_golden_lora.py: the REFERENCE at TINY_DIMS, B=3, ragged, fp32 + bf16, rank 8,
non-zero lora_B, after tie / freeze_unused_weights / freeze_non_lora_weights_in_vlm) holds the loss, gradient probes of
every parameter (-1 where the reference has no grad) and the action chunk of the reference's cached infer_action after
model.eval(), which merges W += B A.  Gates: the ones of tests/test_adaln_gpu.py, unchanged.
"""

import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.golden.make_golden_lora import lora_cfg
from tests.oracle_helpers import O
from tests.pizero_gpu_helpers import check_grads_probe, gpu_inputs, run_infer, run_loss
from tests.test_adaln_gpu import _check_actions, _check_loss

pytestmark = pytest.mark.gpu

LB = "joint_model.mixtures.vlm.layers.1.mlp.gate_proj.lora_B"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def build_lora_model(d, cfg=None, zero_b=False, freeze=True):
    """tests.pizero_gpu_helpers.build_gpu_model with LoRA on: generator-defined weights by name"""
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.model.vla.pizero import PiZero

    m = PiZero(cfg if cfg is not None else lora_cfg(d), device="cuda", dtype=torch.bfloat16, init="none")
    m.tie_action_proprio_weights()
    m.freeze_unused_weights()
    if freeze:
        m.freeze_non_lora_weights_in_vlm()
    for name in m._arena.order:
        v = m._arena.view(name)
        if zero_b and name.endswith(".lora_B"):
            v.zero_()
            continue
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    torch.cuda.synchronize()
    return m


@pytest.fixture(scope="module")
def lora():
    d = O.TINY_DIMS
    g = np.load(os.path.join(ROOT, "tests", "golden", "lora.npz"))
    m = build_lora_model(d)
    gi = gpu_inputs(m, d, int(g["bsz"]))
    return d, g, m, gi


def test_loss_and_all_grads(lora):
    d, g, m, gi = lora
    m.zero_grad(set_to_none=True)
    loss = run_loss(m, gi)
    _check_loss(g, loss.item())
    named = dict(m.named_parameters())
    trainable = set(str(n) for n in g["trainable"])
    assert set(n for n, p in named.items() if p.requires_grad) == trainable
    for n, p in named.items():
        if n not in trainable:
            assert p.grad is None, f"{n}: frozen but has a gradient"
    check_grads_probe(g, named, label="lora tiny")
    # the last vlm layer's q adapter: trainable, exactly zero gradient (its queries feed nothing)
    last = d["n_layers"] - 1
    for ab in ("lora_A", "lora_B"):
        q = named[f"joint_model.mixtures.vlm.layers.{last}.self_attn.q_proj.{ab}"]
        assert q.grad is not None and float(q.grad.float().abs().max()) == 0.0


def test_run_loss_twice_bitwise(lora):
    d, g, m, gi = lora
    l1 = run_loss(m, gi).item()
    g1 = m._arena.grad.clone()
    l2 = run_loss(m, gi).item()
    assert l1 == l2
    assert torch.equal(g1, m._arena.grad)


def test_grad_accumulation(lora):
    d, g, m, gi = lora
    m.zero_grad(set_to_none=True)
    run_loss(m, gi)
    p = dict(m.named_parameters())[LB]
    g1 = p.grad.float().clone()
    assert float(g1.abs().max()) > 0
    run_loss(m, gi, accumulate=True)
    g2 = p.grad.float().clone()
    assert torch.allclose(g2, 2 * g1, rtol=2e-2, atol=1e-3)  # test_tiny_grad_accumulation_and_zero's bound
    m.zero_grad(set_to_none=True)
    assert p.grad is None


def _graph(m, gi, B):
    from pizero_native.graph import InferenceGraph

    ig = InferenceGraph(m, B, clip=False)
    ig.load(gi["input_ids"], gi["pixel_values"], m.block_prefix_counts(gi["itp"], gi["amask"]), gi["vpos"], gi["ppos"],
            gi["apos"], gi["proprios"].float(), gi["noise"])
    return ig.capture()


def test_actions_merged_eager_and_graph_base_untouched(lora):
    d, g, m, gi = lora
    base = m._arena.data.clone()
    a = run_infer(m, gi, clip=False)
    _check_actions(g, a, "actions_unclipped")
    a3 = run_infer(m, gi, clip=True)
    assert a3.abs().max().item() <= 1.0
    _check_actions(g, a3, "actions_clipped")
    ig = _graph(m, gi, int(g["bsz"]))
    for _ in range(2):
        ag = ig.replay()
    torch.cuda.synchronize()
    _check_actions(g, ag.clone(), "actions_unclipped")
    assert torch.equal(ag.float(), a.float())
    # train -> infer -> train: the base weights are bit-equal, and state_dict() holds them (unmerged) plus the adapters
    run_loss(m, gi)
    run_infer(m, gi, clip=False)
    assert torch.equal(base, m._arena.data)
    sd = m.state_dict()
    n = "joint_model.mixtures.vlm.layers.0.mlp.down_proj."
    assert torch.equal(sd[n + "weight"], m._arena.view(n + "weight")) and n + "lora_A" in sd and n + "lora_B" in sd
    merged = m._engine().ar.view(n + "weight", m._engine()._merged)
    assert not torch.equal(merged, sd[n + "weight"])  # non-zero B: the shadow differs from the base
    ref = sd[n + "weight"].float() + sd[n + "lora_B"].float() @ sd[n + "lora_A"].float()
    assert float((merged.float() - ref).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())  # two bf16 roundings


def test_graph_replay_sees_optimizer_step(lora):
    """one optimizer step, then a replay of the graph captured before it == a fresh model loaded from the stepped
    state_dict, bit for bit"""
    from pizero_native.optim import FusedAdamW

    d, g, _, _ = lora
    m = build_lora_model(d)
    gi = gpu_inputs(m, d, int(g["bsz"]))
    ig = _graph(m, gi, int(g["bsz"]))
    before = ig.replay().clone()
    opt = FusedAdamW(m.lora_trainable_vlm_parameters, lr=1e-2, state_bits=32)
    run_loss(m, gi)
    opt.step()
    after = ig.replay().clone()
    torch.cuda.synchronize()
    assert not torch.equal(before, after)
    m2 = build_lora_model(d)
    m2.load_state_dict(m.state_dict(), strict=True)
    a2 = run_infer(m2, gpu_inputs(m2, d, int(g["bsz"])), clip=False)
    assert torch.equal(after.float(), a2.float()), float((after.float() - a2.float()).abs().max())


def test_zero_b_matches_plain_model(lora):
    """B = 0: the adapters add exactly nothing -- loss and actions equal the same model built without LoRA"""
    from tests.golden.make_golden import ref_cfg

    d, g, _, _ = lora
    m0 = build_lora_model(d, zero_b=True)
    mp = build_lora_model(d, cfg=ref_cfg(d), freeze=False)
    gi0, gip = gpu_inputs(m0, d, int(g["bsz"])), gpu_inputs(mp, d, int(g["bsz"]))
    l0, lp = run_loss(m0, gi0, backward=False).item(), run_loss(mp, gip, backward=False).item()
    a0, ap = run_infer(m0, gi0, clip=False), run_infer(mp, gip, clip=False)
    print(f"B = 0: loss {l0!r} vs plain {lp!r}; actions max|d| {float((a0.float() - ap.float()).abs().max()):.3e}")
    assert torch.equal(a0.float(), ap.float())
    assert l0 == lp


def test_lora_with_adaln_zero(lora):
    d, g, _, _ = lora
    cfg = lora_cfg(d)
    cfg.action_expert_adaptive_mode = "adaLN-Zero"
    cfg.joint.config.action_expert_adaptive_mode = "adaLN-Zero"
    for mixes in (cfg.mixture, cfg.joint.config.mixture):
        for k in ("proprio", "action"):
            mixes[k].adaptive_mode = "adaLN-Zero"
    m = build_lora_model(d, cfg=cfg)
    gi = gpu_inputs(m, d, int(g["bsz"]))
    loss = run_loss(m, gi)
    assert bool(torch.isfinite(loss))
    p = dict(m.named_parameters())
    for n in (LB, LB.replace("lora_B", "lora_A"), "vision_tower.vision_model.encoder.layers.0.mlp.fc1.lora_B"):
        assert p[n].grad is not None and float(p[n].grad.float().abs().max()) > 0, n


def test_lora_with_fp8_inference_quantises_merged_weights(lora):
    from pizero_native import ops

    d, g, _, _ = lora
    m = build_lora_model(d)
    gi = gpu_inputs(m, d, int(g["bsz"]))
    m.use_fp8_inference(True)
    eng = m._engine()
    n = "joint_model.mixtures.vlm.layers.0.mlp.down_proj.weight"
    merged = eng.ar.view(n, eng._merged)
    q, sc = eng.f8[n]
    sc_ref = ops.fp8_weight_scale(merged)
    q_ref = torch.empty_like(q)
    ops.fp8_quant_tensor(merged, q_ref, sc_ref)
    q_base = torch.empty_like(q)
    ops.fp8_quant_tensor(m._arena.view(n), q_base, ops.fp8_weight_scale(m._arena.view(n)))
    torch.cuda.synchronize()
    assert sc == sc_ref and torch.equal(q, q_ref) and not torch.equal(q, q_base)
    a = run_infer(m, gi, clip=False)
    assert bool(torch.isfinite(a.float()).all())
