"""End-to-end parity of the adaLN / adaLN-Zero action expert against the reference fixtures.

tests/golden/{adaln,adaln_zero}.npz (tests/golden/make_golden_adaln.py, which runs the REFERENCE at TINY_DIMS,
B=3, ragged, fp32 + bf16) hold the loss, gradient probes of every parameter and the action chunk of
``infer_action_naive`` -- the reference's cached ``infer_action`` raises in these modes, so both native entry
points are held to the naive result.  Gates: the ones of tests/test_pizero_gpu.py, unchanged (the reference's own
bf16 deviations here -- loss 1.4406 vs 1.4453, actions mean 5e-3 / max 5e-2 on |a| <= 3.1 -- are of tiny.npz's order).
"""

import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.golden.make_golden_adaln import FIXTURE, adaptive_cfg
from tests.oracle_helpers import O
from tests.pizero_gpu_helpers import check_grads_probe, gpu_inputs, run_infer, run_loss

pytestmark = pytest.mark.gpu

MODES = ("adaLN", "adaLN-Zero")
NEW = "joint_model.mixtures.action.layers.1.post_attention_layernorm.to_gamma.0.weight"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _check_loss(g, loss):
    ref, rb = float(g["fp32/loss"]), float(g["bf16/loss"])
    tol = max(3 * abs(rb - ref), 1e-2 * abs(ref))
    print(f"loss {loss:.6f} reference fp32 {ref:.6f} bf16 {rb:.6f} tol {tol:.2e}")
    assert abs(loss - ref) <= tol, (loss, ref, rb)


def _check_grads(g, m, label):
    return check_grads_probe(g, dict(m.named_parameters()), label=label)


def _check_actions(g, a, key, sel=None):
    ref = g[f"fp32/{key}"]
    rb = g[f"bf16/{key}"]
    if sel is not None:  # a sub-batch of the fixture's samples (samples are independent)
        ref, rb = ref[list(sel)], rb[list(sel)]
    a = a.float().cpu().numpy()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    dev = np.abs(rb - ref)
    err = np.abs(a - ref)
    print(f"{key}: mean|d| {err.mean():.3e} (reference bf16 {dev.mean():.3e}), max|d| {err.max():.3e} ({dev.max():.3e})")
    assert err.mean() <= max(3 * dev.mean(), 5e-3), (err.mean(), dev.mean())
    assert err.max() <= max(3 * dev.max(), 3e-2), (err.max(), dev.max())


def build_adaptive_model(d, mode):
    """tests.pizero_gpu_helpers.build_gpu_model with the adaptive mode set: generator-defined weights by name"""
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.model.vla.pizero import PiZero

    m = PiZero(adaptive_cfg(d, mode), device="cuda", dtype=torch.bfloat16, init="none")
    m.tie_action_proprio_weights()
    m.freeze_unused_weights()
    for name in m._arena.order:
        v = m._arena.view(name)
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    torch.cuda.synchronize()
    return m


@pytest.fixture(scope="module", params=MODES)
def ada(request):
    d = O.TINY_DIMS
    g = np.load(os.path.join(ROOT, "tests", "golden", FIXTURE[request.param] + ".npz"))
    m = build_adaptive_model(d, request.param)
    gi = gpu_inputs(m, d, int(g["bsz"]))
    return d, g, m, gi


def _naive(m, gi, clip):
    return m.infer_action_naive(input_ids=gi["input_ids"], pixel_values=gi["pixel_values"].float(),
                                causal_mask=gi["causal_mask"], vlm_position_ids=gi["vpos"],
                                proprio_position_ids=gi["ppos"], action_position_ids=gi["apos"],
                                proprios=gi["proprios"], noise=gi["noise"], clip=clip)


def test_loss_and_all_grads(ada):
    d, g, m, gi = ada
    loss = run_loss(m, gi)
    _check_loss(g, loss.item())
    w = _check_grads(g, m, "adaLN tiny")
    assert w.get("noise", 0) == 2  # the two SigLIP k_proj.bias only: no adaLN tensor in the noise-only branch


def test_run_loss_twice_bitwise(ada):
    d, g, m, gi = ada
    l1 = run_loss(m, gi).item()
    g1 = m._arena.grad.clone()
    l2 = run_loss(m, gi).item()
    assert l1 == l2
    assert torch.equal(g1, m._arena.grad)


def test_grad_accumulation(ada):
    d, g, m, gi = ada
    run_loss(m, gi)
    p = dict(m.named_parameters())[NEW.replace("mixtures.action.", "mixtures.proprio.")]
    g1 = p.grad.float().clone()
    assert float(g1.abs().max()) > 0
    run_loss(m, gi, accumulate=True)
    g2 = p.grad.float().clone()
    assert torch.allclose(g2, 2 * g1, rtol=2e-2, atol=1e-3)  # test_tiny_grad_accumulation_and_zero's bound
    m.zero_grad(set_to_none=True)
    assert p.grad is None


def test_batch_invariance_repeat2(ada):
    d, g, m, gi = ada
    gi2 = gpu_inputs(m, d, int(g["bsz"]), repeat=2)
    assert gi2["input_ids"].shape[0] == 2 * int(g["bsz"])
    loss = run_loss(m, gi2)
    _check_loss(g, loss.item())
    _check_grads(g, m, "adaLN tiny x2")


def test_actions_cached_and_naive(ada):
    d, g, m, gi = ada
    a = run_infer(m, gi, clip=False)
    _check_actions(g, a, "actions_naive_unclipped")
    a2 = _naive(m, gi, clip=False)
    _check_actions(g, a2, "actions_naive_unclipped")
    assert torch.equal(a, a2)
    a3 = run_infer(m, gi, clip=True)
    assert a3.abs().max().item() <= 1.0
    _check_actions(g, a3, "actions_naive_clipped")


def test_actions_gemm_attention_path(ada, monkeypatch):
    """the GEMM + softmax attention path of the denoise step (query rows starting at token P)"""
    d, g, m, gi = ada
    monkeypatch.setattr(m._engine(), "infer_flash", False)
    _check_actions(g, run_infer(m, gi, clip=False), "actions_naive_unclipped")


def test_actions_single_sample(ada):
    d, g, m, gi = ada
    g1 = gpu_inputs(m, d, int(g["bsz"]), select=[0])
    a = run_infer(m, g1, clip=False)
    _check_actions(g, a, "actions_naive_unclipped", sel=[0])


def test_actions_hipgraph_bitwise(ada):
    from pizero_native.graph import InferenceGraph

    d, g, m, gi = ada
    B = int(g["bsz"])
    eager = run_infer(m, gi, clip=False)
    ig = InferenceGraph(m, B, clip=False)
    ig.load(gi["input_ids"], gi["pixel_values"], m.block_prefix_counts(gi["itp"], gi["amask"]), gi["vpos"], gi["ppos"],
            gi["apos"], gi["proprios"].float(), gi["noise"])
    ig.capture()
    for _ in range(2):
        a = ig.replay()
    torch.cuda.synchronize()
    _check_actions(g, a.clone(), "actions_naive_unclipped")
    assert torch.equal(a.float(), eager.float()), float((a.float() - eager.float()).abs().max())


def test_fp8_with_adaptive_mode_raises(ada):
    d, g, m, gi = ada
    with pytest.raises(NotImplementedError, match="fp8 inference is not available with action_expert_adaptive_mode"):
        m.use_fp8_inference(True)
    with pytest.raises(NotImplementedError, match="fp8 inference is not available with action_expert_adaptive_mode"):
        m._engine().prepare_fp8()
    assert m._engine().f8 is None


def test_actions_general_mask_path(ada):
    """A caller mask that is not the Pi0 block pattern takes the additive-mask path: the denoise step's
    [B, C + H, L] mask is rebuilt from the caller's pair.  (a) The block pattern handed over as a general additive
    mask is the same computation as the block-count GEMM path: it meets the fixture gate and agrees with that
    path to bf16 rounding of the actions' range (|a| <= 3.1: 2^-7 per element at most).  (b) A genuinely different
    mask -- action rows blind to the proprio token -- goes through the public entry point and changes the chunk."""
    from pizero_native.engine import GeneralMask

    d, g, m, gi = ada
    eng = m._engine()
    B = gi["input_ids"].shape[0]
    prev = eng.infer_flash
    eng.infer_flash = False
    try:
        blk = run_infer(m, gi, clip=False).float()
    finally:
        eng.infer_flash = prev
    k, v = m._kv_buffers(B)
    spec = GeneralMask(itp=gi["itp"][:, 0].float().contiguous(), act=gi["amask"][:, 0].float().contiguous())
    a = eng.infer_action(gi["input_ids"], gi["pixel_values"], spec, gi["vpos"], gi["ppos"], gi["apos"],
                         gi["proprios"].float().contiguous(), gi["noise"].float().contiguous(), k, v, clip=False)
    torch.cuda.synchronize()
    _check_actions(g, a, "actions_naive_unclipped")
    assert float((a.float() - blk).abs().max()) <= 2.0 ** -7
    P, C = d["max_seq_len"], d["cond_steps"]
    am = gi["amask"].clone()
    am[:, :, :, P:P + C] = torch.finfo(torch.bfloat16).min
    assert isinstance(m._mask_spec([gi["itp"], am], [torch.arange(P + C, device="cuda"),
                                                     torch.arange(P + C, P + C + am.shape[2], device="cuda")]), GeneralMask)
    e = dict(gi, amask=am)
    a2 = run_infer(m, e, clip=False).float()
    assert bool(torch.isfinite(a2).all())
    assert float((a2 - blk).abs().max()) > 1e-3
