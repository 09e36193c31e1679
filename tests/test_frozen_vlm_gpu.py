"""The frozen-VLM training pass (train_vlm: False; Engine.vlm_forward_only): the VLM runs forward-only into
the joint K/V buffers, the action expert alone keeps activations and runs a backward.

Expert gradients do not depend on whether the VLM trains, so the reference fixtures of tests/test_pizero_gpu.py
(tiny / full / b16), tests/test_adaln_gpu.py (adaln) and the restatement of tests/prefix_ref.py pin this pass directly,
at their unchanged gates.  The tiny fixture (head_dim 32) runs the GEMM fallback on the expert's query rows, the full
dims run pz_expert_attn_fwd / pz_expert_attn_bwd.
"""

import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.golden.make_golden import ref_cfg
from tests.oracle_helpers import O, load_golden
from tests.pizero_gpu_helpers import GRAD_COS, GRAD_REL, build_gpu_model, check_grads_probe, gpu_inputs, run_loss

pytestmark = pytest.mark.gpu

D_MIX = (0, 1, 3)  # prefix lengths of the three tiny samples (tests/test_prefix_gpu.py's)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _vlm_names(m):
    return [n for n in m._arena.order if m._arena.slots[n].region in ("vlm", "lora")]


def _freeze(m):
    """what TrainAgent does for train_vlm: False"""
    for p in m.trainable_vlm_parameters:
        p.requires_grad = False
    for p in getattr(m, "lora_trainable_vlm_parameters", []) if m.has_lora else []:
        p.requires_grad = False
    assert not m._vlm_needs_grad()
    assert m._engine().vlm_forward_only is True
    return m


def _check_loss(g, loss):
    ref, rb = float(g["fp32/loss"]), float(g["bf16/loss"])
    tol = max(3 * abs(rb - ref), 1e-2 * abs(ref))
    print(f"loss {loss:.6f} reference fp32 {ref:.6f} bf16 {rb:.6f} tol {tol:.2e}")
    assert abs(loss - ref) <= tol, (loss, ref, rb)
    return tol


def _gate(g, m, label):
    """the unchanged gradient gate on every trainable tensor; no VLM tensor has a gradient; nothing passes by skipping"""
    named = dict(m.named_parameters())
    for n in _vlm_names(m):
        assert m._param(n).grad is None, f"{n}: frozen VLM tensor has a gradient"
    w = check_grads_probe(g, named, label=label, skip_frozen=True)
    trainable = [str(n) for n in g["grad_names"] if named[str(n)].requires_grad]
    assert trainable and w["n"] + w.get("noise", 0) == len(trainable), (w, len(trainable))
    return w


def _saved(m, gi):
    """the saved state of one training forward"""
    eng = m._engine()
    box = {}
    orig = eng.train_forward

    def wrap(*a, save, **k):
        box["save"] = save
        return orig(*a, save=save, **k)

    eng.train_forward = wrap
    try:
        run_loss(m, gi, backward=False)
    finally:
        del eng.train_forward
    return box["save"]


@pytest.fixture(scope="module")
def tiny():
    d = O.TINY_DIMS
    g = load_golden("tiny")
    m = _freeze(build_gpu_model(d))
    return d, g, m, gpu_inputs(m, d, int(g["bsz"]))


@pytest.fixture(scope="module")
def full_model():
    return _freeze(build_gpu_model(O.FULL_DIMS))


@pytest.fixture(scope="module")
def full(full_model):
    d = O.FULL_DIMS
    g = load_golden("full")
    return d, g, full_model, gpu_inputs(full_model, d, int(g["bsz"]))


# ---------------------------------------------------------------------------------------------- fixture gates --
def test_tiny_fixture_gate_gemm_fallback(tiny):
    d, g, m, gi = tiny
    assert not m._engine()._expert_kernels_ok(m._engine().d.C + m._engine().d.H)
    loss = run_loss(m, gi)
    _check_loss(g, loss.item())
    _gate(g, m, "frozen tiny")


def test_full_fixture_gate_new_kernels(full):
    d, g, m, gi = full
    assert m._engine()._expert_kernels_ok(m._engine().d.C + m._engine().d.H)
    loss = run_loss(m, gi)
    _check_loss(g, loss.item())
    _gate(g, m, "frozen full B=2")


def test_microbatch64_batch_invariance(full_model):
    """the 16 fixture samples x 4 in different row orders against b16.npz: batch strides of the new kernels and of the
    forward-only pass at the benched GEMM routes"""
    d, m = O.FULL_DIMS, full_model
    g = load_golden("b16")
    gi = gpu_inputs(m, d, 16, repeat=4)
    assert gi["input_ids"].shape[0] == 64
    loss = run_loss(m, gi)
    _check_loss(g, loss.item())
    _gate(g, m, "frozen micro-batch 64")


# ------------------------------------------------------------------------------------ no VLM activation saved --
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_saved_state_holds_no_vlm_activation(which, request):
    d, g, m, gi = request.getfixturevalue(which)
    sv = _saved(m, gi)
    assert sv["frozen"] and not sv.get("sv_v")  # no SigLIP state
    assert [gr.name for gr in sv["groups"]] == ["expert"]
    assert len(sv["joint"]) == m._engine().d.nL
    for st in sv["joint"]:
        assert "vlm" not in st["g"] and set(st["g"]) == {"expert"}
    eng = m._engine()
    try:
        eng.vlm_forward_only = False
        old = _saved(m, gi)
    finally:
        eng.vlm_forward_only = True
    assert not old["frozen"] and old["sv_v"] and "vlm" in old["joint"][0]["g"]  # the check can tell the two apart


def _act_peak(m, gi):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run_loss(m, gi)
    return torch.cuda.max_memory_allocated() - base


def test_activation_peak_at_most_half(full_model):
    """Full dims, B = 16: peak memory of forward + backward above what was allocated before.  The old pass keeps at
    least 17 x 276 x 49152 x 2 B (0.46 GB) per sample of MLP activations alone; the new pass keeps
    18 x Lp x 256 x 2 x 2 B (5 MB) per sample of K/V plus one layer's transients: at most half is a condition from
    the shapes, not a measurement."""
    d, m = O.FULL_DIMS, full_model
    gi = gpu_inputs(m, d, 16)
    eng = m._engine()
    run_loss(m, gi)  # workspaces, the lent K/V buffers and the gradient arena exist before either measurement
    new = _act_peak(m, gi)
    try:
        eng.vlm_forward_only = False
        run_loss(m, gi)
        old = _act_peak(m, gi)
    finally:
        eng.vlm_forward_only = True
    print(f"activation peak at B=16: vlm_forward_only False {old / 2**30:.3f} GiB, True {new / 2**30:.3f} GiB")
    assert old >= 16 * 17 * 276 * 49152 * 2
    assert new <= old / 2


# ----------------------------------------------------------------------------------- old pass against new pass --
def test_old_and_new_pass_agree(full):
    d, g, m, gi = full
    eng = m._engine()
    new = run_loss(m, gi).item()
    tol = _check_loss(g, new)
    _gate(g, m, "new pass")
    try:
        eng.vlm_forward_only = False
        old = run_loss(m, gi).item()
        _check_loss(g, old)
        _gate(g, m, "old pass")
    finally:
        eng.vlm_forward_only = True
    print(f"loss old pass {old:.6f} new pass {new:.6f}")
    assert abs(old - new) <= tol


# ---------------------------------------------------------------------------------------- per-feature cases --
@pytest.mark.parametrize("mode", ["adaLN", "adaLN-Zero"])
def test_adaln_expert(mode):
    from tests.golden.make_golden_adaln import FIXTURE
    from tests.test_adaln_gpu import build_adaptive_model

    d = O.TINY_DIMS
    g = np.load(os.path.join(ROOT, "tests", "golden", FIXTURE[mode] + ".npz"))
    m = _freeze(build_adaptive_model(d, mode))
    gi = gpu_inputs(m, d, int(g["bsz"]))
    loss = run_loss(m, gi)
    _check_loss(g, loss.item())
    _gate(g, m, f"frozen {mode}")


def _loss_prefix(m, g, prefix_len):
    m.zero_grad(set_to_none=True)
    loss = m(input_ids=g["input_ids"], pixel_values=g["pixel_values"], causal_mask=g["causal_mask"],
             vlm_position_ids=g["vpos"], proprio_position_ids=g["ppos"], action_position_ids=g["apos"],
             proprios=g["proprios"], actions=g["actions32"], t=g["t32"], noise=g["x0"], prefix_len=prefix_len)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item()


def _whole_tensor_gate(names, got, want, dev_of, label):
    """per tensor GRAD_REL / GRAD_COS on the whole gradient, widened to 3 x the reference's own deviation ``dev_of(n)``
    where that is larger (tests/test_prefix_gpu.py's rule)"""
    bad, worst = [], [0.0, 1.0]
    for n in names:
        a, w = got[n].double().cpu().flatten(), want[n].double().cpu().flatten()
        wn = float(w.norm())
        if wn == 0.0:
            if float(a.abs().max()) != 0.0:
                bad.append((n, "reference gradient is exactly 0"))
            continue
        brel = dev_of(n, w, wn)
        if brel > 1.0:
            continue
        tol = max(GRAD_REL, 3.0 * brel)
        rel = float((a - w).norm()) / wn
        cos = float(a @ w) / (float(a.norm()) * wn + 1e-300)
        worst = [max(worst[0], rel), min(worst[1], cos)]
        if rel > tol or cos < min(GRAD_COS, 1.0 - 0.5 * tol * tol):
            bad.append((n, round(rel, 5), round(cos, 6), round(tol, 4)))
    print(f"[{label}] {len(names)} tensors: max rel-L2 {worst[0]:.4f}, min cos {worst[1]:.6f}")
    assert not bad, "\n".join(map(str, bad))


def test_action_prefix_matches_the_restatement(tiny):
    from tests.prefix_ref import restatement_run

    d, g, m, gi = tiny
    r32, _ = restatement_run(d, 3, D_MIX)
    r16, _ = restatement_run(d, 3, D_MIX, bf16=True)
    loss = _loss_prefix(m, gi, torch.tensor(D_MIX))
    tol = max(3 * abs(r16["loss"] - r32["loss"]), 1e-2 * abs(r32["loss"]))
    print(f"prefix loss {loss:.6f} restatement {r32['loss']:.6f} (bf16 {r16['loss']:.6f})")
    assert abs(loss - r32["loss"]) <= tol
    names = m._trainable_names()
    assert len(names) > 10 and not any(n in set(_vlm_names(m)) for n in names)
    got = {n: m._param(n).grad.detach() for n in names}
    _whole_tensor_gate(names, got, r32["grads"],
                       lambda n, w, wn: float((r16["grads"][n].double().flatten() - w).norm()) / wn, "frozen prefix")


def test_frozen_lora_adapters_are_included():
    """lora: True with nothing trainable in the VLM and NON-ZERO adapters: the forward-only pass reads the merged
    shadow, so it agrees with the old pass (which sums the adapter terms inside its GEMMs) at the gate's tolerances;
    without the adapter term it would not"""
    from tests.test_lora_gpu import build_lora_model

    d = O.TINY_DIMS
    m = _freeze(build_lora_model(d))
    gi = gpu_inputs(m, d, 3)
    eng = m._engine()
    new = run_loss(m, gi).item()
    names = m._trainable_names()
    gn = {n: m._param(n).grad.detach().clone() for n in names}
    try:
        eng.vlm_forward_only = False
        old = run_loss(m, gi).item()
        go = {n: m._param(n).grad.detach().clone() for n in names}
    finally:
        eng.vlm_forward_only = True
    print(f"frozen LoRA: loss old pass {old:.6f} new pass {new:.6f}")
    assert abs(new - old) <= 1e-2 * abs(old)
    _whole_tensor_gate(names, gn, go, lambda n, w, wn: 0.0, "frozen LoRA new vs old")
    # the adapters matter: zeroing lora_B moves the loss by more than the two passes differ (a pass that dropped the
    # adapter term would sit at the zeroed loss)
    with torch.no_grad():
        for n in m._arena.order:
            if n.endswith(".lora_B"):
                m._param(n).zero_()
    bare = run_loss(m, gi, backward=False).item()
    print(f"frozen LoRA: loss with zeroed adapters {bare:.6f}")
    assert abs(bare - old) > 2 * abs(new - old)


# ------------------------------------------------------------------------------------------------ determinism --
def test_two_frozen_steps_bitwise(full):
    d, g, m, gi = full
    l1 = run_loss(m, gi).item()
    g1 = m._arena.grad.clone()
    l2 = run_loss(m, gi).item()
    assert l1 == l2
    assert torch.equal(g1, m._arena.grad)


# ------------------------------------------------------------------------------------------------- TrainAgent --
def _agent_cfg(**kw):
    c = ref_cfg(O.TINY_DIMS)
    c.update(dict(global_batch_size=8, per_device_batch_size=4, action_lr=1e-3, vlm_lr=1e-3,
                  action_weight_decay=0.0, vlm_weight_decay=0.0, max_grad_norm=1.0, n_updates=3, log_freq=1,
                  train_vlm=False, use_bf16=True, flow_sampling="beta", load_pretrained_weights=False,
                  action_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2),
                  vlm_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2)))
    c.update(kw)
    return c


def _one_update(agent, batch, seed):
    from pizero_native.optim import clip_grad_norm_

    torch.manual_seed(seed)
    inputs = agent.preprocess_batch(batch)
    loss = agent.model(**inputs, noise=torch.zeros(inputs["actions"].shape, device="cuda"))
    loss.backward()
    clip_grad_norm_(agent.optimizers, agent.max_grad_norm)
    for o in agent.optimizers:
        o.step()
        o.zero_grad(set_to_none=True)
    agent.action_lr_scheduler.step()
    return loss.item()


def test_train_agent_train_vlm_false(tmp_path, caplog):
    """three optimizer steps with accumulation 2: finite losses, every VLM tensor bit-unchanged, expert tensors
    changed; save, then resume, reproduces the next step bit for bit"""
    import logging

    from src.agent.train import SyntheticBridgeDataset, TrainAgent

    with caplog.at_level(logging.INFO):
        a = TrainAgent(_agent_cfg(log_dir=str(tmp_path), save_model_freq=3))
    assert any("frozen-VLM pass active" in r.getMessage() for r in caplog.records)
    assert a.grad_accumulation_steps == 2 and a.optimizers == [a.action_optimizer]
    m = a.model
    assert not m._vlm_needs_grad() and m._engine().vlm_forward_only
    vlm = _vlm_names(m)
    before = {n: m._arena.view(n).clone() for n in m._arena.order}
    losses = []
    orig = m._engine().train_forward

    def wrap(*args, **k):
        out = orig(*args, **k)
        assert k["save"]["frozen"]
        losses.append(out)
        return out

    m._engine().train_forward = wrap
    try:
        a.run()
    finally:
        del m._engine().train_forward
    assert a.cnt_update == 3 and len(losses) == 6
    assert all(bool(torch.isfinite(x).all()) for x in losses)
    for n in vlm:
        assert torch.equal(before[n], m._arena.view(n)), f"{n}: frozen VLM tensor changed"
    changed = [n for n in m._trainable_names() if not torch.equal(before[n], m._arena.view(n))]
    assert "action_decoder.weight" in changed and len(changed) > 10
    path = tmp_path / "checkpoint" / "step3.pt"
    assert path.exists()
    b = TrainAgent(_agent_cfg(resume_checkpoint_path=str(path)))
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    batch = next(iter(SyntheticBridgeDataset(_agent_cfg(), 4, seed=9)))
    la, lb = _one_update(a, batch, 5), _one_update(b, batch, 5)
    assert la == lb
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------- untied proprio / action --
@pytest.mark.parametrize("dims", ["tiny", "full"])
def test_untied_mixtures_old_and_new_pass_agree(dims):
    """Without tie_action_proprio_weights the expert side is two groups (proprio, whose last-layer output is dropped,
    and action): the new kernels then read one joint O / dO buffer that is split into / gathered from the groups' rows
    (full dims), the GEMM fallback takes the groups as they are (tiny).  New pass against old pass at the gate's
    tolerances."""
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.model.vla.pizero import PiZero

    d = O.TINY_DIMS if dims == "tiny" else O.FULL_DIMS
    m = PiZero(ref_cfg(d), device="cuda", dtype=torch.bfloat16, init="none")
    m.freeze_unused_weights()
    for name in m._arena.order:
        v = m._arena.view(name)
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    torch.cuda.synchronize()
    assert not m._tied
    _freeze(m)
    gi = gpu_inputs(m, d, 2)
    eng = m._engine()
    sv = _saved(m, gi)
    assert sv["frozen"] and [gr.name for gr in sv["groups"]] == ["proprio", "action"]
    assert ("lse" in sv["joint"][0]) == (dims == "full")
    new = run_loss(m, gi).item()
    names = m._trainable_names()
    gn = {n: m._param(n).grad.detach().clone() for n in names}
    try:
        eng.vlm_forward_only = False
        old = run_loss(m, gi).item()
        go = {n: m._param(n).grad.detach().clone() for n in names}
    finally:
        eng.vlm_forward_only = True
    print(f"untied {dims}: loss old pass {old:.6f} new pass {new:.6f}")
    assert abs(new - old) <= 1e-2 * abs(old)
    assert any(n.startswith("joint_model.mixtures.proprio.") for n in names)
    _whole_tensor_gate(names, gn, go, lambda n, w, wn: 0.0, f"untied {dims} new vs old")
