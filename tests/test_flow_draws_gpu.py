"""Several flow draws per observation (flow_samples_per_observation): B observations x S draws (t, x0) train
on B * S pairs that share the observation's one forward-only VLM prefill.

The feature is defined by an equivalence -- the loss and gradients of today's frozen-VLM pass on the batch in which
every observation is repeated S times with those (t, x0) -- and the tests pin it: against the CPU oracle on the
replicated batch (tests/draws_ref.py) at tiny dims (the GEMM attention fallback), against the unchanged fixture gates
and against today's pass on the replicated batch at full dims (pz_expert_attn_fwd_shared / _bwd_shared).
"""

import logging

import numpy as np
import pytest
import torch

from tests.golden.make_golden import ref_cfg
from tests.oracle_helpers import O, load_golden
from tests.pizero_gpu_helpers import build_gpu_model, gpu_inputs
from tests.test_frozen_vlm_gpu import _agent_cfg, _check_loss, _freeze, _gate, _vlm_names, _whole_tensor_gate

pytestmark = pytest.mark.gpu

KEY = "flow_samples_per_observation"
D_MIX = (0, 1, 3)  # prefix lengths of the three tiny samples (tests/test_prefix_gpu.py's)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(m, g, t, x0, prefix_len=None, backward=True):
    m.zero_grad(set_to_none=True)
    kw = {} if prefix_len is None else dict(prefix_len=prefix_len)
    loss = m(input_ids=g["input_ids"], pixel_values=g["pixel_values"], causal_mask=g["causal_mask"],
             vlm_position_ids=g["vpos"], proprio_position_ids=g["ppos"], action_position_ids=g["apos"],
             proprios=g["proprios"], actions=g["actions32"], t=t, noise=x0, **kw)
    if backward:
        loss.backward()
    torch.cuda.synchronize()
    return loss.item()


def _grads(m):
    return {n: m._param(n).grad.detach().clone() for n in m._trainable_names()}


def _replicated(g, S):
    """the batch with every observation repeated S times: sample e = b * S + s"""
    return {k: v.repeat_interleave(S, dim=0) for k, v in g.items()}


def _distinct_draws(g, S, seed=11):
    """t [B, S] in [0.02, 0.98] and x0 [B, S, H, A], all different, on the device"""
    B, H, A = g["actions32"].shape
    gen = torch.Generator().manual_seed(seed)
    t = torch.rand(B, S, generator=gen) * 0.96 + 0.02
    x0 = torch.randn(B, S, H, A, generator=gen)
    return t.cuda(), x0.cuda()


def _vs_replicated(m, g, S, label, prefix_len=None):
    """S distinct draws through the new path against today's pass on the B * S replicated batch: loss within 1 % and
    every gradient at the whole-tensor gate (GRAD_REL / GRAD_COS); the deviations are printed"""
    B, H, A = g["actions32"].shape
    t, x0 = _distinct_draws(g, S)
    new = _run(m, g, t, x0, prefix_len)
    gn = _grads(m)
    pl = None if prefix_len is None else torch.as_tensor(prefix_len).repeat_interleave(S)
    old = _run(m, _replicated(g, S), t.reshape(B * S), x0.reshape(B * S, H, A), pl)
    go = _grads(m)
    print(f"[{label}] loss {S} draws {new:.7f}, replicated batch {old:.7f}, |d| {abs(new - old):.3e}")
    assert abs(new - old) <= 1e-2 * abs(old)
    names = m._trainable_names()
    assert len(names) > 10
    _whole_tensor_gate(names, gn, go, lambda n, w, wn: 0.0, label)


def _spy(eng, name, box):
    orig = getattr(eng, name)

    def wrap(*a, **k):
        box.append((a, k))
        return orig(*a, **k)

    setattr(eng, name, wrap)
    return lambda: delattr(eng, name)


@pytest.fixture(scope="module")
def tiny():
    d = O.TINY_DIMS
    m = _freeze(build_gpu_model(d))
    return d, m, gpu_inputs(m, d, 3)


@pytest.fixture(scope="module")
def full():
    d = O.FULL_DIMS
    g = load_golden("full")
    m = _freeze(build_gpu_model(d))
    return d, g, m, gpu_inputs(m, d, int(g["bsz"]))


# ------------------------------------------------------------------------------- tiny: against the CPU oracle --
def test_tiny_two_draws_match_the_oracle_on_the_replicated_batch(tiny):
    """B = 3, S = 2, GEMM fallback: loss within max(3 |bf16 - fp32|, 1e-2 |fp32|) of the oracle's on the replicated
    batch, gradients at the whole-tensor gate widened by the oracle's own bf16 deviation"""
    from tests.draws_ref import draws_run

    d, m, gi = tiny
    assert not m._engine()._expert_kernels_ok(m._engine().d.C + m._engine().d.H)
    r32, _ = draws_run(d, 3, 2)
    r16, _ = draws_run(d, 3, 2, bf16=True)
    t, x0 = torch.from_numpy(r32["t"]).cuda(), torch.from_numpy(r32["x0"]).cuda()
    loss = _run(m, gi, t, x0)
    tol = max(3 * abs(r16["loss"] - r32["loss"]), 1e-2 * abs(r32["loss"]))
    print(f"2 draws: loss {loss:.6f} oracle on the replicated batch fp32 {r32['loss']:.6f} bf16 {r16['loss']:.6f} "
          f"tol {tol:.2e}")
    assert abs(loss - r32["loss"]) <= tol
    names = m._trainable_names()
    assert len(names) > 10 and not any(n in set(_vlm_names(m)) for n in names)
    _whole_tensor_gate(names, _grads(m), r32["grads"],
                       lambda n, w, wn: float((r16["grads"][n].double().flatten() - w).norm()) / wn, "tiny 2 draws")


def test_t_with_one_draw_axis_is_todays_step(tiny):
    """t [B, 1] (noise [B, 1, H, A]): the loss and the gradient arena of t [B], bit for bit"""
    d, m, gi = tiny
    l1 = _run(m, gi, gi["t32"], gi["x0"])
    g1 = m._arena.grad.clone()
    l2 = _run(m, gi, gi["t32"][:, None], gi["x0"][:, None])
    assert l1 == l2 and torch.equal(g1, m._arena.grad)


def test_tiny_prefix_len_mixed(tiny):
    d, m, gi = tiny
    _vs_replicated(m, gi, 2, "tiny prefix (0, 1, 3) x 2 draws", prefix_len=torch.tensor(D_MIX))
    # [B, S]: a prefix length per pair
    B, H, A = gi["actions32"].shape
    t, x0 = _distinct_draws(gi, 2)
    pl = torch.tensor([[0, 2], [1, 1], [3, 0]])
    new = _run(m, gi, t, x0, pl)
    gn = m._arena.grad.clone()
    old = _run(m, _replicated(gi, 2), t.reshape(B * 2), x0.reshape(B * 2, H, A), pl.reshape(B * 2))
    print(f"[tiny prefix per pair] loss {new:.7f} replicated {old:.7f}")
    assert abs(new - old) <= 1e-2 * abs(old)
    rel = float((gn.double() - m._arena.grad.double()).norm() / m._arena.grad.double().norm())
    print(f"[tiny prefix per pair] gradient arena rel-L2 {rel:.3e}")
    assert rel <= 0.08


@pytest.mark.parametrize("mode", ["adaLN", "adaLN-Zero"])
def test_tiny_adaln_expert(mode):
    from tests.test_adaln_gpu import build_adaptive_model

    d = O.TINY_DIMS
    m = _freeze(build_adaptive_model(d, mode))
    _vs_replicated(m, gpu_inputs(m, d, 3), 2, f"tiny {mode} x 2 draws")


def _untied_model(d):
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.model.vla.pizero import PiZero

    m = PiZero(ref_cfg(d), device="cuda", dtype=torch.bfloat16, init="none")
    m.freeze_unused_weights()
    for name in m._arena.order:
        v = m._arena.view(name)
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    torch.cuda.synchronize()
    assert not m._tied
    return _freeze(m)


def test_tiny_untied_mixtures():
    d = O.TINY_DIMS
    m = _untied_model(d)
    _vs_replicated(m, gpu_inputs(m, d, 3), 2, "tiny untied x 2 draws")
    assert any(n.startswith("joint_model.mixtures.proprio.") for n in m._trainable_names())


# ------------------------------------------------------------------------------------- full dims: new kernels --
def _identical(gi, S):
    B, H, A = gi["actions32"].shape
    return gi["t32"][:, None].expand(B, S).contiguous(), gi["x0"][:, None].expand(B, S, H, A).contiguous()


def test_full_identical_draws_pass_the_fixture_gates(full):
    """S = 3 draws that each copy the fixture's (t, x0): the mean over pairs is the fixture's loss, so the unchanged
    loss and gradient gates of the ``full`` fixture hold"""
    d, g, m, gi = full
    assert m._engine()._expert_kernels_ok(m._engine().d.C + m._engine().d.H)
    loss = _run(m, gi, *_identical(gi, 3))
    _check_loss(g, loss)
    _gate(g, m, "full B=2 x 3 identical draws")


def test_full_distinct_draws_match_the_replicated_batch(full):
    d, g, m, gi = full
    _vs_replicated(m, gi, 3, "full B=2 x 3 draws vs 6-sample replicated batch")


def test_full_two_identical_steps_bitwise(full):
    d, g, m, gi = full
    t, x0 = _distinct_draws(gi, 3)
    l1 = _run(m, gi, t, x0)
    g1 = m._arena.grad.clone()
    l2 = _run(m, gi, t, x0)
    assert l1 == l2 and torch.equal(g1, m._arena.grad)


def test_full_saved_state(full):
    """the VLM K/V once per observation, the own K/V per pair, no VLM activation, one prefill for B observations"""
    d, g, m, gi = full
    eng = m._engine()
    B, S = gi["input_ids"].shape[0], 3
    fwd, pre = [], []
    undo = [_spy(eng, "train_forward", fwd), _spy(eng, "prefill", pre)]
    try:
        _run(m, gi, *_distinct_draws(gi, S), backward=False)
    finally:
        for u in undo:
            u()
    assert len(fwd) == 1 and len(pre) == 1
    assert pre[0][0][0].shape[0] == B and pre[0][0][2].numel() == B  # ids and cnt of the prefill: B observations
    sv = fwd[0][1]["save"]
    assert sv["frozen"] and sv["draws"] == S and sv["B"] == B * S and not sv.get("sv_v")
    assert sv["cnt"].numel() == B * S
    assert [gr.name for gr in sv["groups"]] == ["expert"] and len(sv["joint"]) == eng.d.nL
    T = eng.d.C + eng.d.H
    for st in sv["joint"]:
        assert set(st["g"]) == {"expert"}
        assert st["K"].shape == (B, eng.d.Lp, eng.d.hd) and st["V"].shape == st["K"].shape
        assert st["Ko"].shape == (B * S, T, eng.d.hd) and st["Vo"].shape == st["Ko"].shape
        assert st["Q"].shape[0] == B * S and st["lse"].shape[0] == B * S
    # all layers' shared K/V are views of one [nL, B, Lp, hd] buffer: B, not B * S, batches of it exist
    assert sv["joint"][1]["K"].data_ptr() - sv["joint"][0]["K"].data_ptr() == B * eng.d.Lp * eng.d.hd * 2


def test_draws_need_the_frozen_pass(full):
    d, g, m, gi = full
    eng = m._engine()
    t, x0 = _identical(gi, 2)
    try:
        eng.vlm_forward_only = False
        with pytest.raises(ValueError, match=KEY):
            _run(m, gi, t, x0)
    finally:
        eng.vlm_forward_only = True
    p = m.trainable_vlm_parameters[0]
    try:
        p.requires_grad = True
        with pytest.raises(ValueError, match=KEY):
            _run(m, gi, t, x0)
    finally:
        p.requires_grad = False
    with pytest.raises(ValueError, match=KEY):  # noise for another S
        _run(m, gi, t, gi["x0"])


# ------------------------------------------------------------------------------------------------- TrainAgent --
def _one_update(agent, batch, seed):
    from pizero_native.optim import clip_grad_norm_

    torch.manual_seed(seed)
    inputs = agent.preprocess_batch(batch)
    B, H, A = inputs["actions"].shape
    assert inputs["t"].shape == (B, agent.flow_samples)
    loss = agent.model(**inputs, noise=torch.zeros(B, agent.flow_samples, H, A, device="cuda"))
    loss.backward()
    clip_grad_norm_(agent.optimizers, agent.max_grad_norm)
    for o in agent.optimizers:
        o.step()
        o.zero_grad(set_to_none=True)
    agent.action_lr_scheduler.step()
    return loss.item()


def test_train_agent_two_draws(tmp_path, caplog):
    """three optimizer steps with accumulation 2 and 2 draws per observation: finite losses, the log line, every VLM
    tensor bit-unchanged, expert tensors changed; save, then resume, reproduces the next step bit for bit"""
    from src.agent.train import SyntheticBridgeDataset, TrainAgent

    cfg = lambda **kw: _agent_cfg(flow_samples_per_observation=2, **kw)  # noqa: E731
    with caplog.at_level(logging.INFO):
        a = TrainAgent(cfg(log_dir=str(tmp_path), save_model_freq=3))
    assert any(KEY + " 2" in r.getMessage() for r in caplog.records)
    assert a.flow_samples == 2 and a.optimizers == [a.action_optimizer]
    m = a.model
    before = {n: m._arena.view(n).clone() for n in m._arena.order}
    calls = []
    undo = _spy(m._engine(), "train_forward", calls)
    try:
        a.run()
    finally:
        undo()
    assert a.cnt_update == 3 and len(calls) == 6
    for args, k in calls:
        assert k["draws"] == 2 and k["t"].numel() == 8 and k["ids"].shape[0] == 4 and k["save"]["frozen"]
    for n in _vlm_names(m):
        assert torch.equal(before[n], m._arena.view(n)), f"{n}: frozen VLM tensor changed"
    changed = [n for n in m._trainable_names() if not torch.equal(before[n], m._arena.view(n))]
    assert "action_decoder.weight" in changed and len(changed) > 10
    path = tmp_path / "checkpoint" / "step3.pt"
    assert path.exists()
    b = TrainAgent(cfg(resume_checkpoint_path=str(path)))
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    batch = next(iter(SyntheticBridgeDataset(cfg(), 4, seed=9)))
    la, lb = _one_update(a, batch, 5), _one_update(b, batch, 5)
    assert np.isfinite(la) and la == lb
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_train_agent_one_draw_consumes_the_generator_as_before():
    """flow_samples_per_observation 1 (and the key absent): preprocess_batch draws the times it always drew"""
    from src.agent.train import SyntheticBridgeDataset, TrainAgent

    batch = next(iter(SyntheticBridgeDataset(_agent_cfg(), 4, seed=9)))
    ts = []
    for kw in ({}, {KEY: 1}):
        a = TrainAgent(_agent_cfg(**kw))
        torch.manual_seed(3)
        ts.append(a.preprocess_batch(batch)["t"])
        assert ts[-1].shape == (4,)
        torch.manual_seed(3)
        assert torch.equal(ts[-1].cpu(), a.sample_fm_time(4).to(torch.bfloat16))
    assert torch.equal(ts[0], ts[1])


def test_train_agent_refuses_draws_with_a_trainable_vlm(monkeypatch):
    from src.agent.train import TrainAgent
    from src.model.vla.pizero import PiZero
    from tests.golden.make_golden_lora import lora_cfg

    with pytest.raises(ValueError, match=KEY):
        TrainAgent(_agent_cfg(train_vlm=True, **{KEY: 2}))
    with pytest.raises(ValueError, match=KEY):
        TrainAgent(_agent_cfg(**{KEY: 0}))
    monkeypatch.setattr(PiZero, "load_pretrained_weights", lambda self: None)  # the default init stands in
    c = lora_cfg(O.TINY_DIMS)
    c.update(dict(global_batch_size=8, per_device_batch_size=4, action_lr=1e-3, vlm_lr=1e-3,
                  action_weight_decay=0.0, vlm_weight_decay=0.0, max_grad_norm=1.0, n_updates=3, log_freq=1,
                  use_bf16=True, flow_sampling="beta",
                  action_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2),
                  vlm_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2)))
    c.update(dict(lora=True, train_vlm=True, load_pretrained_weights=True, **{KEY: 2}))
    with pytest.raises(ValueError, match=KEY):
        TrainAgent(c)
