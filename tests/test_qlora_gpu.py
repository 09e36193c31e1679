"""QLoRA end to end (quantize: True with lora: True), pinned without a tolerance.

Model A is the rank-8 LoRA model of tests/test_lora_gpu.py built with quantize: True.  Model B is the plain LoRA model
with the same weights whose every quantisable base weight is overwritten with the numpy restatement's
dequant(quant(W)) (tests/quant4_ref.py).  A and B then run the same GEMMs on the same operand bits, so the loss, every
gradient and the action chunk (eager and captured) must be bit-equal, before and after an optimizer step.  B is pinned
to the reference by tests/golden/lora.npz (tests/test_lora_gpu.py), so A is the reference's LoRA on a base that differs
by the quantisation alone."""

import numpy as np
import pytest
import torch

from tests.oracle_helpers import O
from tests.pizero_gpu_helpers import gpu_inputs, run_infer, run_loss
from tests.qlora_helpers import bits_of, qlora_cfg, ref_roundtrip_
from tests.test_lora_gpu import _graph, build_lora_model

pytestmark = pytest.mark.gpu

BSZ = 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pair(qtype="fp4", **kw):
    d = O.TINY_DIMS
    a = build_lora_model(d, cfg=qlora_cfg(d, qtype), **kw)
    b = build_lora_model(d, **kw)
    ref = ref_roundtrip_(b, a._q4_names(), qtype)
    return d, a, b, ref


@pytest.fixture(scope="module")
def pair():
    d, a, b, ref = _pair()
    return d, a, b, ref, gpu_inputs(a, d, BSZ), gpu_inputs(b, d, BSZ)


def _grads(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad}


def _same_step(a, b, ga, gb, what):
    la, lb = run_loss(a, ga).item(), run_loss(b, gb).item()
    assert la == lb, f"{what}: loss {la!r} vs {lb!r}"
    A, B = _grads(a), _grads(b)
    assert list(A) == list(B) and any("lora_" in n for n in A) and any("lora_" not in n for n in A)
    for n in A:
        assert torch.equal(A[n].view(torch.int16), B[n].view(torch.int16)), f"{what}: gradient of {n}"
    assert any(float(A[n].float().abs().max()) > 0 for n in A if "lora_A" in n)
    xa, xb = run_infer(a, ga), run_infer(b, gb)
    assert torch.equal(xa.float(), xb.float()), f"{what}: eager action chunk"
    return xa


def test_packed_state_equals_the_restatement_and_memory(pair):
    d, a, b, ref, ga, gb = pair
    names = a._q4_names()
    plain_total, side_total = b._arena.total, a._arena.side_total
    if a._q4 is None:  # built and filled in bf16, in the arena's side buffer, until packed
        assert a._arena.side is not None and a._arena.side.numel() == side_total
    a.quantize_base_()
    torch.cuda.synchronize()
    # every packed tensor is the restatement's, bit for bit
    for n in names:
        q, r = a._q4.w[n], ref[n]
        assert np.array_equal(q.packed.cpu().numpy(), r["packed"]), n
        assert np.array_equal(q.absmax.cpu().numpy(), r["absmax"]), n
        assert np.array_equal(q.nested_absmax.cpu().numpy().view(np.uint32), r["nested_absmax"].view(np.uint32)), n
        assert np.float32(q.offset) == r["offset"], n
    # memory, on sizes against the slot table: no bf16 parameter or gradient element of a quantised weight
    ar = a._arena
    assert ar.side is None
    quant = sum(-(-ar.slots[n].numel // 8) * 8 for n in names)
    kept = sum(-(-s.numel // 8) * 8 for s in ar.slots.values() if not s.side)
    assert side_total >= quant > 0
    assert ar.data.numel() == ar.total == -(-kept // 64) * 64
    assert plain_total - quant - 64 < ar.total <= plain_total - quant + 64
    run_loss(a, ga)
    assert ar.grad.numel() == ar.data.numel()
    for n in names:
        p = a._param(n)
        assert p.dtype == torch.uint8 and not p.requires_grad and p.grad is None
        with pytest.raises(RuntimeError, match="packed to 4 bits"):
            ar.view(n)
    # packed: 0.5 B per weight + one absmax byte per 64, + 4 B per 256 blocks and 4 B per tensor
    nw = sum(ar.slots[n].numel for n in names)
    blocks = sum(-(-ar.slots[n].numel // 64) for n in names)
    small = sum(4 * -(-(-(-ar.slots[n].numel // 64)) // 256) + 4 for n in names)
    assert a._q4.nbytes() == nw // 2 + blocks + small
    assert small <= 0.01 * nw or nw < 1 << 20  # negligible at real sizes; tiny tensors pay 8 B each
    # training holds one scratch, sized for the largest fused site, and no shadow
    eng = a._engine()
    most = max(sum(ar.slots[f"{pre}{pr}.weight"].numel for pr in projs) for pre, projs in a._vlm_linear_sites())
    assert eng._q4_buf.numel() == most and eng._merged is None and eng._merged_side is None


def test_loss_grads_actions_bitwise_before_and_after_a_step(pair):
    from pizero_native.optim import FusedAdamW

    d, a, b, ref, ga, gb = pair
    xa = _same_step(a, b, ga, gb, "step 0")
    iga, igb = _graph(a, ga, BSZ), _graph(b, gb, BSZ)
    ra, rb = iga.replay().clone(), igb.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(ra.float(), rb.float()) and torch.equal(ra.float(), xa.float())
    assert a._engine()._merged is None  # the shadow of a quantised model holds the 4-bit set alone
    opts = [FusedAdamW(m.lora_trainable_vlm_parameters, lr=1e-2, state_bits=32) for m in (a, b)]
    run_loss(a, ga), run_loss(b, gb)
    for o in opts:
        o.step()
    x1 = _same_step(a, b, ga, gb, "after one step")
    assert not torch.equal(x1.float(), xa.float())
    ra, rb = iga.replay().clone(), igb.replay().clone()  # the captured graphs see the rebuilt shadow
    torch.cuda.synchronize()
    assert torch.equal(ra.float(), rb.float()) and torch.equal(ra.float(), x1.float())
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.detach().view(torch.int16), pb[n].detach().view(torch.int16)), n


def test_nf4_loss_and_actions_bitwise():
    d, a, b, ref = _pair("nf4")
    ga, gb = gpu_inputs(a, d, BSZ), gpu_inputs(b, d, BSZ)
    _same_step(a, b, ga, gb, "nf4")
    assert a._q4.qtype == "nf4" and any(k.endswith("bitsandbytes__nf4") for k in a.state_dict())


def test_quantize_without_lora_is_a_frozen_vlm():
    """quantize: True, lora: False: no VLM tensor is trainable and the loss equals model B's with zero lora_B.  B's
    adapters are frozen as well, so that both models take the frozen-VLM pass -- with trainable adapters B
    would run the full joint pass, whose kernels differ from the forward-only ones whatever the weights are."""
    d = O.TINY_DIMS
    a = build_lora_model(d, cfg=qlora_cfg(d, lora=False), freeze=False)
    vlm = [p for part in (a.vision_tower, a.multi_modal_projector, a.joint_model.mixtures["vlm"])
           for p in part.parameters()]
    assert vlm and not any(p.requires_grad for p in vlm) and not a._vlm_needs_grad()
    assert any(p.requires_grad for p in a.action_expert_parameters)
    b = build_lora_model(d, zero_b=True)
    ref_roundtrip_(b, a._q4_names(), "fp4")
    for p in b.lora_trainable_vlm_parameters:
        p.requires_grad = False
    ga, gb = gpu_inputs(a, d, BSZ), gpu_inputs(b, d, BSZ)
    la, lb = run_loss(a, ga).item(), run_loss(b, gb).item()
    assert la == lb
    A, B = _grads(a), _grads(b)
    assert list(A) == list(B) and A
    for n in A:
        assert torch.equal(A[n].view(torch.int16), B[n].view(torch.int16)), n
    assert torch.equal(run_infer(a, ga).float(), run_infer(b, gb).float())
    eng = a._engine()
    n0 = a._q4_names()[0]
    shadow = eng.ar.view(n0, eng._merged_side)
    assert torch.equal(shadow.view(torch.int16), b._arena.view(n0).view(torch.int16))  # the shadow is dequant(W4)


def test_state_dict_round_trips(pair):
    d, a, b, ref, ga, gb = pair
    la = run_loss(a, ga, backward=False).item()
    sd = a.state_dict()
    n0 = a._q4_names()[0]
    numel = a._arena.slots[n0].numel
    assert sd[n0].dtype == torch.uint8 and tuple(sd[n0].shape) == (numel // 2, 1)
    from pizero_native.quant4 import parse_quant_state, state_keys

    keys = list(sd)
    i = keys.index(n0)
    assert keys[i:i + 6] == [n0[: -len("weight")] + k for k in state_keys("fp4")]
    st = parse_quant_state(sd[n0 + ".quant_state.bitsandbytes__fp4"])
    assert tuple(st["shape"]) == a._arena.slots[n0].shape and st["blocksize"] == 64
    assert tuple(sd[n0 + ".quant_map"].shape) == (16,) and tuple(sd[n0 + ".nested_quant_map"].shape) == (256,)
    # packed tensors into a fresh model: installed without requantising, the loss comes back bit for bit
    m2 = build_lora_model(d, cfg=qlora_cfg(d))
    m2.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    for n in a._q4_names():
        assert torch.equal(m2._q4.w[n].packed, a._q4.w[n].packed) and m2._q4.w[n].offset == a._q4.w[n].offset, n
    assert run_loss(m2, gpu_inputs(m2, d, BSZ), backward=False).item() == la
    # a bf16 state_dict (the raw weights A was built from) loaded into a packed model quantises on load
    raw = build_lora_model(d)
    m3 = build_lora_model(d, cfg=qlora_cfg(d))
    m3.quantize_base_()
    with torch.no_grad():
        for n in m3._q4_names()[:3]:
            m3._q4.w[n].packed.zero_()
    rsd = raw.state_dict()
    for k in rsd:  # the adapters A trained in the test above, the rest as built
        if "lora_" in k:
            rsd[k] = sd[k]
    m3.load_state_dict(rsd, strict=True)
    for n in a._q4_names():
        assert torch.equal(m3._q4.w[n].packed, a._q4.w[n].packed), n
        assert torch.equal(m3._q4.w[n].absmax, a._q4.w[n].absmax), n
    assert run_loss(m3, gpu_inputs(m3, d, BSZ), backward=False).item() == la
    # ... and before quantize_base_() a bf16 load is a plain copy, packed by the first forward
    m4 = build_lora_model(d, cfg=qlora_cfg(d))
    m4.load_state_dict(rsd, strict=True)
    assert m4._q4 is None
    assert run_loss(m4, gpu_inputs(m4, d, BSZ), backward=False).item() == la
    with pytest.raises(RuntimeError, match="missing keys"):
        m4.load_state_dict({k: v for k, v in sd.items() if k != n0 + ".absmax" and k != n0}, strict=True)


def test_train_agent_checkpoint_resumes_bitwise(tmp_path, monkeypatch):
    from src.agent.train import SyntheticBridgeDataset, TrainAgent
    from src.model.vla.pizero import PiZero
    from tests.test_agents_gpu import _one_update

    monkeypatch.setattr(PiZero, "load_pretrained_weights", lambda self: None)  # the default init stands in

    def cfg(**kw):
        c = qlora_cfg(O.TINY_DIMS)
        c.update(dict(global_batch_size=8, per_device_batch_size=4, action_lr=1e-3, vlm_lr=1e-3,
                      action_weight_decay=0.0, vlm_weight_decay=0.0, max_grad_norm=1.0, n_updates=2, log_freq=1,
                      train_vlm=True, use_bf16=True, flow_sampling="beta", load_pretrained_weights=True,
                      lora=True, quantize=True,
                      action_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2),
                      vlm_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2)))
        c.update(kw)
        return c

    a = TrainAgent(cfg(log_dir=str(tmp_path), save_model_freq=2))
    assert a.model._q4 is not None and a.model._arena.side is None  # packed by the agent, before the first step
    a.run()
    path = tmp_path / "checkpoint" / "step2.pt"
    assert path.exists()
    b = TrainAgent(cfg(resume_checkpoint_path=str(path)))
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert list(sa) == list(sb) and any(v.dtype == torch.uint8 for v in sa.values())
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    lb = [k for k in sa if k.endswith("lora_B")]
    assert any(float(sa[k].float().abs().max()) > 0 for k in lb)  # the adapters moved
    batch = next(iter(SyntheticBridgeDataset(cfg(), 4, seed=9)))
    losses = []
    for ag in (a, b):
        torch.manual_seed(5)
        inputs = ag.preprocess_batch(batch)
        losses.append(ag.model(**inputs, noise=torch.zeros(inputs["actions"].shape, device="cuda")).item())
        ag.model.zero_grad(set_to_none=True)
    assert losses[0] == losses[1]
    _one_update(a, batch, 5)
    _one_update(b, batch, 5)
    sa, sb = a.model.state_dict(), b.model.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_refusals_by_name():
    from src.model.vla.pizero import PiZero

    d = O.TINY_DIMS
    with pytest.raises(ValueError, match="quantize_type"):
        PiZero(qlora_cfg(d, qtype="int8"), device="cuda", dtype=torch.bfloat16, init="none")
    cfg = qlora_cfg(d)
    cfg.vision.config.lora.dropout = 0.1
    with pytest.raises(NotImplementedError, match="lora_dropout"):
        PiZero(cfg, device="cuda", dtype=torch.bfloat16, init="none")
