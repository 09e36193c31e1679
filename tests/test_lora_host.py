"""LoRA model surface on the host (no GPU): reference state_dict keys / shapes, the freeze selections, init,
the two refused settings, a strict state_dict round trip, arena adjacency of the fused sites, and the ABI version."""

import math
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.golden.make_golden_lora import RANK, lora_cfg
from tests.oracle_helpers import O


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "lora.npz"))


def build(d, init="default", cfg=None):
    from src.model.vla.pizero import PiZero

    m = PiZero(cfg if cfg is not None else lora_cfg(d), init=init)
    m.tie_action_proprio_weights()
    m.freeze_unused_weights()
    m.freeze_non_lora_weights_in_vlm()
    return m


@pytest.fixture(scope="module")
def model():
    return build(O.TINY_DIMS)


def test_state_dict_names_and_shapes_equal_the_reference(model, g):
    sd = model.state_dict()
    ref = {str(n): tuple(int(x) for x in str(s).split(",")) for n, s in zip(g["sd_names"], g["sd_shapes"])}
    assert list(sd.keys()) == list(ref.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    assert sum("lora_" in k for k in sd) > 0


def test_requires_grad_set_equals_the_reference(model, g):
    mine = [n for n, p in model.named_parameters() if p.requires_grad]
    assert mine == [str(n) for n in g["trainable"]]


def test_lora_trainable_vlm_parameters(model):
    d = O.TINY_DIMS
    named = dict(model.named_parameters())
    ids = {id(p) for p in model.lora_trainable_vlm_parameters}
    last = d["n_layers"] - 1
    for n, p in named.items():
        lora_vlm = "lora_" in n and ("vision_tower" in n or "multi_modal_projector" in n or ".mixtures.vlm." in n)
        unused = (".mixtures.vlm." in n and any(k in n for k in (f"{last}.post", f"{last}.mlp", f"{last}.self_attn.o_proj",
                                                                f"{last}.self_attn.v_proj")))
        assert (id(p) in ids) == (lora_vlm and not unused), n
        if lora_vlm and unused:
            assert not p.requires_grad, n  # frozen through freeze_unused_weights
    assert all(p.requires_grad for p in model.lora_trainable_vlm_parameters)
    assert {id(p) for p in model.trainable_lora_gemma_parameters} <= ids
    assert not any(id(p) in ids for p in model.action_expert_parameters)


def test_default_init(model):
    n_b = 0
    for n, p in model.state_dict().items():
        if n.endswith("lora_B"):
            assert float(p.abs().max()) == 0.0, n
            n_b += 1
        elif n.endswith("lora_A"):
            bound = 1.0 / math.sqrt(p.shape[1])  # kaiming_uniform(a=sqrt(5)) on [r, in]
            assert p.shape[0] == RANK and 0.5 * bound < float(p.abs().max()) <= bound, (n, float(p.abs().max()), bound)
    assert n_b > 0


def test_quantize_and_dropout_are_refused_by_name():
    from src.model.vla.pizero import PiZero

    d = O.TINY_DIMS
    cfg = lora_cfg(d)
    cfg.vision.use_quantize = True
    with pytest.raises(NotImplementedError, match="quantize"):
        PiZero(cfg, init="none")
    cfg = lora_cfg(d)
    cfg.joint.config.lora.dropout = 0.05
    with pytest.raises(NotImplementedError, match="lora_dropout"):
        PiZero(cfg, init="none")
    cfg = lora_cfg(d)
    cfg.vision.config.lora.dropout = 0.05
    with pytest.raises(NotImplementedError, match="lora_dropout"):
        PiZero(cfg, init="none")


def test_state_dict_round_trip_strict(model):
    d = O.TINY_DIMS
    sd = {k: torch.randn_like(v) for k, v in model.state_dict().items()}
    for k in sd:  # tied: the proprio keys are the action tensors
        if ".mixtures.proprio." in k:
            sd[k] = sd[k.replace(".mixtures.proprio.", ".mixtures.action.")]
    m2 = build(d, init="none")
    m2.load_state_dict(sd, strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_arena_adjacency_of_fused_sites(model):
    ar = model._arena
    d = O.TINY_DIMS
    r = RANK
    assert ar.slots["joint_model.mixtures.vlm.layers.0.mlp.gate_proj.lora_A"].region == "lora"
    for p, projs, outs in (
            ("joint_model.mixtures.vlm.layers.1.self_attn.", ["q_proj", "k_proj", "v_proj"],
             [d["n_heads"] * d["head_dim"], d["head_dim"], d["head_dim"]]),
            ("joint_model.mixtures.vlm.layers.1.mlp.", ["gate_proj", "up_proj"], [d["vlm_inter"]] * 2),
            ("vision_tower.vision_model.encoder.layers.0.self_attn.", ["q_proj", "k_proj", "v_proj"], [d["vis_hidden"]] * 3)):
        A = ar.span(p + projs[0] + ".lora_A", p + projs[-1] + ".lora_A")
        B = ar.span(p + projs[0] + ".lora_B", p + projs[-1] + ".lora_B")
        assert A.shape[0] == len(projs) * r and B.shape == (sum(outs), r)
        for i, pr in enumerate(projs):
            a = ar.view(p + pr + ".lora_A")
            assert A[i * r:(i + 1) * r].data_ptr() == a.data_ptr() and A.shape[1] == a.shape[1]
            assert B[sum(outs[:i]):sum(outs[:i + 1])].data_ptr() == ar.view(p + pr + ".lora_B").data_ptr()
        # the base weights keep their fused span
        W = ar.span(p + projs[0] + ".weight", p + projs[-1] + ".weight")
        assert W.shape[0] == sum(outs)
    # every trainable adapter sits in the one "lora" region: one optimizer run per gap left by frozen adapters
    lo, hi = ar.region_range["lora"]
    for n, p_ in model.named_parameters():
        if "lora_" in n:
            assert lo <= ar.slots[n].offset < hi, n
    from pizero_native.optim import contiguous_runs

    assert len(list(contiguous_runs(model.lora_trainable_vlm_parameters))) <= 3


def test_plain_model_has_no_lora_region():
    from src.model.vla.pizero import PiZero
    from tests.golden.make_golden import ref_cfg

    m = PiZero(ref_cfg(O.TINY_DIMS), init="none")
    assert not m.has_lora and not any("lora_" in k for k in m.state_dict())
    assert m.lora_trainable_vlm_parameters == []


def test_abi_version_22():
    import pizero_native
    from pizero_native._lib import ABI_VERSION

    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    assert ABI_VERSION == 22 and "#define PZ_ABI_VERSION 22" in hdr
    L = pizero_native.lib()
    assert L.pz_abi_version() == 22
    assert L.pz_lora_wgrad_ws_bytes(4104, 256, 32) == 17 * 32 * 256 * 4
