"""Host-side surface of the adaLN / adaLN-Zero action expert (CPU only: no kernels are launched)."""

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.golden.make_golden import ref_cfg
from tests.golden.make_golden_adaln import ADALN_KEYS, FIXTURE, adaptive_cfg
from tests.oracle_helpers import O

MODES = ("adaLN", "adaLN-Zero")


def fixture(mode):
    import os

    return np.load(os.path.join(ROOT, "tests", "golden", FIXTURE[mode] + ".npz"))


def build(mode, tied, init="default"):
    from src.model.vla.pizero import PiZero

    m = PiZero(adaptive_cfg(O.TINY_DIMS, mode), init=init)
    if tied:
        m.tie_action_proprio_weights()
    m.freeze_unused_weights()
    return m


@pytest.fixture(scope="module", params=MODES)
def tied_model(request):
    return request.param, build(request.param, True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tied", (True, False))
def test_constructs(mode, tied):
    m = build(mode, tied, init="none")
    assert m.action_expert_adaptive_mode == mode
    assert m.time_embedding.half_dim == 128  # time_hidden_size 256, not the expert width
    assert not m.action_encoder.time_cond
    aH = O.TINY_DIMS["act_hidden"]
    assert tuple(m.action_encoder.linear_2.weight.shape) == (aH, aH)
    # untied: the proprio mixture carries its own modulation block
    n = sum(1 for k in m.state_dict() if "mixtures.proprio." in k and any(a in k for a in ADALN_KEYS))
    assert n > 0
    a = m.joint_model.mixtures["action"].norm.to_beta.weight
    p = m.joint_model.mixtures["proprio"].norm.to_beta.weight
    assert (a is p) == tied


def test_state_dict_matches_reference(tied_model):
    mode, m = tied_model
    f = fixture(mode)
    want = {str(n): tuple(int(x) for x in str(s).split(",")) for n, s in zip(f["sd_names"], f["sd_shapes"])}
    sd = m.state_dict()
    assert set(sd) == set(want), set(sd) ^ set(want)
    for k, v in sd.items():
        assert tuple(v.shape) == want[k], k
    assert bool(f["fp32/cached_infer_raises"])


def test_gemma_norm_weights_of_the_expert_are_absent(tied_model):
    mode, m = tied_model
    sd = m.state_dict()
    for k in sd:
        if "mixtures.action." in k or "mixtures.proprio." in k:
            assert not k.endswith("layernorm.weight") and not k.endswith("norm.weight"), k
    assert "joint_model.mixtures.vlm.layers.0.input_layernorm.weight" in sd
    zero = [k for k in sd if "to_adaln_zero_gamma" in k]
    assert bool(zero) == (mode == "adaLN-Zero")


def test_default_init(tied_model):
    mode, m = tied_model
    sd = m.state_dict()
    for k, v in sd.items():
        if "to_adaln_zero_gamma.weight" in k:
            assert float(v.abs().max()) == 0.0, k
        elif "to_adaln_zero_gamma.bias" in k:
            assert bool((v == -2.0).all()), k
        elif "to_gamma.0.weight" in k or "to_beta.weight" in k:
            bound = 1.0 / np.sqrt(v.shape[1])
            assert 0.0 < float(v.abs().max()) <= bound, k


def test_action_expert_parameters_cover_new_tensors_once(tied_model):
    mode, m = tied_model
    new = {n: p for n, p in m.named_parameters() if any(a in n for a in ADALN_KEYS)}
    assert new
    ptrs = [p.data_ptr() for p in m.action_expert_parameters]
    assert len(ptrs) == len(set(ptrs))
    for n, p in new.items():
        assert ptrs.count(p.data_ptr()) == 1, n
        assert p.requires_grad, n


def test_modulation_block_is_adjacent(tied_model):
    """the arena lays a mixture's time-conditioning Linears out as one [nslots * hidden, time_hidden] matrix"""
    from src.model.vla.pizero import adaln_slots

    mode, m = tied_model
    d = O.TINY_DIMS
    sl = adaln_slots("joint_model.mixtures.action.", d["n_layers"], mode)
    per_layer = 6 if mode == "adaLN-Zero" else 4
    assert len(sl["w"]) == per_layer * d["n_layers"] + 2 and len(set(sl["slot"].values())) == len(sl["w"])
    W = m._arena.span(sl["w"][0], sl["w"][-1])
    assert tuple(W.shape) == (len(sl["w"]) * d["act_hidden"], 256)
    assert torch.equal(W, torch.cat([m._arena.view(n) for n in sl["w"]], 0))
    b = m._arena.span(sl["b"][0], sl["b"][-1])
    assert torch.equal(b, torch.cat([m._arena.view(n) for n in sl["b"]], 0))
    # the block follows the expert's layer 0 in the backward-completion order and precedes the encoders
    order = m._arena.order
    assert order.index("joint_model.mixtures.action.layers.0.self_attn.v_proj.weight") < order.index(sl["w"][0])
    assert order.index(sl["b"][-1]) < order.index("action_encoder.linear_3.weight")
    assert all(m._arena.slots[n].region == "action" for n in sl["w"] + sl["b"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tied", (True, False))
def test_ddp_marks_keep_the_modulation_block_for_the_encoders_notification(mode, tied):
    """The data-parallel reducer treats the arena prefix up to marks[(stage, layer)] as final.  A layer's
    conditioning Linears live in the modulation block after expert layer 0 and get their gradients only after the
    joint backward: no ("joint", l) mark may reach the block, nor the weights of a layer that has not run yet."""
    from pizero_native.ddp import region_marks
    from src.model.vla.pizero import adaln_slots

    m = build(mode, tied, init="none")
    ar = m._arena
    nL = O.TINY_DIMS["n_layers"]
    marks = region_marks(m)
    block = []
    for mix in ("action",) if tied else ("action", "proprio"):
        sl = adaln_slots(f"joint_model.mixtures.{mix}.", nL, mode)
        block += sl["w"] + sl["b"]
    block_start = min(ar.slots[n].offset for n in block)
    block_end = max(ar.slots[n].offset + ar.slots[n].numel for n in block)

    def layer_names(l):
        return [n for n in ar.order if n not in block and any(
            n.startswith(f"joint_model.mixtures.{mix}.layers.{l}.") for mix in ("action", "proprio"))]

    prev = 0
    for l in reversed(range(nL)):
        end = marks[("joint", l)]["action"]
        own = layer_names(l)
        assert end == max(ar.slots[n].offset + ar.slots[n].numel for n in own), l  # exactly this layer's weights
        limit = min(ar.slots[n].offset for n in layer_names(l - 1)) if l > 0 else block_start
        assert prev < end <= limit, (l, end, limit)
        prev = end
    assert marks[("encoders", -1)]["action"] >= block_end


def test_default_mode_ddp_marks_unchanged():
    from pizero_native.ddp import region_marks
    from src.model.vla.pizero import PiZero

    m = PiZero(ref_cfg(O.TINY_DIMS), init="none")
    m.tie_action_proprio_weights()
    ar = m._arena
    marks = region_marks(m)
    for l in range(O.TINY_DIMS["n_layers"]):
        p = f"joint_model.mixtures.action.layers.{l}."
        last = ar.slots[p + "input_layernorm.weight"]
        assert marks[("joint", l)]["action"] == last.offset + last.numel


def test_reference_checkpoint_loads_strict_and_default_checkpoint_fails(tied_model):
    from src.model.vla.pizero import PiZero

    mode, m = tied_model
    f = fixture(mode)
    g = torch.Generator().manual_seed(1)
    ck = {str(n): torch.rand([int(x) for x in str(s).split(",")], generator=g)
          for n, s in zip(f["sd_names"], f["sd_shapes"])}
    m.load_state_dict(ck, strict=True)
    k = "joint_model.mixtures.action.layers.1.input_layernorm.to_gamma.0.bias"
    assert torch.equal(m.state_dict()[k], ck[k])
    default = PiZero(ref_cfg(O.TINY_DIMS), init="none")
    default.tie_action_proprio_weights()
    with pytest.raises(RuntimeError, match="Missing key|size mismatch"):
        m.load_state_dict(default.state_dict(), strict=True)


def test_default_mode_key_set_is_unchanged():
    from src.model.vla.pizero import PiZero

    m = PiZero(ref_cfg(O.TINY_DIMS), init="none")
    m.tie_action_proprio_weights()
    assert set(m.state_dict()) == set(O.param_shapes(O.TINY_DIMS))
    assert m.time_embedding.half_dim == O.TINY_DIMS["act_hidden"] // 2 and m.action_encoder.time_cond


def test_mismatched_mixture_mode_is_rejected():
    from src.model.vla.pizero import PiZero

    cfg = adaptive_cfg(O.TINY_DIMS, "adaLN")
    cfg.mixture.proprio.adaptive_mode = None
    cfg.joint.config.mixture.proprio.adaptive_mode = None
    with pytest.raises(ValueError, match="adaptive_mode"):
        PiZero(cfg, init="none")
