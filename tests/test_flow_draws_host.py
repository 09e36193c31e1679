"""Host side of several flow draws per observation (flow_samples_per_observation): the ABI surface of
pz_expert_attn_fwd_shared / pz_expert_attn_bwd_shared and their argument checks (which fail before any launch, so they
run without a GPU), the reference statement tests/draws_ref.py at S = 1 against the oracle, and the shape validation
of PiZero.forward's t / noise / prefix_len, which runs without a device."""

import ctypes as C
import os
import re

import pytest
import torch

from tests.conftest import ROOT
from tests.test_frozen_vlm_host import PTR, _bwd_args, _fwd_args, _refused

NEW = ("pz_expert_attn_fwd_shared", "pz_expert_attn_bwd_shared")


def test_abi_surface():
    import pizero_native
    from pizero_native import ops
    from pizero_native._lib import ABI_VERSION, SIGNATURES

    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    decl = set(re.findall(r"\b(pz_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    L = pizero_native.lib()
    for s in NEW:
        assert s in decl and s in SIGNATURES and hasattr(L, s), s
    assert len(SIGNATURES["pz_expert_attn_fwd_shared"]) == 7 and len(SIGNATURES["pz_expert_attn_bwd_shared"]) == 6
    assert ABI_VERSION == 22 and "#define PZ_ABI_VERSION 22" in hdr and L.pz_abi_version() == 22
    assert callable(ops.expert_attn_fwd_shared) and callable(ops.expert_attn_bwd_shared)


# own buffers of the bridge geometry: 5 own keys per pair, 2 pairs per observation
OWN = dict(k_own=PTR, v_own=PTR, own_bstride=5 * 256, kv_group=2)


@pytest.mark.parametrize("own,kw,msg", [
    (dict(kv_group=0), {}, b"kv_group must be >= 1"),
    (dict(kv_group=-2), {}, b"kv_group must be >= 1"),
    (dict(kv_group=3), dict(B=4), b"multiple of kv_group"),
    ({}, dict(prefix=282), b"prefix must lie in [0, nk]"),
    (dict(k_own=None), {}, b"k_own / v_own"),
    (dict(own_bstride=4 * 256), {}, b"own_bstride"),
    ({}, dict(T=129), b"1024 query rows"),
    ({}, dict(head_dim=32), b"head_dim 256"),
])
def test_shared_argument_checks(own, kw, msg):
    import pizero_native

    o = {**OWN, **own}
    L = pizero_native.lib()
    _refused(L.pz_expert_attn_fwd_shared(C.byref(_fwd_args(**kw)), o["k_own"], o["v_own"], o["own_bstride"], o["kv_group"],
                                         PTR, None), msg)
    kb = dict(kw, Lq=129) if kw.get("T") == 129 else kw
    _refused(L.pz_expert_attn_bwd_shared(C.byref(_bwd_args(**kb)), o["k_own"], o["v_own"], o["own_bstride"],
                                         o["kv_group"], None), msg)


def test_draws_ref_at_one_draw_is_the_oracle():
    """S = 1: the replicated batch is the fixture's, so loss and every gradient are oracle_run's bit for bit"""
    from tests.draws_ref import draws_run
    from tests.oracle_helpers import O, oracle_run

    d = O.TINY_DIMS
    want, inp = oracle_run(d, 3, ragged=True)
    got, _ = draws_run(d, 3, 1)
    assert got["loss"] == want["loss"]
    assert got["t"].shape == (3, 1) and (got["t"][:, 0] == inp["t"]).all() and (got["x0"][:, 0] == inp["x0"]).all()
    assert set(got["grads"]) == set(want["grads"])
    for n, w in want["grads"].items():
        g = got["grads"][n]
        assert (g is None) == (w is None), n
        if w is not None:
            assert torch.equal(g, w), n


def test_draws_ref_draws_are_distinct():
    from oracle.synth import synth_inputs
    from tests.draws_ref import draws
    from tests.oracle_helpers import O

    t, x0 = draws(synth_inputs(O.TINY_DIMS, 3, seed=0, ragged=True), 3)
    assert t.shape == (3, 3) and x0.shape[:2] == (3, 3)
    for s in range(3):
        for r in range(s + 1, 3):
            assert (t[:, s] != t[:, r]).all() and (x0[:, s] != x0[:, r]).any()


def test_forward_shape_validation_runs_without_a_device():
    from src.model.vla.pizero import flow_draws

    B, H, A = 4, 5, 7
    assert flow_draws(B, H, A, (B,)) == 1
    assert flow_draws(B, H, A, (B,), (B, H, A), (B,)) == 1
    assert flow_draws(B, H, A, (B, 1), (B, 1, H, A)) == 1
    assert flow_draws(B, H, A, (B, 3)) == 3
    assert flow_draws(B, H, A, (B, 3), (B, 3, H, A), (B,)) == 3
    assert flow_draws(B, H, A, (B, 3), (B, 3, H, A), (B, 3)) == 3
    key = "flow_samples_per_observation"
    for args in (((B, 3), (B, 2, H, A)),      # noise for another S
                 ((B, 3), (B, H, A)),         # noise without the draw axis
                 ((B,), (B, 3, H, A)),        # t without the draw axis
                 ((B, 3), None, (B, 2)),      # prefix_len for another S
                 ((B,), None, (B, 2)),
                 ((B, 0),), ((B + 1, 3),), ((B, 3, 1),)):
        with pytest.raises(ValueError, match=key):
            flow_draws(B, H, A, *args)
