"""Host side of the frozen-VLM training pass: the ABI surface of pz_expert_attn_fwd / pz_expert_attn_bwd,
their argument checks (which fail before any launch, so they run without a GPU), and the data-parallel wrapper leaving
a region in which nothing trains out of the all-reduce when the freeze happens after it was built (gloo, two ranks,
the tiny model's real arena layout, as tests/test_ddp_cpu.py)."""

import ctypes as C
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.conftest import ROOT

NEW = ("pz_expert_attn_fwd", "pz_expert_attn_bwd", "pz_expert_attn_bwd_ws_bytes")
PTR = 0x100000  # a 16-B aligned non-NULL address: the checks under test return before anything dereferences it


# ------------------------------------------------------------------------------------------------ ABI surface --
def test_abi_surface():
    import pizero_native
    from pizero_native import ops
    from pizero_native._lib import ABI_VERSION, SIGNATURES

    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    decl = set(re.findall(r"\b(pz_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    L = pizero_native.lib()
    for s in NEW:
        assert s in decl and s in SIGNATURES and hasattr(L, s), s
    assert "typedef struct pz_expert_attn_bwd_args" in hdr
    assert ABI_VERSION == 22 and "#define PZ_ABI_VERSION 22" in hdr and L.pz_abi_version() == 22
    assert callable(ops.expert_attn_fwd) and callable(ops.expert_attn_bwd)
    assert "pz_expert_attn.hip" in open(os.path.join(ROOT, "open-pi-zero_amd", "build_native.py")).read()


def test_bwd_ws_bytes():
    import pizero_native

    L = pizero_native.lib()
    # bridge, micro-batch 2: 9 chunks x 2 row tiles x 2 samples = 36 workgroups, one chunk each -> 9 dQ partials
    rpad, nkeys, B = 64, 5, 2
    want = (B * 9 * rpad * 256 + 2 * B * 2 * nkeys * 256) * 4
    assert L.pz_expert_attn_bwd_ws_bytes(B, 40, 281, nkeys) == want
    # micro-batch 256: 4608 (chunk, tile) pairs -> every workgroup walks all 9 chunks, one dQ partial
    assert L.pz_expert_attn_bwd_ws_bytes(256, 40, 281, nkeys) == (256 * rpad * 256 + 2 * 256 * 2 * nkeys * 256) * 4


# ------------------------------------------------------------------------------------------- argument checks --
def _fwd_args(**kw):
    from pizero_native._lib import DecodeAttnArgs

    a = DecodeAttnArgs()
    a.q = a.k = a.v = a.o = a.ws = PTR
    a.ldq, a.Lq, a.qoff, a.ldo = 2048, 5, 0, 2048
    a.k_bstride = a.v_bstride = 288 * 256
    a.B, a.nh, a.T, a.nk, a.head_dim = 2, 8, 5, 281, 256
    a.scale, a.cap = 1 / 16.0, 50.0
    a.prefix, a.cond, a.qtok0 = 276, 1, 276
    a.ws_bytes = 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bwd_args(**kw):
    from pizero_native._lib import ExpertAttnBwdArgs

    a = ExpertAttnBwdArgs()
    a.q = a.k = a.v = a.o = a.dO = a.lse = a.dq = a.dk = a.dv = a.ws = PTR
    a.ldq, a.Lq, a.qoff, a.ldo, a.lddo = 2048, 5, 0, 2048, 2048
    a.k_bstride = a.v_bstride = a.dk_bstride = a.dv_bstride = 288 * 256
    a.B, a.nh, a.T, a.nk, a.head_dim = 2, 8, 5, 281, 256
    a.scale, a.cap = 1 / 16.0, 50.0
    a.prefix, a.cond, a.qtok0, a.key0, a.nkeys = 276, 1, 276, 276, 5
    a.ws_bytes = 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refused(rc, msg):
    import pizero_native

    assert rc == 1, rc  # PZ_ERR_INVALID_ARG: returned by the checks, before any launch
    err = pizero_native.lib().pz_last_error()
    assert msg in err, err


@pytest.mark.parametrize("kw,msg", [
    (dict(T=129), b"1024 query rows"),  # E4 with H = 128: 1032 rows
    (dict(head_dim=32), b"head_dim 256"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(q=None), b"bad args"),
    (dict(ldq=2052), b"alignment"),
])
def test_fwd_argument_checks(kw, msg):
    import pizero_native

    _refused(pizero_native.lib().pz_expert_attn_fwd(C.byref(_fwd_args(**kw)), PTR, None), msg)


def test_fwd_needs_lse():
    import pizero_native

    _refused(pizero_native.lib().pz_expert_attn_fwd(C.byref(_fwd_args()), None, None), b"lse")


@pytest.mark.parametrize("kw,msg", [
    (dict(T=129, Lq=129), b"1024 query rows"),
    (dict(head_dim=32), b"head_dim 256"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(lse=None), b"bad args"),
    (dict(dk=None), b"bad args"),
    (dict(key0=280), b"key range"),  # [280, 285) leaves [0, 281)
    (dict(nkeys=0), b"key range"),
    (dict(qoff=1), b"outside Lq"),
    (dict(lddo=2052), b"alignment"),
])
def test_bwd_argument_checks(kw, msg):
    import pizero_native

    _refused(pizero_native.lib().pz_expert_attn_bwd(C.byref(_bwd_args(**kw)), None), msg)


# ------------------------------------------------------------------------------------------------------- DDP --
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _drive(red, m):
    """the engine's notifications of one backward, in order, then the flush"""
    nL = m.joint_model.num_hidden_layers
    vL = len(m.vision_tower.vision_model.encoder.layers)
    order = [("joint", l) for l in reversed(range(nL))] + [("encoders", -1)]
    order += [("vision", i) for i in reversed(range(vL))] + [("vision", -1)]
    launched = []
    orig = red._launch
    red._launch = lambda region, lo, hi, streams=(): (launched.append((region, lo, hi)), orig(region, lo, hi, streams))
    for st, l in order:
        red.notify(st, l)
    red.finish()
    red._launch = orig
    return launched


def _worker(rank, world, port, q):
    try:
        import sys

        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "open-pi-zero_amd"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from oracle.pizero_oracle import TINY_DIMS
        from pizero_native.ddp import GradReducer, PiZeroDDP, region_marks
        from src.model.vla.pizero import PiZero
        from tests.golden.make_golden import ref_cfg

        out = {}
        m = PiZero(ref_cfg(TINY_DIMS))
        m.tie_action_proprio_weights()
        m.freeze_unused_weights()
        ar = m._arena
        ddp = PiZeroDDP(m, bucket_bytes=4096)
        red = ddp.reducer
        # 1. a trainable VLM: the wrapper's buckets are the ones of a reducer built the way it always was
        out["skip_trainable"] = sorted(ddp.sync_regions())
        g = ar.ensure_grad()
        g.fill_(float(rank + 1))
        mine = _drive(red, m)
        log_ddp = list(red.log)
        plain = GradReducer(ar, region_marks(m), bucket_bytes=4096)
        g.fill_(float(rank + 1))
        theirs = _drive(plain, m)
        out["same_as_parent"] = mine == theirs and log_ddp == plain.log and len(mine) > 2
        # 2. TrainAgent's order: the VLM is frozen AFTER the wrapper was built
        for p in m.trainable_vlm_parameters:
            p.requires_grad = False
        out["skip_frozen"] = sorted(ddp.sync_regions())
        g.fill_(float(rank + 1))
        n0 = len(red.log)
        launched = _drive(red, m)
        lo_a, hi_a = ar.region_range["action"]
        lo_v, hi_v = ar.region_range["vlm"]
        out["regions"] = sorted({r for r, _, _ in launched})
        out["vlm_untouched"] = bool(torch.all(g[lo_v:hi_v] == rank + 1))
        out["action_reduced"] = bool(torch.allclose(g[lo_a:hi_a], torch.full_like(g[lo_a:hi_a], 1.5)))
        spans = sorted((lo, hi) for _, lo, hi in launched)
        out["action_cover"] = (spans[0][0] == lo_a and spans[-1][1] >= hi_a
                               and all(a[1] == b[0] for a, b in zip(spans, spans[1:])))
        out["no_vlm_element"] = all(hi <= lo_v or lo >= hi_v for _, lo, hi in launched)
        out["log_elements"] = sum(n for _, n in red.log[n0:]) == spans[-1][1] - lo_a
        # 3. thawed again: the region comes back
        for p in m.trainable_vlm_parameters:
            p.requires_grad = True
        m.freeze_unused_weights()
        out["skip_thawed"] = sorted(ddp.sync_regions())
        q.put((rank, out))
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, {"error": repr(e) + traceback.format_exc()}))


@pytest.mark.timeout(300)
def test_ddp_leaves_a_region_frozen_after_wrapping_out_of_the_all_reduce():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=240) for _ in ps]
    for p in ps:
        p.join(timeout=60)
    for rank, out in res:
        assert "error" not in out, out
        assert out["skip_trainable"] == [] and out["same_as_parent"], out
        assert out["skip_frozen"] == ["vlm"] and out["regions"] == ["action"], out
        assert out["vlm_untouched"] and out["action_reduced"] and out["action_cover"] and out["no_vlm_element"], out
        assert out["log_elements"] and out["skip_thawed"] == [], out
