"""Inference-time guidance toward the previous chunk end to end on the MI355X, tiny model, B = 3 ragged,
beta = 5, (delay, overlap) in {(1, 4), (1, 3), (2, 4), (0, 4)}.

No reference exists for this feature: the pin is tests/rtc_ref.py, the guided loop composed from the CPU oracle's
pieces with torch.autograd.grad as the vector-Jacobian product (it equals the oracle bit for bit with W = 0 and agrees
with fp64 central differences, tests/test_rtc_host.py).  Parity bound, the rule of tests/test_prefix_gpu.py: max |err|
<= max(3 dev, 3e-2), dev = the restatement's own bf16-autocast deviation from its fp32 run.  The bound discriminates:
guidance moves the chunk by more than 10 x the bound, and the restatement without the Jacobian term lies more than
3 x the bound from the full one, so a backward that returns nothing (or garbage) cannot pass.
"""

import json
import os

import numpy as np
import pytest
import torch

from tests import rtc_ref as R
from tests.conftest import ROOT
from tests.golden.make_golden import ref_cfg
from tests.oracle_helpers import O
from tests.pizero_gpu_helpers import GRAD_COS, GRAD_REL, build_gpu_model, gpu_inputs

pytestmark = pytest.mark.gpu

D = O.TINY_DIMS
B = 3
BETA = 5.0
CASES = [(1, 4), (1, 3), (2, 4), (0, 4)]
FLOOR = 3e-2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tables(delay, overlap):
    from src.agent.chunking import guidance_coef, soft_mask

    w = np.tile(soft_mask(D["horizon_steps"], delay, overlap)[None], (B, 1))
    return w, guidance_coef(D["num_inference_steps"], BETA)


@pytest.fixture(scope="module")
def tiny():
    m = build_gpu_model(D)
    return m, gpu_inputs(m, D, B)


@pytest.fixture(scope="module")
def ref():
    """the restatement on the fixture inputs, target = the fixture's actions: per case the fp32 chunk, its bf16
    deviation and the bound; the unguided oracle chunk; for (1, 4) the chunk without the Jacobian term.  Computed once,
    shared, never modified."""
    W, inp, args = R.fixture(D, B, ragged=True)
    target = inp["actions"]
    out = {"target": target, "inp": inp}
    with torch.no_grad():
        out["plain"] = O.pizero_infer(W, D, *args, clip=False)
    for case in CASES:
        w, coef = _tables(*case)
        r32, _ = R.restatement_run(D, B, target, w, coef)
        r16, _ = R.restatement_run(D, B, target, w, coef, bf16=True)
        dev = (r16 - r32).abs().max().item()
        out[case] = dict(a=r32, dev=dev, tol=max(3 * dev, FLOOR), w=w, coef=coef)
    w, coef = _tables(1, 4)
    out["nojac"], _ = R.restatement_run(D, B, target, w, coef, jacobian=False)
    return out


def _infer(m, g, guide=None, clip=False):
    kw = {} if guide is None else dict(guide=guide)
    a = m.infer_action(input_ids=g["input_ids"], pixel_values=g["pixel_values"].float(),
                       image_text_proprio_mask=g["itp"], action_mask=g["amask"], vlm_position_ids=g["vpos"],
                       proprio_position_ids=g["ppos"], action_position_ids=g["apos"], proprios=g["proprios"],
                       noise=g["noise"], clip=clip, **kw)
    torch.cuda.synchronize()
    return a.float().cpu()


@pytest.mark.parametrize("case", CASES)
def test_guided_chunk_matches_the_restatement(tiny, ref, case):
    m, g = tiny
    r = ref[case]
    a = _infer(m, g, (ref["target"], r["w"], r["coef"]))
    err = (a - r["a"]).abs().max().item()
    moved = (r["a"] - ref["plain"]).abs().max().item()
    print(f"{case}: max |gpu - restatement| {err:.4f}, bound {r['tol']:.4f} (bf16 deviation {r['dev']:.4f}); "
          f"guided vs unguided {moved:.3f}")
    assert moved > 10 * r["tol"], "the case does not discriminate: guidance barely moves the chunk"
    assert err <= r["tol"]
    delay = case[0]
    if delay:  # the W = 1 rows land on the target
        tgt = torch.from_numpy(ref["target"])[:, :delay]
        near, far = (a[:, :delay] - tgt).abs().mean().item(), (ref["plain"][:, :delay] - tgt).abs().mean().item()
        print(f"{case}: mean |a - Y| on the W = 1 rows: guided {near:.4f}, unguided {far:.4f}")
        assert near < 0.25 * far


def test_the_jacobian_term_is_visible(ref):
    """the restatement without the Jacobian term differs from the full one by more than 3 x the bound"""
    r = ref[(1, 4)]
    gap = (ref["nojac"] - r["a"]).abs().max().item()
    print(f"max |no Jacobian - full| {gap:.4f}, bound {r['tol']:.4f}")
    assert gap > 3 * r["tol"]


def test_vjp_of_one_step(tiny, ref):
    """dA of step 0 (A_0 = the noise, t = 0) against the restatement's torch.autograd.grad"""
    m, g = tiny
    r = ref[(1, 4)]
    eng = m._engine()
    seen = []
    orig = eng.denoise_step_guided

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append(out.float().cpu())
        return out

    eng.denoise_step_guided = spy
    try:
        _infer(m, g, (ref["target"], r["w"], r["coef"]))
    finally:
        del eng.denoise_step_guided
    assert len(seen) == D["num_inference_steps"]
    W, inp, args = R.fixture(D, B, ragged=True)
    ids, pix, itp, amask, vpos, ppos, apos, prop, noise = args
    with torch.no_grad():
        emb = O.embed_siglip_and_text(W, D, ids, pix)
        pe = O.linear(prop, W, "proprio_encoder")
        _, cache = O.joint_forward(W, D, {"vlm": emb, "proprio": pe}, {"vlm": vpos, "proprio": ppos}, itp,
                                   return_cache=True)
    _, _, _, dA = R.guided_step(W, D, noise, torch.zeros(B), cache, apos, amask, torch.from_numpy(ref["target"]),
                                torch.from_numpy(r["w"]), float(r["coef"][0]), 0.1)
    got = seen[0][:, : D["action_dim"]].reshape(dA.shape).double()
    want = dA.double()
    rel = ((got - want).norm() / want.norm()).item()
    cos = ((got * want).sum() / (got.norm() * want.norm())).item()
    print(f"dA of step 0: rel-L2 {rel:.4f} (<= {GRAD_REL}), cosine {cos:.5f} (>= {GRAD_COS}), |dA| {want.norm():.3f}")
    assert want.norm() > 1e-2 and rel <= GRAD_REL and cos >= GRAD_COS


def test_zero_weight_is_the_unguided_chunk(tiny, ref):
    m, g = tiny
    r = ref[(1, 4)]
    a = _infer(m, g, (ref["target"], np.zeros_like(r["w"]), r["coef"]))
    plain = _infer(m, g)
    err = (a - plain).abs().max().item()
    print(f"W = 0: max |guided - infer_action| {err:.5f}; vs the oracle {(a - ref['plain']).abs().max().item():.5f}")
    assert err <= r["tol"] and (a - ref["plain"]).abs().max().item() <= r["tol"]


def test_forced_onto_linear_dgrad(tiny, ref):
    """the guided loop with every few-row input gradient on ops.linear_dgrad: the same chunk within the bound"""
    from pizero_native import ops

    m, g = tiny
    r = ref[(1, 4)]
    eng = m._engine()
    guide = (ref["target"], r["w"], r["coef"])
    calls, orig = [], ops.linear_dgrad_rows

    def spy(*a, **k):
        calls.append(orig(*a, **k))
        return calls[-1]

    ops.linear_dgrad_rows = spy
    try:
        new = _infer(m, g, guide)
        taken = list(calls)
        eng.dgrad_rows = False
        old = _infer(m, g, guide)
    finally:
        eng.dgrad_rows = True
        ops.linear_dgrad_rows = orig
    # the engine takes the kernel for W [N, K] with N < K (where it measured faster): per step and layer down_proj
    # and o_proj, per step the action encoder's linear_2
    assert len(taken) == D["num_inference_steps"] * (2 * D["n_layers"] + 1) and all(taken)
    assert len(calls) == len(taken), "the forced run still called pz_dgrad_rows"
    print(f"max |pz_dgrad_rows - pz_gemm| {(new - old).abs().max().item():.5f}; "
          f"forced vs restatement {(old - r['a']).abs().max().item():.4f}")
    assert (old - r["a"]).abs().max().item() <= r["tol"] and (new - old).abs().max().item() <= r["tol"]


def test_unguided_calls_keep_their_bits(tiny, ref):
    """a model that has run the guided loop returns, for calls without a guide, the bits of one that never did"""
    m, g = tiny
    r = ref[(1, 4)]
    _infer(m, g, (ref["target"], r["w"], r["coef"]))
    after = _infer(m, g)
    fresh = _infer(build_gpu_model(D), g)
    assert torch.equal(after.view(torch.int32), fresh.view(torch.int32))


def test_clip_covers_every_row(tiny, ref):
    m, g = tiny
    r = ref[(1, 4)]
    big = ref["target"] * 3.0  # pulls the W = 1 row well past the clip value
    a = _infer(m, g, (big, r["w"], r["coef"]), clip=True)
    c = D["final_action_clip_value"]
    assert a.abs().max().item() <= c and (a.abs() == c).any()


def test_refusals(tiny, ref):
    from pizero_native.engine import GUIDE_FP8_MSG, GUIDE_PREFIX_MSG, GeneralMask

    m, g = tiny
    r = ref[(1, 4)]
    guide = (ref["target"], r["w"], r["coef"])
    with pytest.raises(NotImplementedError, match="action_guidance_beta"):
        m.infer_action_naive(input_ids=g["input_ids"], pixel_values=g["pixel_values"].float(),
                             causal_mask=g["causal_mask"], vlm_position_ids=g["vpos"], proprio_position_ids=g["ppos"],
                             action_position_ids=g["apos"], proprios=g["proprios"], noise=g["noise"], guide=guide)
    eng = m._engine()
    dev_guide = tuple(torch.as_tensor(x).cuda().float().contiguous() for x in guide)
    with pytest.raises(NotImplementedError, match="prefix_len"):
        eng._guide_args(dev_guide, B, None, torch.zeros(B, dtype=torch.int32, device="cuda"))
    with pytest.raises(NotImplementedError, match="GeneralMask"):
        eng._guide_args(dev_guide, B, GeneralMask(), None)
    eng.f8 = {}
    try:
        with pytest.raises(NotImplementedError, match="fp8"):
            eng._guide_args(dev_guide, B, None, None)
    finally:
        eng.f8 = None
    with pytest.raises(ValueError, match="guide w"):
        eng._guide_args((dev_guide[0], dev_guide[1][:, :2].contiguous(), dev_guide[2]), B, None, None)
    assert "action_guidance_beta" in GUIDE_FP8_MSG and "prefix_len" in GUIDE_PREFIX_MSG


# ------------------------------------------------------------------------------------------------- the graph --
def _graph_args(m, g):
    return (g["input_ids"], g["pixel_values"], m.block_prefix_counts(g["itp"], g["amask"]), g["vpos"], g["ppos"],
            g["apos"], g["proprios"].float(), g["noise"])


def test_graph_replay_is_the_eager_run_and_serves_any_guide(tiny, ref):
    from pizero_native.graph import InferenceGraph
    from src.agent.chunking import guidance_coef, soft_mask

    m, g = tiny
    ig = InferenceGraph(m, B, clip=True).enable_guidance()
    r = ref[(1, 4)]
    H = D["horizon_steps"]
    w2 = np.stack([soft_mask(H, dl, 3) for dl in (0, 2, 3)])  # another delay per sample, overlap 3, beta 2
    loads = [(ref["target"], r["w"], r["coef"]),
             (ref["target"][::-1] * 0.5, w2, guidance_coef(D["num_inference_steps"], 2.0))]
    captured = None
    for target, w, coef in loads:
        target = np.ascontiguousarray(target)
        ig.load(*_graph_args(m, g), guide_target=torch.from_numpy(target), guide_w=torch.from_numpy(w),
                guide_coef=torch.from_numpy(coef))
        if captured is None:
            ig.capture()
            captured = ig.graph
        a = ig.replay().float().cpu()
        torch.cuda.synchronize()
        eager = _infer(m, g, (target, w, coef), clip=True)
        assert torch.equal(a.view(torch.int32), eager.view(torch.int32))
    assert ig.graph is captured
    assert not torch.equal(a, _infer(m, g, clip=True))
    with pytest.raises(ValueError, match="go together"):
        ig.load(*_graph_args(m, g), guide_w=torch.from_numpy(w2))
    with pytest.raises(NotImplementedError, match="prefix_len"):
        ig.enable_prefix()
    with pytest.raises(ValueError, match="enable_guidance"):
        InferenceGraph(m, B).load(*_graph_args(m, g), guide_target=torch.from_numpy(target),
                                  guide_w=torch.from_numpy(w), guide_coef=torch.from_numpy(coef))


# --------------------------------------------------------------------------------------------- EvalAgent.act --
def _bridge_stats():
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")))
    s["proprio"]["mean"] = [0.0] * 7
    s["proprio"]["std"] = [1.0 - 1e-8] * 7  # (x - 0) / (std + 1e-8): the identity
    return s


@pytest.mark.parametrize("use_graph", [True, False])
def test_act_with_overlap(tmp_path, use_graph):
    """rows < delay of act's output are prev_actions' bits, the clamp covers the other rows only, the rest is the
    guided infer_action on the normalised target followed by the denormalisation; another (delay, overlap, beta)
    replays the same capture; calls without overlap keep their graph and their bits"""
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.agent.chunking import guidance_coef, soft_mask
    from src.agent.eval import EvalAgent
    from src.agent.train import SyntheticBridgeDataset

    p = tmp_path / "stats.json"
    p.write_text(json.dumps(_bridge_stats()))
    c = ref_cfg(D)
    c.update(dict(use_bf16=True, load_pretrained_weights=False))
    c["env"] = dict(adapter=dict(dataset_statistics_path=str(p), proprio_normalization_type="gaussian",
                                 action_normalization_type="bound"))
    ag = EvalAgent(c, use_graph=use_graph)
    for name in ag.model._arena.order:
        v = ag.model._arena.view(name)
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    torch.cuda.synchronize()
    m = ag.model
    Bn, H, A = 2, 4, 7
    b = next(iter(SyntheticBridgeDataset(c, Bn, seed=3)))
    noise = torch.randn(Bn, H, A, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    st = _bridge_stats()["action"]
    sa, sb = (torch.tensor(st[k], dtype=torch.float64).float().cuda() for k in ("p01", "p99"))
    rng = np.random.default_rng(7)
    lo, hi = np.array(st["p01"]), np.array(st["p99"])
    prev = torch.from_numpy(lo + (hi - lo) * rng.uniform(-0.2, 1.2, (Bn, H, A))).float()  # some beyond [p01, p99]
    obs = (b["pixel_values"], b["input_ids"], b["attention_mask"], b["proprio"])
    plain = ag.act(*obs, noise=noise, channels_last=False).clone()
    hard = ag.act(*obs, noise=noise, channels_last=False, prev_actions=prev, delay=1).clone()
    plain_graph = ag.observation_graph(Bn, (56, 56), channels_last=False).graph
    n_graphs = len(ag._obs_graphs)
    mask, vpos, ppos, apos = m.build_causal_mask_and_position_ids(b["attention_mask"].cuda(), torch.bfloat16)
    itp, amask = m.split_full_mask_into_submasks(mask)
    pix = ((b["pixel_values"].float() / 255 - 0.5) / 0.5).to(torch.bfloat16)
    clipv = D["final_action_clip_value"]
    first = None
    for delay, overlap, beta in (([1, 2], 4, None), (1, 3, 2.0), (0, 4, None)):
        out = ag.act(*obs, noise=noise, channels_last=False, prev_actions=prev, delay=delay, overlap=overlap,
                     guidance_beta=beta).clone()
        g = ag.observation_graph(Bn, (56, 56), channels_last=False, guidance=True)
        first = first or g.graph
        dl = torch.as_tensor(delay).expand(Bn) if isinstance(delay, int) else torch.tensor(delay)
        pre = (torch.arange(H)[None, :] < dl[:, None])[..., None].expand(Bn, H, A).cuda()
        assert torch.equal(out[pre].view(torch.int32), prev.cuda()[pre].view(torch.int32)), delay
        w = np.stack([soft_mask(H, int(x), overlap) for x in dl])
        coef = guidance_coef(D["num_inference_steps"], 5.0 if beta is None else beta)
        pn = ops.action_normalize(prev.cuda(), sa, sb, "bound")
        want_norm = m.infer_action(b["input_ids"].cuda(), pix.cuda(), itp, amask, vpos, ppos, apos,
                                   b["proprio"].cuda(), noise=noise, guide=(pn, w, coef), clip=False)
        clamped = torch.where(pre, want_norm, want_norm.clamp(-clipv, clipv))
        assert torch.equal(g.out_norm.view(torch.int32), clamped.view(torch.int32)), delay
        assert (g.out_norm[~pre].abs() <= clipv).all()
        want = ops.action_denormalize(clamped, sa, sb, "bound")
        assert torch.equal(out[~pre].view(torch.int32), want[~pre].view(torch.int32)), delay
        assert not torch.equal(out, plain)
    assert len(ag._obs_graphs) == n_graphs + 1
    if use_graph:
        assert first is not None and ag.observation_graph(Bn, (56, 56), channels_last=False, guidance=True).graph is first
        assert ag.observation_graph(Bn, (56, 56), channels_last=False).graph is plain_graph
    # calls without overlap: the graphs and the bits they had
    assert torch.equal(ag.act(*obs, noise=noise, channels_last=False).view(torch.int32), plain.view(torch.int32))
    again = ag.act(*obs, noise=noise, channels_last=False, prev_actions=prev, delay=1)
    assert torch.equal(again.view(torch.int32), hard.view(torch.int32))
    for bad, msg in ((dict(prev_actions=prev, delay=3, overlap=2), "delay <= overlap"),
                     (dict(prev_actions=prev, delay=1, overlap=5), "delay <= overlap"),
                     (dict(prev_actions=prev, delay=4, overlap=4), "delay < horizon_steps"),
                     (dict(overlap=3), "overlap needs prev_actions"),
                     (dict(prev_actions=prev, delay=1, guidance_beta=2.0), "guidance_beta needs overlap")):
        with pytest.raises(ValueError, match=msg):
            ag.act(*obs, channels_last=False, **bad)
