"""Action-prefix conditioning end to end on the MI355X, tiny model: training loss and gradients, the saved
encoder inputs, inference (eager, both glue routes, hipGraph), EvalAgent.act and TrainAgent.

No reference exists for this feature: the pin is tests/prefix_ref.py, the semantics of DESIGN 7f composed from the CPU
oracle's pieces (it equals the oracle bit for bit without a prefix, tests/test_prefix_host.py).  The parity
tolerances of tests/test_pizero_gpu.py catch a wrong mask or a wrong d per sample, but not a prefix row fed time t
instead of 1 or psi_t instead of x1 (0.1 % / 0.6 % of the loss): those properties are pinned bit for bit here through
Engine.train_forward's saved tensors, and at kernel level in tests/test_prefix_kernels_gpu.py.
"""

import json
import logging
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.golden.make_golden import ref_cfg
from tests.oracle_helpers import O
from tests.pizero_gpu_helpers import GRAD_COS, GRAD_REL, build_gpu_model, gpu_inputs
from tests.prefix_ref import restatement_run

pytestmark = pytest.mark.gpu

D_MIX = (0, 1, 3)  # one sample without a prefix, one with the first row, one with all rows but the last (H = 4)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tiny():
    d = O.TINY_DIMS
    m = build_gpu_model(d)
    return d, m, gpu_inputs(m, d, 3)


@pytest.fixture(scope="module")
def ref():
    """the restatement on the fixture inputs with d = (0, 1, 3), in fp32 (with every gradient) and under bf16 autocast
    (its own deviation): computed once, shared, never modified"""
    d = O.TINY_DIMS
    r32, inp = restatement_run(d, 3, D_MIX)
    r16, _ = restatement_run(d, 3, D_MIX, bf16=True)
    return r32, r16, inp


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _loss(m, g, prefix_len=None, backward=True):
    m.zero_grad(set_to_none=True)
    kw = {} if prefix_len is None else dict(prefix_len=prefix_len)
    loss = m(input_ids=g["input_ids"], pixel_values=g["pixel_values"], causal_mask=g["causal_mask"],
             vlm_position_ids=g["vpos"], proprio_position_ids=g["ppos"], action_position_ids=g["apos"],
             proprios=g["proprios"], actions=g["actions32"], t=g["t32"], noise=g["x0"], **kw)
    if backward:
        loss.backward()
    torch.cuda.synchronize()
    return loss


def _infer(m, g, prefix=None, prefix_len=None, clip=False):
    kw = {} if prefix_len is None else dict(prefix_actions=prefix, prefix_len=prefix_len)
    return m.infer_action(input_ids=g["input_ids"], pixel_values=g["pixel_values"].float(),
                          image_text_proprio_mask=g["itp"], action_mask=g["amask"], vlm_position_ids=g["vpos"],
                          proprio_position_ids=g["ppos"], action_position_ids=g["apos"], proprios=g["proprios"],
                          noise=g["noise"], clip=clip, **kw)


def _grads(m):
    return {n: m._param(n).grad.detach().clone() for n in m._trainable_names()}


def _graph(m, g, clip=False, prefix=False):
    from pizero_native.graph import InferenceGraph

    ig = InferenceGraph(m, g["input_ids"].shape[0], clip=clip)
    if prefix:
        ig.enable_prefix()
    return ig


def _graph_args(m, g):
    return (g["input_ids"], g["pixel_values"], m.block_prefix_counts(g["itp"], g["amask"]), g["vpos"], g["ppos"],
            g["apos"], g["proprios"].float(), g["noise"])


# ------------------------------------------------------------------------------------- 1. no-prefix equivalence --
def test_zero_prefix_len_gives_the_bits_of_no_prefix(tiny):
    """prefix_len all zero against no argument: loss, every gradient and the actions, eager and through the graph"""
    d, m, g = tiny
    l0 = _loss(m, g).detach().clone()
    g0 = _grads(m)
    z = torch.zeros(3, dtype=torch.int64)
    l1 = _loss(m, g, prefix_len=z).detach().clone()
    g1 = _grads(m)
    assert torch.equal(_bits(l0.reshape(1)), _bits(l1.reshape(1))), (l0.item(), l1.item())
    assert set(g0) == set(g1) and g0
    bad = [n for n in g0 if not torch.equal(_bits(g0[n]), _bits(g1[n]))]
    assert not bad, bad
    for clip in (False, True):
        a0 = _infer(m, g, clip=clip).float()
        a1 = _infer(m, g, prefix=g["actions32"], prefix_len=z, clip=clip)
        assert a1.dtype == torch.float32 and torch.equal(_bits(a0), _bits(a1.to(a0.dtype))), clip
    plain = _graph(m, g)
    plain.load(*_graph_args(m, g))
    ap = plain.capture().replay().clone()
    pg = _graph(m, g, prefix=True)
    pg.load(*_graph_args(m, g), prefix=g["actions32"], prefix_len=z)
    a2 = pg.capture().replay().clone()
    pg.load(*_graph_args(m, g))  # no prefix given to a prefix-capable graph: prefix_len = 0
    a3 = pg.replay().clone()
    torch.cuda.synchronize()
    eager = _infer(m, g, prefix=g["actions32"], prefix_len=z)
    assert torch.equal(_bits(ap), _bits(a2)) and torch.equal(_bits(ap), _bits(a3)) and torch.equal(_bits(ap), _bits(eager))
    with pytest.raises(ValueError, match="enable_prefix"):
        plain.load(*_graph_args(m, g), prefix=g["actions32"], prefix_len=z)


# ------------------------------------------------------------------- 2. loss and gradients vs the restatement --
def test_loss_and_gradients_match_the_restatement(tiny, ref):
    """the loss rule of test_pizero_gpu._check_loss; per tensor GRAD_REL / GRAD_COS on the WHOLE gradient, widened to
    3 x the restatement's own bf16 deviation where that is larger; a tensor whose bf16 restatement deviates by more
    than 100 % (exact gradient 0: rounding noise only) must stay at that noise level, and an exactly-zero gradient
    must be exactly zero"""
    d, m, g = tiny
    r32, r16, _ = ref
    loss = _loss(m, g, prefix_len=torch.tensor(D_MIX)).item()
    tol = max(3 * abs(r16["loss"] - r32["loss"]), 1e-2 * abs(r32["loss"]))
    plain = _loss(m, g, backward=False).item()
    print(f"prefix loss {loss:.6f} restatement {r32['loss']:.6f} (bf16 {r16['loss']:.6f}); without a prefix {plain:.6f}")
    assert abs(plain - r32["loss"]) > tol  # the check can tell the two apart
    _loss(m, g, prefix_len=torch.tensor(D_MIX))
    assert abs(loss - r32["loss"]) <= tol, (loss, r32["loss"], r16["loss"])
    bad, worst, noise = [], [0.0, 1.0], 0
    names = m._trainable_names()
    assert len(names) > 20
    for n in names:
        got = m._param(n).grad.detach().double().cpu().flatten()
        want, wb = r32["grads"][n].double().flatten(), r16["grads"][n].double().flatten()
        wn = float(want.norm())
        if wn == 0.0:
            if float(got.abs().max()) != 0.0:
                bad.append((n, "restatement gradient is exactly 0"))
            continue
        brel = float((wb - want).norm()) / wn
        if brel > 1.0:
            noise += 1
            lim = 10.0 * max(wn, float(wb.norm()))
            if float(got.norm()) > lim:
                bad.append((n, f"noise-level gradient {float(got.norm()):.3e} > {lim:.3e}"))
            continue
        tol_g = max(GRAD_REL, 3.0 * brel)
        cmin = min(GRAD_COS, 1.0 - 0.5 * tol_g * tol_g)
        rel = float((got - want).norm()) / wn
        cos = float(got @ want) / (float(got.norm()) * wn + 1e-300)
        worst = [max(worst[0], rel), min(worst[1], cos)]
        if rel > tol_g or cos < cmin:
            bad.append((n, round(rel, 5), round(cos, 6), round(tol_g, 4)))
    print(f"[prefix grad gate] {len(names)} tensors ({noise} noise-only): max rel-L2 {worst[0]:.4f}, min cos {worst[1]:.6f}")
    assert not bad, "\n".join(map(str, bad))


# ----------------------------------------------------------------------------------- 3. the saved encoder inputs --
def test_saved_encoder_inputs_hold_clean_prefix_rows(tiny, monkeypatch):
    """Engine.train_forward's save["ae_psi"] / save["ae_cat"]: a prefix row's encoder input is bf16(x1) exactly (no
    noise term) and its time columns are the embedding of 1.0f; every other row is what a run without a prefix
    saves.  Both time modes."""
    from pizero_native import ops

    d, m, g = tiny
    e = m._engine()
    saves = []
    orig = e.train_forward
    monkeypatch.setattr(e, "train_forward", lambda **kw: (saves.append(kw["save"]), orig(**kw))[1])
    H, A, aH = d["horizon_steps"], d["action_dim"], d["act_hidden"]
    pre = (torch.arange(H, device="cuda")[None, :] < torch.tensor(D_MIX, device="cuda")[:, None]).reshape(-1)
    keep = e.d.time_bf16
    try:
        for mode in (False, True):
            e.d.time_bf16 = mode
            saves.clear()
            with torch.no_grad():
                _loss(m, g, backward=False)
                _loss(m, g, prefix_len=torch.tensor(D_MIX), backward=False)
            s0, s1 = saves
            assert s0["prefix_len"] is None and s1["prefix_len"].tolist() == list(D_MIX)
            psi0, psi1, cat0, cat1 = s0["ae_psi"], s1["ae_psi"], s0["ae_cat"], s1["ae_cat"]
            assert psi1.shape == (3 * H, A) and cat1.shape == (3 * H, 2 * aH)
            x1 = g["actions32"].reshape(3 * H, A).to(torch.bfloat16)
            assert torch.equal(_bits(psi1[pre]), _bits(x1[pre]))
            assert not torch.equal(_bits(psi0[pre]), _bits(x1[pre]))
            assert torch.equal(_bits(psi1[~pre]), _bits(psi0[~pre]))
            one = torch.empty(1, aH, device="cuda", dtype=torch.bfloat16)
            ops.time_embed(torch.ones(1, device="cuda"), one, e.d.tmax, ref_bf16=mode)
            assert torch.equal(_bits(cat1[pre][:, :aH]), _bits(one.expand(int(pre.sum()), aH)))
            assert not torch.equal(_bits(cat0[pre][:, :aH]), _bits(cat1[pre][:, :aH]))
            assert torch.equal(_bits(cat1[~pre]), _bits(cat0[~pre]))
            # the Linear columns of a prefix row: linear_1 of the clean action, i.e. of a run whose noise is irrelevant
            assert not torch.equal(_bits(cat1[pre][:, aH:]), _bits(cat0[pre][:, aH:]))
    finally:
        e.d.time_bf16 = keep


# ----------------------------------------------------------------------------------------------- 4. the actions --
def test_actions_with_a_prefix(tiny, ref):
    d, m, g = tiny
    r32, r16, _ = ref
    pl = torch.tensor(D_MIX)
    a = _infer(m, g, prefix=g["actions32"], prefix_len=pl)
    assert a.dtype == torch.float32
    want, wb = r32["actions"].numpy(), r16["actions"].numpy()
    got = a.cpu().numpy()
    dev, err = np.abs(wb - want), np.abs(got - want)
    print(f"prefix actions: mean|d| {err.mean():.4g} max {err.max():.4g}; restatement bf16 {dev.mean():.4g} / {dev.max():.4g}")
    assert err.mean() <= max(3 * dev.mean(), 5e-3), (err.mean(), dev.mean())
    assert err.max() <= max(3 * dev.max(), 3e-2), (err.max(), dev.max())
    # prefix rows come back bit for bit; the sample without a prefix is the no-prefix chunk bit for bit
    pf = g["actions32"]
    assert torch.equal(_bits(a[1, :1]), _bits(pf[1, :1])) and torch.equal(_bits(a[2, :3]), _bits(pf[2, :3]))
    plain = _infer(m, g).float()
    assert torch.equal(_bits(a[0]), _bits(plain[0]))
    assert not torch.equal(a[1, 1:], plain[1, 1:]) and not torch.equal(a[2, 3:], plain[2, 3:])
    # the prefix rows of the noise are ignored
    g2 = dict(g, noise=g["noise"].clone())
    g2["noise"][1, 0] = 9.0
    g2["noise"][2, :3] = -9.0
    assert torch.equal(_bits(_infer(m, g2, prefix=pf, prefix_len=pl)), _bits(a))
    # clamp exemption: prefix values of +-1.5 are returned as given, everything else is clamped
    pf15 = pf.clone()
    pf15[1, 0, :] = 1.5
    pf15[2, :3, 2] = -1.5
    pf15[0, 0, :] = 1.5  # beyond d_0 = 0: ignored
    ac = _infer(m, g, prefix=pf15, prefix_len=pl, clip=True)
    assert torch.equal(_bits(ac[1, :1]), _bits(pf15[1, :1])) and torch.equal(_bits(ac[2, :3]), _bits(pf15[2, :3]))
    assert ac[1, 1:].abs().max() <= 1.0 and ac[2, 3:].abs().max() <= 1.0 and ac[0].abs().max() <= 1.0
    assert torch.equal(_bits(ac[0]), _bits(_infer(m, g, clip=True).float()[0]))
    with pytest.raises(ValueError, match="prefix_len must lie in"):
        _infer(m, g, prefix=pf, prefix_len=torch.tensor([0, 4, 1]))
    with pytest.raises(ValueError, match="prefix_actions must be"):
        _infer(m, g, prefix=pf[:, :3], prefix_len=pl)


# ---------------------------------------------------------------------------------------- 5. the two glue routes --
def test_glue_routes_agree_with_a_prefix(tiny, monkeypatch):
    d, m, g = tiny
    pl = torch.tensor(D_MIX)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("PZ_FUSED_GLUE", fused)
        outs.append(_infer(m, g, prefix=g["actions32"], prefix_len=pl, clip=True).clone())
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), float((outs[0] - outs[1]).abs().max())


# ------------------------------------------------------------------------------------------------- 6. the graph --
def test_graph_replays_any_prefix_without_recapture(tiny):
    d, m, g = tiny
    ig = _graph(m, g, clip=True, prefix=True)
    pf = g["actions32"]
    ig.load(*_graph_args(m, g), prefix=pf, prefix_len=torch.tensor(D_MIX))
    ig.capture()
    captured = ig.graph
    a = ig.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(_infer(m, g, prefix=pf, prefix_len=torch.tensor(D_MIX), clip=True)))
    pf2 = (pf * 0.5).contiguous()
    for pl in ([3, 0, 2], 1, torch.tensor([0, 0, 0], device="cuda", dtype=torch.int32)):
        ig.load(*_graph_args(m, g), prefix=pf2, prefix_len=pl)
        b = ig.replay().clone()
        torch.cuda.synchronize()
        plt = torch.as_tensor(pl).cpu()
        plt = plt.expand(3) if plt.dim() == 0 else plt
        eager = _infer(m, g, prefix=pf2, prefix_len=plt, clip=True)
        assert torch.equal(_bits(b), _bits(eager)), pl
    assert ig.graph is captured
    with pytest.raises(ValueError, match=r"\[0, horizon_steps - 1\]"):
        ig.load(*_graph_args(m, g), prefix=pf, prefix_len=[0, 1, 4])
    with pytest.raises(ValueError, match="go together"):
        ig.load(*_graph_args(m, g), prefix=pf)
    for bad in (1.0, True, torch.tensor([0.0, 1.0, 2.0])):
        with pytest.raises(ValueError, match="must be integers"):
            ig.load(*_graph_args(m, g), prefix=pf, prefix_len=bad)


# ------------------------------------------------------------------------------------------- 7. EvalAgent.act --
def _bridge_stats():
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")))
    s["proprio"]["mean"] = [0.0] * 7
    s["proprio"]["std"] = [1.0 - 1e-8] * 7  # (x - 0) / (std + 1e-8): the identity
    return s


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("kind", ["bound", "gaussian"])
def test_act_with_prev_actions(tmp_path, use_graph, kind):
    """rows < delay of act's output are the caller's bits; the rest are infer_action on the normalised prefix followed
    by the denormalisation; another delay and prefix replay the same capture; calls without prev_actions keep the
    graph without the option"""
    from oracle.synth import param_rule, tensor_seed
    from pizero_native import ops
    from src.agent.eval import EvalAgent
    from src.agent.train import SyntheticBridgeDataset

    p = tmp_path / "stats.json"
    p.write_text(json.dumps(_bridge_stats()))
    c = ref_cfg(O.TINY_DIMS)
    c.update(dict(use_bf16=True, load_pretrained_weights=False))
    c["env"] = dict(adapter=dict(dataset_statistics_path=str(p), proprio_normalization_type="gaussian",
                                 action_normalization_type=kind))
    ag = EvalAgent(c, use_graph=use_graph)
    for name in ag.model._arena.order:
        v = ag.model._arena.view(name)
        off, sc = param_rule(name, tuple(v.shape))
        ops.fill_uniform(v, tensor_seed(name, 0), off, sc)
    torch.cuda.synchronize()
    m = ag.model
    B, H, A = 2, 4, 7
    b = next(iter(SyntheticBridgeDataset(c, B, seed=3)))
    noise = torch.randn(B, H, A, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    st = _bridge_stats()["action"]
    names = ("p01", "p99") if kind == "bound" else ("mean", "std")
    sa, sb = (torch.tensor(st[k], dtype=torch.float64).float().cuda() for k in names)
    r = np.random.default_rng(7)
    lo, hi = np.array(st["p01"]), np.array(st["p99"])
    prev = torch.from_numpy(lo + (hi - lo) * r.uniform(-0.2, 1.2, (B, H, A))).float()  # some beyond [p01, p99]
    plain = ag.act(b["pixel_values"], b["input_ids"], b["attention_mask"], b["proprio"], noise=noise,
                   channels_last=False).clone()
    n_graphs = len(ag._obs_graphs)
    mask, vpos, ppos, apos = m.build_causal_mask_and_position_ids(b["attention_mask"].cuda(), torch.bfloat16)
    itp, amask = m.split_full_mask_into_submasks(mask)
    pix = ((b["pixel_values"].float() / 255 - 0.5) / 0.5).to(torch.bfloat16)
    first = None
    for delay in ([1, 3], 2, [0, 0]):
        out = ag.act(b["pixel_values"], b["input_ids"], b["attention_mask"], b["proprio"], noise=noise,
                     channels_last=False, prev_actions=prev, delay=delay).clone()
        g = ag.observation_graph(B, (56, 56), channels_last=False, prefix=True)
        first = first or g.graph
        dl = torch.as_tensor(delay).expand(B) if isinstance(delay, int) else torch.tensor(delay)
        pre = (torch.arange(H)[None, :] < dl[:, None])[..., None].expand(B, H, A).cuda()
        assert torch.equal(_bits(out[pre]), _bits(prev.cuda()[pre])), delay
        pn = ops.action_normalize(prev.cuda(), sa, sb, kind)
        want_norm = m.infer_action(b["input_ids"].cuda(), pix.cuda(), itp, amask, vpos, ppos, apos,
                                   b["proprio"].cuda(), noise=noise, prefix_actions=pn, prefix_len=dl)
        assert torch.equal(_bits(g.out_norm), _bits(want_norm)), delay
        want = ops.action_denormalize(want_norm, sa, sb, kind)
        assert torch.equal(_bits(out[~pre]), _bits(want[~pre])), delay
        if int(dl.max()) == 0:
            assert torch.equal(_bits(out), _bits(plain))
    assert len(ag._obs_graphs) == n_graphs + 1
    if use_graph:
        assert first is not None and ag.observation_graph(B, (56, 56), channels_last=False, prefix=True).graph is first
    with pytest.raises(ValueError, match="go together"):
        ag.act(b["pixel_values"], b["input_ids"], b["attention_mask"], b["proprio"], channels_last=False, delay=1)
    with pytest.raises(ValueError, match="prev_actions must be"):
        ag.act(b["pixel_values"], b["input_ids"], b["attention_mask"], b["proprio"], channels_last=False,
               prev_actions=prev[:, :2], delay=1)
    with pytest.raises(ValueError, match=r"\[0, horizon_steps - 1\]"):
        ag.act(b["pixel_values"], b["input_ids"], b["attention_mask"], b["proprio"], channels_last=False,
               prev_actions=prev, delay=H)
    with pytest.raises(ValueError, match="must be integers"):
        ag.act(b["pixel_values"], b["input_ids"], b["attention_mask"], b["proprio"], channels_last=False,
               prev_actions=prev, delay=1.0)


# ---------------------------------------------------------------------------------------------- 8. TrainAgent --
def _train_cfg(**kw):
    c = ref_cfg(O.TINY_DIMS)
    c.update(dict(global_batch_size=8, per_device_batch_size=4, action_lr=1e-3, vlm_lr=1e-3,
                  action_weight_decay=0.0, vlm_weight_decay=0.0, max_grad_norm=1.0, n_updates=3, log_freq=1,
                  train_vlm=True, use_bf16=True, flow_sampling="beta", load_pretrained_weights=False, seed=5,
                  action_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2),
                  vlm_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2)))
    c.update(kw)
    return c


def _run_logged(agent, seed=0):
    """run() and the logged loss of every micro-batch; every prefix_len the model saw"""
    losses, seen = [], []

    class Grab(logging.Handler):
        def emit(self, rec):
            if rec.msg.startswith("Batch"):
                losses.append(float(rec.args[2]))

    fwd = agent.model.forward

    def spy(*a, **kw):
        seen.append(kw.get("prefix_len"))
        return fwd(*a, **kw)

    agent.model.forward = spy
    lg = logging.getLogger("src.agent.train")
    h, lvl = Grab(), lg.level
    lg.addHandler(h)
    lg.setLevel(logging.INFO)
    try:
        if seed is not None:
            torch.manual_seed(seed)
        agent.run()
    finally:
        lg.removeHandler(h)
        lg.setLevel(lvl)
        del agent.model.forward
    return losses, seen


def _new_agent(**kw):
    from src.agent.train import TrainAgent

    torch.manual_seed(0)
    return TrainAgent(_train_cfg(**kw))


def test_train_agent_with_the_key_off_is_the_run_without_it():
    """action_prefix_max_delay: 0 against a config without the key: the same loss trajectory over 3 updates and the
    same weights, bit for bit, and no prefix_len ever reaches the model (so the engine launches the kernels it always
    launched); with D = 3 the trajectory differs and every micro-batch carries its draw"""
    from pizero_native import augment as A

    a, b = _new_agent(), _new_agent(action_prefix_max_delay=0)
    la, sa_ = _run_logged(a)
    lb, sb_ = _run_logged(b)
    assert len(la) == 6 and la == lb, (la, lb)
    assert all(s is None for s in sa_ + sb_)
    wa, wb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(wa[k], wb[k]) for k in wa)
    c = _new_agent(action_prefix_max_delay=3)
    lc, sc_ = _run_logged(c)
    assert len(lc) == 6 and all(np.isfinite(x) and x > 0 for x in lc) and lc != la
    for k, s in enumerate(sc_):
        assert s.dtype == torch.int32 and s.tolist() == A.draw_prefix_len(4, 3, 5, k, 0).tolist()
    assert len({tuple(s.tolist()) for s in sc_}) > 1


class _Feed:
    """micro-batches ``start``.. of a fixed list, torch's generator re-seeded before each (the flow-matching times of
    micro-batch k are then the same in an uninterrupted and in a resumed run)"""

    def __init__(self, batches, start):
        self.batches, self.start = batches, start

    def __iter__(self):
        for k in range(self.start, len(self.batches)):
            torch.manual_seed(100 + k)
            yield self.batches[k]


def test_train_agent_resumes_the_draws(tmp_path):
    """D = 3, one micro-batch per update: an uninterrupted run of 3 updates against a run resumed from the checkpoint
    after update 2 and fed the third micro-batch.  The resumed agent draws the prefix lengths of micro-batch 2 -- not
    those of micro-batch 1 again, although the checkpoint's cnt_batch is 1 (the index of its last micro-batch) -- and
    ends with the uninterrupted run's weights bit for bit."""
    from pizero_native import augment as A
    from src.agent.train import SyntheticBridgeDataset, TrainAgent

    kw = dict(action_prefix_max_delay=3, global_batch_size=4, per_device_batch_size=4, n_updates=3)
    it = iter(SyntheticBridgeDataset(_train_cfg(), 4, seed=9))
    batches = [next(it) for _ in range(3)]
    torch.manual_seed(0)
    a = TrainAgent(_train_cfg(log_dir=str(tmp_path), save_model_freq=2, **kw), dataset=_Feed(batches, 0))
    _, seen_a = _run_logged(a, seed=None)
    path = tmp_path / "checkpoint" / "step2.pt"
    assert path.exists() and a.cnt_update == 3 and a.micro_batches_seen == 3
    b = TrainAgent(_train_cfg(resume_checkpoint_path=str(path), **kw), dataset=_Feed(batches, 2))
    assert (b.cnt_update, b.cnt_batch, b.micro_batches_seen) == (2, 1, 2)
    _, seen_b = _run_logged(b, seed=None)
    assert b.cnt_update == 3 and len(seen_a) == 3 and len(seen_b) == 1
    draws = [A.draw_prefix_len(4, 3, 5, k, 0).tolist() for k in range(3)]
    assert [s.tolist() for s in seen_a] == draws and seen_b[0].tolist() == draws[2] != draws[1]
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_train_agent_refusals_and_evaluate():
    from src.agent.train import SyntheticBridgeDataset, TrainAgent
    from tests.golden.make_golden_adaln import adaptive_cfg

    with pytest.raises(ValueError, match="action_prefix_max_delay must lie in"):
        _new_agent(action_prefix_max_delay=4)  # = horizon_steps
    ca = adaptive_cfg(O.TINY_DIMS, "adaLN")
    for k, v in _train_cfg(action_prefix_max_delay=2).items():
        if k not in ca or k in ("action_prefix_max_delay", "global_batch_size", "per_device_batch_size"):
            ca[k] = v
    with pytest.raises(NotImplementedError, match="action_expert_adaptive_mode"):
        TrainAgent(ca)
    # evaluate() reports the suffix L1 around the ground-truth first D actions when D > 0, and only then
    c = _train_cfg(action_prefix_max_delay=3, eval_size=4)
    on = TrainAgent(c, val_dataset=SyntheticBridgeDataset(c, 4, seed=77))
    r = on.evaluate()
    assert np.isfinite(r["l1"]) and np.isfinite(r["l1_prefix_suffix"]) and r["l1_prefix_suffix"] > 0
    c0 = _train_cfg(eval_size=4)
    off = TrainAgent(c0, val_dataset=SyntheticBridgeDataset(c0, 4, seed=77))
    assert "l1_prefix_suffix" not in off.evaluate()
