"""EMA / SWA weight averaging, in-training evaluation and averaged checkpoints at the agent level (MI355X).

The schedule and the EMA bits are held against the reference's own ModelAveraging (tests/golden/averaging.npz, written
by tests/golden/make_golden_averaging.py on the CPU); the training-loop integration is held against a CPU replay of
copy / ``torch.lerp`` from the saved live weights.
"""

import types

import numpy as np
import pytest
import torch

from tests.oracle_helpers import load_golden
from tests.test_agents_gpu import _cfg, _one_update

pytestmark = pytest.mark.gpu

EMA = dict(use_ema=True, ema_start=3, ema_freq=2, ema_decay=0.99, ema_device="cuda")
SWA = dict(use_swa=True, swa_start=2, swa_freq=3, swa_device="cpu")  # cpu: accepted, the average stays on the GPU


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.detach().contiguous().view(torch.int16)


def same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(bits(a), bits(b)) if a.dtype == torch.bfloat16 else torch.equal(a, b)


def same_state(sa, sb):
    assert list(sa) == list(sb)
    bad = [k for k in sa if not same_bits(sa[k], sb[k])]
    assert not bad, (len(bad), bad[:5])


class FlatModel(torch.nn.Module):
    """one parameter that is a view (element offset 8) of a flat CUDA buffer: the smallest "arena" model"""

    def __init__(self, n):
        super().__init__()
        self._arena = types.SimpleNamespace(data=torch.zeros(8 + (n + 7) // 8 * 8, device="cuda", dtype=torch.bfloat16))
        self.w = torch.nn.Parameter(self._arena.data[8:8 + n])


def _drive(cfg, g):
    """the fixture's script: update u = 1..12 sets the live weights, then maybe_initialize(u), maybe_update(u)"""
    from src.agent.model_averaging import ModelAveraging

    live = torch.from_numpy(g["live"].view(np.int16)).cuda()
    model = FlatModel(live.shape[1])
    ma = ModelAveraging(model, cfg, torch.device("cuda:0"))
    out = []
    for u in range(1, live.shape[0] + 1):
        with torch.no_grad():
            model.w.copy_(live[u - 1].view(torch.bfloat16))
        ma.maybe_initialize(u)
        ma.maybe_update(u)
        sd = ma.state_dict()
        if not sd:
            out.append((-1, None))
            continue
        assert sd["model_type"] == ("ema" if cfg.get("use_ema") else "swa")
        assert sd["n_averaged"].dtype == torch.int64 and sd["n_averaged"].dim() == 0
        out.append((int(sd["n_averaged"]), sd["state_dict"]["w"].clone()))
        assert same_bits(model.w, live[u - 1].view(torch.bfloat16))  # the live weights are never touched
    return out


def test_ema_trajectory_matches_reference_bitwise():
    g = load_golden("averaging")
    assert [f"{k}={v}" for k, v in EMA.items() if k != "ema_device"] == [s for s in g["ema/cfg"] if "device" not in s]
    out = _drive(EMA, g)
    assert [n for n, _ in out] == g["ema/n"].tolist()
    assert max(g["ema/n"]) >= 4  # the schedule copies once and lerps several times
    for u, (n, avg) in enumerate(out):
        if n < 0:
            continue
        want = torch.from_numpy(g["ema/avg"][u].view(np.int16))
        bad = (bits(avg).cpu() != want).nonzero().flatten()
        assert bad.numel() == 0, (u + 1, n, bad.numel(), bad[:5].tolist())


def test_swa_schedule_and_mean_bound():
    """n_averaged as the reference's; after k averaged snapshots |avg - fp64 mean| <= (k - 1) 2^-8 max|snapshot|
    (elementwise): each lerp rounds its bf16 result once, by at most half an ulp = 2^-8 of a value that lies between
    the snapshots, and earlier errors only shrink under the convex update.  The first snapshot is a copy: exact."""
    g = load_golden("averaging")
    assert [f"{k}={v}" for k, v in SWA.items()] == list(g["swa/cfg"])
    out = _drive(SWA, g)
    ns = [n for n, _ in out]
    assert ns == g["swa/n"].tolist() and max(ns) >= 4
    live = torch.from_numpy(g["live"].view(np.int16)).view(torch.bfloat16).double()
    snaps, prev = [], 0
    for u, (n, avg) in enumerate(out):
        if n < 0:
            continue
        if n > prev:  # this update averaged the live weights of update u + 1
            snaps.append(live[u])
            prev = n
        if n == 0:  # started, nothing averaged yet: the copy made at the start
            assert same_bits(avg, live[u].to(torch.bfloat16))
            continue
        assert len(snaps) == n
        S = torch.stack(snaps)
        err = (avg.cpu().double() - S.mean(0)).abs()
        bound = (n - 1) * 2.0 ** -8 * S.abs().amax(0)
        worst = float((err - bound).max())
        print(f"update {u + 1}: k = {n}, max err {float(err.max()):.3e}, max (err - bound) {worst:.3e}")
        assert worst <= 0, (u + 1, n, worst)


def test_lora_average_through_merged_shadow_and_captured_graph():
    """Under LoRA the average moves the adapters only; inside swapped() a graph captured BEFORE the swap replays with the
    averaged weights (same addresses, merged shadow rebuilt on the version bump) and equals, bit for bit, a fresh model
    loaded from the averaged state_dict; after it, the live result is back."""
    from pizero_native.averaging import FlatAverage
    from pizero_native.optim import FusedAdamW
    from tests.oracle_helpers import O
    from tests.pizero_gpu_helpers import gpu_inputs, run_infer, run_loss
    from tests.test_lora_gpu import _graph, build_lora_model

    d, B = O.TINY_DIMS, 3
    m = build_lora_model(d)
    gi = gpu_inputs(m, d, B)
    fa = FlatAverage.for_model(m)
    base = m._arena.data.clone()
    opt = FusedAdamW(m.lora_trainable_vlm_parameters + m.action_expert_parameters, lr=1e-2, state_bits=32)
    run_loss(m, gi)
    opt.step()
    fa.update(0.25)
    live = m._arena.data.clone()
    sd_live, sd_avg = m.state_dict(), fa.state_dict()
    assert list(sd_avg) == list(sd_live) and any(k.endswith("lora_A") for k in sd_avg)
    named = dict(m.named_parameters())
    for k in sd_live:
        if k in named and not named[k].requires_grad:  # frozen: the initial copy, which is the live tensor
            assert same_bits(sd_avg[k], sd_live[k]), k
    lb = [k for k in sd_live if k.endswith("lora_B") and named[k].requires_grad]
    assert any(not same_bits(sd_avg[k], sd_live[k]) for k in lb)
    want = torch.lerp(base.cpu(), live.cpu(), 0.25)
    for k in lb[:8]:
        s = m._arena.slots[k]
        assert same_bits(sd_avg[k].flatten(), want[s.offset:s.offset + s.numel]), k
    ig = _graph(m, gi, B)
    out_live = ig.replay().clone()
    with fa.swapped():
        out_avg = ig.replay().clone()
        eager_avg = run_infer(m, gi, clip=False)
    out_back = ig.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(bits(m._arena.data), bits(live))
    assert torch.equal(out_back, out_live) and not torch.equal(out_avg, out_live)
    assert torch.equal(out_avg.float(), eager_avg.float())
    m2 = build_lora_model(d)
    m2.load_state_dict({k: v.clone() for k, v in sd_avg.items()}, strict=True)
    a2 = run_infer(m2, gpu_inputs(m2, d, B), clip=False)
    assert torch.equal(out_avg.float(), a2.float()), float((out_avg.float() - a2.float()).abs().max())


# ------------------------------------------------------------------------------------------ training loop --
def _ema_cfg(log_dir, n_updates):
    c = _cfg()
    c.update(dict(log_dir=str(log_dir), n_updates=n_updates, save_model_freq=1, use_ema=True, ema_start=1,
                  ema_decay=0.5, ema_freq=1, ema_device="cuda", eval_size=8, eval_freq=10 ** 9))
    return c


def _load(path):
    return torch.load(path, weights_only=True, map_location="cpu")


def _val(cfg):
    from src.agent.train import SyntheticBridgeDataset

    return SyntheticBridgeDataset(cfg, 4, seed=77)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """agent A: three updates with EMA from the first one, a checkpoint after each"""
    from src.agent.train import TrainAgent

    d = tmp_path_factory.mktemp("ema")
    c = _ema_cfg(d, 3)
    a = TrainAgent(c, val_dataset=_val(c)).run()
    return a, d


def test_run_with_ema_saves_the_averaged_weights(trained):
    a, d = trained
    assert a.cnt_update == 3 and a.model_averaging.n_averaged == 3
    avg, last = None, None
    for step in (1, 2, 3):
        ck = _load(d / "checkpoint" / f"step{step}.pt")
        assert "model_train" in ck and list(ck["model_train"]) == list(ck["model"]) == list(a.model.state_dict())
        assert ck["n_averaged"].dtype == torch.int64 and ck["n_averaged"].dim() == 0 and int(ck["n_averaged"]) == step
        live = ck["model_train"]
        # update 1 starts the average (a copy, n = 0) and its first update copies again; then lerp with 1 - 0.5
        avg = ({k: v.clone() for k, v in live.items()} if avg is None else
               {k: torch.lerp(avg[k], live[k], 1.0 - 0.5) if live[k].is_floating_point() else live[k] for k in live})
        same_state(ck["model"], avg)
        last = live
    same_state({k: v for k, v in a.model.state_dict().items()}, last)  # the live weights are back after the saves
    moved = [k for k in last if not same_bits(last[k], avg[k])]
    assert moved, "the averaged weights equal the live ones everywhere"


def test_evaluate_uses_averaged_weights_and_restores_live(trained):
    from src.agent.train import TrainAgent

    a, d = trained
    ck = _load(d / "checkpoint" / "step3.pt")
    live0 = {k: v.detach().clone() for k, v in a.model.state_dict().items()}
    ver0 = a.model._engine().weights_version()
    torch.manual_seed(11)
    ra = a.evaluate()
    assert a.model._engine().weights_version() > ver0
    same_state(a.model.state_dict(), live0)
    assert a.model.training and a.last_eval is ra
    assert set(ra) == {"l1", "accuracy", "cnt_batch"} and len(ra["accuracy"]) == 5 and ra["cnt_batch"] == a.cnt_batch
    assert np.isfinite(ra["l1"]) and all(0.0 <= x <= 1.0 for x in ra["accuracy"])
    # agent B: averaging off, resumed from A's checkpoint -> its LIVE weights are A's average
    c = _cfg()
    c.update(dict(resume_checkpoint_path=str(d / "checkpoint" / "step3.pt"), eval_size=8))
    b = TrainAgent(c, val_dataset=_val(c))
    assert not b.model_averaging.active
    same_state({k: v.cpu() for k, v in b.model.state_dict().items()}, ck["model"])
    torch.manual_seed(11)
    rb = b.evaluate()
    assert (ra["l1"], ra["accuracy"]) == (rb["l1"], rb["accuracy"]), (ra, rb)
    # ... and they are not the live weights: a trained tensor differs
    trained_keys = [k for k, p in a.model.named_parameters() if p.requires_grad]
    assert any(not same_bits(ck["model"][k], ck["model_train"][k]) for k in trained_keys)


def test_exact_resume_of_live_and_averaged_weights(tmp_path):
    from src.agent.train import SyntheticBridgeDataset, TrainAgent

    c = _ema_cfg(tmp_path, 2)
    a = TrainAgent(c).run()
    path = tmp_path / "checkpoint" / "step2.pt"
    c2 = _ema_cfg(tmp_path / "b", 2)
    c2.update(dict(resume_checkpoint_path=str(path)))
    b = TrainAgent(c2)
    assert b.cnt_update == 2 and b.model_averaging.active
    assert a.model_averaging.n_averaged == b.model_averaging.n_averaged == 2

    def check():
        same_state(a.model.state_dict(), b.model.state_dict())
        same_state(a.model_averaging.state_dict()["state_dict"], b.model_averaging.state_dict()["state_dict"])
        assert a.model_averaging.n_averaged == b.model_averaging.n_averaged

    check()
    batch = next(iter(SyntheticBridgeDataset(c, 4, seed=9)))
    for ag in (a, b):
        _one_update(ag, batch, 5)
        ag.cnt_update += 1
        ag.model_averaging.maybe_initialize(ag.cnt_update)
        ag.model_averaging.maybe_update(ag.cnt_update)
    assert a.model_averaging.n_averaged == 3
    check()
    # a checkpoint without "model_train" (the reference's layout) loads as before: live <- "model", no average
    ck = _load(path)
    model_train = ck.pop("model_train")
    torch.save(ck, tmp_path / "plain.pt")
    c3 = _ema_cfg(tmp_path / "c", 2)
    c3.update(dict(resume_checkpoint_path=str(tmp_path / "plain.pt")))
    p = TrainAgent(c3)
    assert not p.model_averaging.active and p.cnt_update == 2
    same_state({k: v.cpu() for k, v in p.model.state_dict().items()}, ck["model"])
    assert any(not same_bits(ck["model"][k], model_train[k]) for k in ck["model"])


def test_averaging_off_checkpoint_is_unchanged(tmp_path):
    from src.agent.train import TrainAgent

    c = _cfg()
    c.update(dict(log_dir=str(tmp_path), n_updates=1, save_model_freq=1))
    a = TrainAgent(c).run()
    assert not a.run_eval and not a.model_averaging.active
    ck = _load(tmp_path / "checkpoint" / "step1.pt")
    assert ck["n_averaged"] == 1 and "model_train" not in ck
    same_state({k: v.cpu() for k, v in a.model.state_dict().items()}, ck["model"])


def test_run_evaluates_every_eval_freq_and_honours_save_model_start(tmp_path):
    from src.agent.train import TrainAgent

    c = _cfg()
    c.update(dict(log_dir=str(tmp_path), n_updates=3, save_model_freq=1, save_model_start=1, eval_freq=4, eval_size=4))
    a = TrainAgent(c, val_dataset=_val(c))
    assert a.run_eval and a.per_device_num_eval_batch == 1 and a.last_eval is None
    a.run()
    saved = sorted(p.name for p in (tmp_path / "checkpoint").iterdir())
    assert saved == ["step2.pt", "step3.pt"]  # step 1 is not past save_model_start; the last update always saves
    # 3 updates x 2 accumulated batches: (cnt_batch + 1) % 4 == 0 at cnt_batch 3 only
    assert a.last_eval is not None and a.last_eval["cnt_batch"] == 3 and len(a.last_eval["accuracy"]) == 5
    assert a.model.training
