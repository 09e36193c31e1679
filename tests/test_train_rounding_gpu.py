"""TrainAgent with ``optimizer_rounding: compensated`` at the tiny dims: the compensation words travel through both
optimizers' state dicts, so a resumed run continues the three-update run bit for bit (weights and comp)."""

import pytest
import torch

from tests.test_agents_gpu import _cfg, _one_update

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _comps(agent):
    out = []
    for o in agent.optimizers:
        sd = o.state_dict()
        assert sd["param_groups"][0]["rounding"] == "compensated" and sd["state"]
        for i in sorted(sd["state"]):
            c = sd["state"][i]["comp"]
            assert c.dtype == torch.bfloat16
            out.append(c)
    return out


def test_compensated_run_saves_resumes_and_continues_bitwise(tmp_path):
    from src.agent.train import SyntheticBridgeDataset, TrainAgent

    c = _cfg()
    c.update(dict(log_dir=str(tmp_path), n_updates=2, save_model_freq=2, optimizer_rounding="compensated"))
    a = TrainAgent(c)
    assert all(o.rounding == "compensated" for o in a.optimizers) and len(a.optimizers) == 2
    losses = []
    h = a.model.register_forward_hook(lambda mod, args, out: losses.append(out.detach().float().reshape(1)))
    a.run()
    h.remove()
    assert a.cnt_update == 2 and len(losses) == a.cnt_batch == 4  # two micro-batches per update
    assert bool(torch.isfinite(torch.cat(losses)).all()), losses
    assert any(bool(x.any()) for x in _comps(a)), "no compensation word was ever written"
    path = tmp_path / "checkpoint" / "step2.pt"
    ck = torch.load(path, weights_only=True, map_location="cpu")
    for key in ("action_optimizer", "vlm_optimizer"):
        assert ck[key]["param_groups"][0]["rounding"] == "compensated"
        assert ck[key]["param_groups"][0]["seed"] == int(c.get("seed", 0))
        assert all("comp" in st for st in ck[key]["state"].values())
    c2 = _cfg()
    c2.update(dict(resume_checkpoint_path=str(path), optimizer_rounding="compensated"))
    b = TrainAgent(c2)
    assert b.cnt_update == 2

    def check():
        sa, sb = a.model.state_dict(), b.model.state_dict()
        bad = [k for k in sa if not torch.equal(_bits(sa[k]), _bits(sb[k]))]
        assert not bad, (len(bad), bad[:5])
        ca, cb = _comps(a), _comps(b)
        assert len(ca) == len(cb) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(ca, cb))

    check()
    batch = next(iter(SyntheticBridgeDataset(c, 4, seed=9)))
    before = [x.clone() for x in _comps(a)]
    _one_update(a, batch, 5)  # a's third update: the uninterrupted run
    _one_update(b, batch, 5)
    check()
    assert any(not torch.equal(_bits(x), _bits(y)) for x, y in zip(before, _comps(a)))  # the third update moved comp


def test_default_agent_rounds_to_nearest():
    from src.agent.train import TrainAgent

    a = TrainAgent(_cfg())
    assert all(o.rounding == "nearest" for o in a.optimizers)
    assert all("rounding" not in o.param_groups[0] and "seed" not in o.param_groups[0] for o in a.optimizers)
    c = _cfg()
    c["optimizer_rounding"] = "bogus"
    with pytest.raises(ValueError, match="rounding"):
        TrainAgent(c)
