"""TrainAgent with on-device image augmentation on the MI355X, tiny model of tests/test_agents_gpu.py."""

import copy

import numpy as np
import pytest
import torch

from tests.golden.make_golden import ref_cfg
from tests.oracle_helpers import O

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    c = ref_cfg(O.TINY_DIMS)
    c.update(dict(global_batch_size=8, per_device_batch_size=4, action_lr=1e-3, vlm_lr=1e-3,
                  action_weight_decay=0.0, vlm_weight_decay=0.0, max_grad_norm=1.0, n_updates=2, log_freq=1,
                  train_vlm=True, use_bf16=True, flow_sampling="beta", load_pretrained_weights=False,
                  action_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2),
                  vlm_lr_scheduler=dict(first_cycle_steps=100, min_lr=1e-8, warmup_steps=2)))
    c.update(kw)
    return c


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _agent(val=False, **kw):
    from src.agent.train import SyntheticBridgeDataset, TrainAgent

    c = _cfg(**kw)
    torch.manual_seed(0)  # the same initial weights for every agent of this file
    return TrainAgent(c, val_dataset=SyntheticBridgeDataset(c, 4, seed=77) if val else None)


def _batch(seed=3, hw=None):
    from src.agent.train import SyntheticBridgeDataset

    b = next(iter(SyntheticBridgeDataset(_cfg(), 4, seed=seed)))
    if hw is not None:
        b["pixel_values"] = torch.randint(0, 256, (4, 3, *hw), dtype=torch.uint8,
                                          generator=torch.Generator().manual_seed(seed))
    return b


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def agent_on():
    return _agent(val=True, image_augment=True, seed=5, eval_size=4)


def test_two_updates_with_augmentation():
    """run() with image_augment: True: two updates, every micro-batch's loss finite; the draws follow cnt_batch"""
    import logging

    a = _agent(image_augment=True)
    losses = []

    class Grab(logging.Handler):
        def emit(self, rec):
            if rec.msg.startswith("Batch"):
                losses.append(float(rec.args[2]))

    lg = logging.getLogger("src.agent.train")
    h, lvl = Grab(), lg.level
    lg.addHandler(h)
    lg.setLevel(logging.INFO)
    try:
        a.run()
    finally:
        lg.removeHandler(h)
        lg.setLevel(lvl)
    assert a.cnt_update == 2 and a.cnt_batch == 4
    assert len(losses) == 4 and all(np.isfinite(x) and x > 0 for x in losses), losses


def test_preprocess_batch_augment_is_image_augment_with_the_drawn_params(agent_on):
    from pizero_native import augment as A
    from pizero_native import ops

    a, b = agent_on, _batch()
    a.cnt_batch = 6
    state = torch.get_rng_state()
    got = a.preprocess_batch(b, augment=True, sample_fm_time=False)["pixel_values"]
    assert torch.equal(torch.get_rng_state(), state)  # torch's generator is not consumed by the augmentation
    params, mask = A.draw_params(A.REFERENCE_PRIMARY, 4, seed=5, cnt_batch=6, rank=0, crop_draws="shared")
    assert (mask == 31).all()
    want = ops.image_augment(b["pixel_values"].cuda(), params, mask, channels_last=False)
    assert got.dtype == torch.bfloat16 and got.shape == (4, 3, 56, 56)
    assert torch.equal(_bits(got), _bits(want))
    again = a.preprocess_batch(b, augment=True, sample_fm_time=False)["pixel_values"]
    assert torch.equal(_bits(got), _bits(again))
    plain = a.preprocess_batch(b, sample_fm_time=False)["pixel_values"]
    assert not torch.equal(_bits(got), _bits(plain))
    a.cnt_batch = 7
    nxt = a.preprocess_batch(b, augment=True, sample_fm_time=False)["pixel_values"]
    assert not torch.equal(_bits(got), _bits(nxt))
    # the other inputs do not depend on the flag
    a.cnt_batch = 6
    torch.manual_seed(1)
    x = a.preprocess_batch(b, augment=True)
    torch.manual_seed(1)
    y = a.preprocess_batch(b)
    assert set(x) == set(y)
    for k in x:
        if k != "pixel_values":
            assert torch.equal(x[k], y[k]), k


def test_augment_from_frames_of_another_size(agent_on):
    """resize to codes first, then augment (the reference's order)"""
    from pizero_native import augment as A
    from pizero_native import ops

    a, b = agent_on, _batch(hw=(97, 131))
    a.cnt_batch = 2
    got = a.preprocess_batch(b, augment=True, sample_fm_time=False)["pixel_values"]
    codes = ops.image_resize_u8(b["pixel_values"].cuda(), 56, channels_last=False)
    params, mask = A.draw_params(A.REFERENCE_PRIMARY, 4, seed=5, cnt_batch=2, rank=0)
    assert got.shape == (4, 3, 56, 56)
    assert torch.equal(_bits(got), _bits(ops.image_augment(codes, params, mask)))
    # without the flag: today's resize + normalisation
    plain = a.preprocess_batch(b, sample_fm_time=False)["pixel_values"]
    assert torch.equal(_bits(plain), _bits(ops.image_resize_norm(b["pixel_values"].cuda(), 56, channels_last=False)))


def test_augment_refuses_normalised_pixels_and_a_config_without_the_key(agent_on):
    b = _batch()
    b["pixel_values"] = (b["pixel_values"].float() / 255 - 0.5) / 0.5
    with pytest.raises(ValueError, match="uint8"):
        agent_on.preprocess_batch(b, augment=True)
    off = _agent()
    assert off.image_augment is False
    with pytest.raises(ValueError, match="image_augment"):
        off.preprocess_batch(_batch(), augment=True)
    with pytest.raises(ValueError, match="augment_order"):
        _agent(image_augment=True, image_augment_kwargs={"augment_order": ["random_hue", "random_brightness"],
                                                         "random_hue": [0.05], "random_brightness": [0.1]})
    with pytest.raises(ValueError, match="image_augment_crop_draws"):
        _agent(image_augment=True, image_augment_crop_draws="both")


def test_default_path_and_evaluate_do_not_depend_on_the_key(agent_on):
    off = _agent(val=True, seed=5, eval_size=4)
    for b in (_batch(), _batch(hw=(37, 53))):
        torch.manual_seed(2)
        x = agent_on.preprocess_batch(copy.deepcopy(b))
        torch.manual_seed(2)
        y = off.preprocess_batch(copy.deepcopy(b))
        for k in x:
            assert torch.equal(x[k], y[k]), k
    sa, sb = agent_on.model.state_dict(), off.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)  # neither agent has trained
    torch.manual_seed(11)
    ra = agent_on.evaluate()
    torch.manual_seed(11)
    rb = off.evaluate()
    assert (ra["l1"], ra["accuracy"]) == (rb["l1"], rb["accuracy"]) and np.isfinite(ra["l1"])
