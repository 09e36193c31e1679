"""EpisodeBatches and TrainAgent on an episode store on the MI355X: tiny model of tests/test_agents_gpu.py,
a synthetic store of a dozen short episodes at the tiny config's image size (56 x 56) and one at 40 x 48."""

import threading

import numpy as np
import pytest
import torch

from tests import episodes_ref as R
from tests.golden.make_golden import ref_cfg
from tests.oracle_helpers import O

pytestmark = pytest.mark.gpu

LENGTHS = (3, 5, 2, 6, 4, 1, 5, 3, 2, 4, 6, 3)
KEYS = ("input_ids", "attention_mask", "pixel_values", "proprio", "action", "action_pad_mask")


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


def _make_store(path, hw):
    from src.data.episode_store import EpisodeStore, EpisodeStoreWriter, synthetic_episode

    d = O.TINY_DIMS
    # shards of at most ~8 frames, so the host placement gathers across shards
    w = EpisodeStoreWriter(path, shard_bytes=8 * hw[0] * hw[1] * 3)
    for e, T in enumerate(LENGTHS):
        w.add_episode(**synthetic_episode(e, T, *hw, token_len=d["max_seq_len"], image_tokens=d["num_image_tokens"],
                                          image_token_index=d["image_token_index"], vocab_size=d["vocab_size"],
                                          labeled=e != 4))
    w.close()
    return EpisodeStore(path)


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    return _make_store(tmp_path_factory.mktemp("store56"), (56, 56))


@pytest.fixture(scope="module")
def store_other(tmp_path_factory):
    return _make_store(tmp_path_factory.mktemp("store40"), (40, 48))


def _ref_rows(store, k, B, seed, stream=None, **filters):
    from pizero_native.augment import EPISODE_STREAM

    ok = R.eligible(store.episode_offsets, store.labeled, store.action, store.proprio, **filters)
    return R.batch_rows(store.episode_offsets, ok, seed, k, 0, 1, B, EPISODE_STREAM if stream is None else stream)


def _workers():
    from pizero_native.episodes import WORKER_NAME

    return [t for t in threading.enumerate() if t.name == WORKER_NAME and t.is_alive()]


def _same(batch, want):
    for k in KEYS:
        got = batch[k]
        assert got.is_cuda, k
        g = got.cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (k, g.dtype, g.shape)
        assert np.array_equal(g.view(np.uint8), want[k].view(np.uint8)), k


@pytest.mark.parametrize("window,kind", [(1, "bound"), (2, "gaussian")])
def test_batches_are_the_restatement_in_both_placements(store, window, kind):
    from pizero_native.episodes import EpisodeBatches

    kw = dict(seed=7, skip_unlabeled=True, action_normalization_type=kind, proprio_normalization_type=kind)
    B, n = 5, sum(T for e, T in enumerate(LENGTHS) if e != 4)
    served = {}
    for placement in ("device", "host"):
        with EpisodeBatches(store, B, window, 4, "cuda", frames_placement=placement, **kw) as eb:
            assert eb.frames_placement == placement and eb.sampler.frames_per_epoch == n
            it = iter(eb)
            served[placement] = [next(it) for _ in range(n // B + 2)]  # past the end of the first epoch
            assert [k for k, _ in eb.recent] == list(range(n // B + 2))
            for k, batch in enumerate(served[placement]):
                rows = _ref_rows(store, k, B, 7, skip_unlabeled=True)
                assert np.array_equal(eb.recent[k][1], rows)
                assert 4 not in store.episode_of[rows]
                _same(batch, R.batch(store, rows, window, 4, kind, kind, n_pass=1))
            # seek: micro-batch 3 again, then 1, through the prefetch
            for k in (3, 1, 2):
                eb.seek(k)
                again = next(it)
                for key in KEYS:
                    assert torch.equal(again[key], served[placement][k][key]), (placement, k, key)
        assert not _workers()
    for a, b in zip(served["device"], served["host"]):
        for key in KEYS:
            assert torch.equal(a[key], b[key]), key


def test_placement_cap_and_auto(store):
    from pizero_native.episodes import EpisodeBatches

    need = store.num_transitions * 56 * 56 * 3
    with pytest.raises(ValueError, match=rf"{need} bytes.*allows {need - 1000} bytes"):
        EpisodeBatches(store, 4, 1, 4, "cuda", frames_placement="device", device_store_max_gb=(need - 1000) / 1e9)
    with pytest.raises(ValueError, match="frames_placement must be one of"):
        EpisodeBatches(store, 4, 1, 4, "cuda", frames_placement="disk")
    small = EpisodeBatches(store, 4, 1, 4, "cuda", device_store_max_gb=(need - 1000) / 1e9)
    assert small.frames_placement == "host" and EpisodeBatches(store, 4, 1, 4, "cuda").frames_placement == "device"
    small.close()


class _Rec:
    """stands in for TrainAgent.model_meta: records every micro-batch's loss"""

    def __init__(self, m):
        self.m, self.losses = m, []

    def __call__(self, **kw):
        loss = self.m(**kw)
        self.losses.append(loss.detach().float().reshape(1).clone())
        return loss

    def __getattr__(self, k):
        return getattr(self.m, k)


def _agent(dataset=None, reseed=False, **kw):
    from src.agent.train import TrainAgent

    torch.manual_seed(0)  # the same initial weights for every agent of this file
    a = TrainAgent(_cfg(**kw), dataset=dataset)
    a.model_meta = _Rec(a.model_meta)
    if reseed:  # the flow-matching times of micro-batch k do not depend on where the process started
        inner = a.preprocess_batch

        def preprocess(batch, **k):
            torch.manual_seed(100 + a.micro_batches_seen)
            return inner(batch, **k)

        a.preprocess_batch = preprocess
    return a


def _losses(a):
    return torch.cat(a.model_meta.losses).cpu()


class _HostDataset:
    """a plain Python dataset: the restatement's batches, as host tensors"""

    def __init__(self, store, B, seed):
        self.store, self.B, self.seed = store, B, seed

    def __iter__(self):
        k = 0
        while True:
            b = R.batch(self.store, _ref_rows(self.store, k, self.B, self.seed), 1, 4)
            yield {key: torch.from_numpy(v) for key, v in b.items()}
            k += 1


@pytest.mark.parametrize("placement", ["device", "host"])
def test_training_from_the_store_is_training_on_its_batches(store, placement):
    """two updates (four micro-batches) from data.train.episode_store against the same agent fed the restatement's
    batches from the host: the same loss bits, micro-batch by micro-batch -- the wiring adds nothing else"""
    from pizero_native.episodes import EpisodeBatches

    a = _agent(seed=11, data=dict(train=dict(episode_store=store.path, frames_placement=placement)))
    assert isinstance(a.train_dataloader, EpisodeBatches) and a.train_dataloader.frames_placement == placement
    a.run()
    b = _agent(seed=11, dataset=_HostDataset(store, 4, seed=11))
    b.run()
    la, lb = _losses(a), _losses(b)
    assert len(la) == 4 and torch.isfinite(la).all() and a.cnt_update == 2
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), (la, lb)
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not _workers()  # run() joined the host placement's worker


def test_augmentation_from_a_store_at_another_resolution(store_other):
    a = _agent(image_augment=True, data=dict(train=dict(episode_store=store_other.path, seed=3)))
    a.run()
    la = _losses(a)
    assert len(la) == 4 and torch.isfinite(la).all() and (la > 0).all()
    # and without the augmentation: preprocess_batch's resize branch takes the 40 x 48 frames
    b = _agent(data=dict(train=dict(episode_store=store_other.path, seed=3)))
    batch = next(iter(b.train_dataloader))
    assert batch["pixel_values"].shape == (4, 3, 40, 48)
    assert b.preprocess_batch(batch)["pixel_values"].shape == (4, 3, 56, 56)


@pytest.mark.parametrize("placement", ["device", "host"])
def test_resume_continues_the_sequence(store, tmp_path, placement):
    """four micro-batches uninterrupted against two, checkpoint, a new agent with resume_checkpoint_path, two more"""
    kw = dict(global_batch_size=4, per_device_batch_size=4, n_updates=4, save_model_freq=2, seed=5,
              data=dict(train=dict(episode_store=store.path, frames_placement=placement)))
    a = _agent(reseed=True, log_dir=str(tmp_path), **kw)
    a.run()
    path = tmp_path / "checkpoint" / "step2.pt"
    assert path.exists() and a.micro_batches_seen == 4
    rows_a = [r for _, r in a.train_dataloader.recent]
    b = _agent(reseed=True, resume_checkpoint_path=str(path), **kw)
    assert (b.cnt_update, b.micro_batches_seen) == (2, 2)
    b.run()
    assert [k for k, _ in b.train_dataloader.recent] == [2, 3]
    rows_b = [r for _, r in b.train_dataloader.recent]
    assert len(rows_a) == 4 and all(np.array_equal(x, y) for x, y in zip(rows_a[2:], rows_b))
    assert all(np.array_equal(rows_a[k], _ref_rows(store, k, 4, 5)) for k in range(4))
    la, lb = _losses(a), _losses(b)
    assert len(lb) == 2 and torch.equal(la[2:].view(torch.int32), lb.view(torch.int32)), (la, lb)
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_validation_from_a_store(store, store_other):
    from pizero_native.augment import EPISODE_VAL_STREAM
    from pizero_native.episodes import EpisodeBatches

    a = _agent(eval_size=4, seed=2, data=dict(train=dict(episode_store=store.path),
                                              val=dict(episode_store=store_other.path, frames_placement="host")))
    assert a.run_eval and isinstance(a.val_dataloader, EpisodeBatches) and a.last_eval is None
    r = a.evaluate()
    assert a.last_eval is r and np.isfinite(r["l1"]) and all(np.isfinite(x) for x in r["accuracy"])
    a.evaluate()
    # its own stream, its own count that goes on across evaluate() calls, no label filter unless asked
    assert [k for k, _ in a.val_dataloader.recent] == [0, 1]
    for k, rows in a.val_dataloader.recent:
        assert np.array_equal(rows, _ref_rows(store_other, k, 4, 2, stream=EPISODE_VAL_STREAM))
    assert a.val_dataloader.sampler.episodes.tolist() == list(range(len(LENGTHS)))
    a.val_dataloader.close()
    assert not _workers()


def test_defaults_without_the_key(store):
    from src.agent.train import SyntheticBridgeDataset

    for extra in ({}, {"data": {"train": {"episode_store": None}}}):
        a = _agent(**extra)
        assert isinstance(a.train_dataloader, SyntheticBridgeDataset) and not a.run_eval
    with pytest.raises(ValueError, match="window_size"):
        _agent(data=dict(train=dict(episode_store=store.path, window_size=2)))
    with pytest.raises(ValueError, match="goal_relabeling_strategy"):
        _agent(data=dict(train=dict(episode_store=store.path, goal_relabeling_strategy="uniform")))
    with pytest.raises(ValueError, match="do not match"):
        _agent(num_images=2, data=dict(train=dict(episode_store=store.path)))


def test_worker_lifecycle(store):
    from pizero_native.episodes import EpisodeBatches

    eb = EpisodeBatches(store, 4, 1, 4, "cuda", frames_placement="host")
    assert not _workers()  # started with the first batch
    next(iter(eb))
    assert len(_workers()) == 1
    eb.close()
    assert not _workers()
    next(iter(eb))  # and again after a close
    assert len(_workers()) == 1
    eb.close()
    eb.close()
    assert not _workers()
    with pytest.raises(RuntimeError, match="consumer"):
        with EpisodeBatches(store, 4, 1, 4, "cuda", frames_placement="host") as eb2:
            for i, _ in enumerate(eb2):
                if i == 1:
                    raise RuntimeError("consumer")
    assert not _workers()
    # the same through TrainAgent.run(): the step fails at the second micro-batch
    a = _agent(data=dict(train=dict(episode_store=store.path, frames_placement="host")))
    inner, calls = a.preprocess_batch, []

    def failing(batch, **k):
        calls.append(1)
        if len(calls) == 2:
            assert len(_workers()) == 1
            raise RuntimeError("consumer")
        return inner(batch, **k)

    a.preprocess_batch = failing
    with pytest.raises(RuntimeError, match="consumer"):
        a.run()
    assert not _workers()
