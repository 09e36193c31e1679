"""The episode store, its statistics, the sampler and the wrappers' host checks, without a GPU."""

import json
import os
import re

import numpy as np
import pytest
import torch

from tests import episodes_ref as R
from tests.conftest import ROOT

LENGTHS = (1, 2, 5, 3, 4, 6, 2, 3)
KW = dict(cameras=1, action_dim=7, proprio_dim=7, token_len=12, image_tokens=4, image_token_index=1000,
          vocab_size=1024)


def _episodes(lengths=LENGTHS, hw=(5, 7), unlabeled=(), big_action=(), **kw):
    from src.data.episode_store import synthetic_episode

    eps = []
    for e, T in enumerate(lengths):
        ep = synthetic_episode(e, T, *hw, labeled=e not in unlabeled, **{**KW, **kw})
        if e in big_action:
            ep["action"][T // 2, 2] = -9.0
        eps.append(ep)
    return eps


def _write(path, eps, **kw):
    from src.data.episode_store import EpisodeStore, EpisodeStoreWriter

    w = EpisodeStoreWriter(path, **kw)
    for ep in eps:
        w.add_episode(**ep)
    w.close()
    return EpisodeStore(path)


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    eps = _episodes(unlabeled=(3,), big_action=(5,))
    # 5 * 7 * 3 = 105 bytes per frame: 600-byte shards hold five frames, so the store has several shards
    return _write(tmp_path_factory.mktemp("store"), eps, shard_bytes=600), eps


def test_round_trip(store):
    s, eps = store
    N = sum(LENGTHS)
    assert (s.num_episodes, s.num_transitions) == (len(LENGTHS), N)
    assert s.frame_shape == (1, 5, 7, 3) and (s.action_dim, s.proprio_dim, s.token_len) == (7, 7, 12)
    assert s.episode_offsets.dtype == np.int64
    assert s.episode_offsets.tolist() == [0] + np.cumsum(LENGTHS).tolist()
    assert len(s.shards) > 2 and sum(a.shape[0] for a in s.shards) == N
    assert all(isinstance(a, np.memmap) for a in s.shards)
    firsts = [int(x["first_row"]) for x in s.meta["shards"]]
    assert set(firsts) <= set(s.episode_offsets.tolist())  # a shard never splits an episode
    assert np.array_equal(s.action, np.concatenate([e["action"] for e in eps]))
    assert np.array_equal(s.proprio, np.concatenate([e["proprio"] for e in eps]))
    assert np.array_equal(s.input_ids, np.stack([e["input_ids"] for e in eps]))
    frames = np.concatenate([e["frames"] for e in eps])
    assert np.array_equal(s.read_frames(np.arange(N)), frames)
    rows = np.asarray([N - 1, 0, 7, 7, 3], np.int64)
    assert np.array_equal(s.read_frames(rows), frames[rows])
    assert s.labeled.tolist() == [e != 3 for e in range(len(LENGTHS))]
    assert s.episode_of.tolist() == [e for e, T in enumerate(LENGTHS) for _ in range(T)]
    # an unlabelled episode: nothing between BOS and the padding
    assert (s.input_ids[3, 5:] == 0).all() and s.input_ids[3, 4] == 2 and (s.input_ids[0, 5:] != 0).any()


def test_statistics_are_numpy_on_the_concatenated_arrays(store):
    s, eps = store
    a, p = np.concatenate([e["action"] for e in eps]), np.concatenate([e["proprio"] for e in eps])
    want = R.statistics(a, p, len(eps))
    got = json.load(open(os.path.join(s.path, "statistics.json")))
    assert got == json.loads(json.dumps(want))  # the same doubles, every one
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "bridge_statistics.json")))
    assert list(got) == list(gold) and list(got["action"]) == list(gold["action"])
    assert list(got["proprio"]) == list(gold["proprio"])
    assert got["num_transitions"] == sum(LENGTHS) and got["num_trajectories"] == len(LENGTHS)
    assert len(got["action"]["p99"]) == 7
    # the statistics cover the whole store, the filtered episode (|action| = 9) included
    assert min(got["action"]["min"]) == -9.0


def test_writer_refusals(tmp_path):
    from src.data.episode_store import EpisodeStoreWriter

    ep = _episodes((3,))[0]
    w = EpisodeStoreWriter(tmp_path / "a")
    with pytest.raises(ValueError, match="ragged"):
        w.add_episode(ep["frames"][:2], ep["action"], ep["proprio"], ep["input_ids"])
    with pytest.raises(ValueError, match="ragged"):
        w.add_episode(ep["frames"], ep["action"], ep["proprio"][:1], ep["input_ids"])
    with pytest.raises(ValueError, match="empty"):
        w.add_episode(ep["frames"][:0], ep["action"][:0], ep["proprio"][:0], ep["input_ids"])
    for key, bad in (("frames", ep["frames"].astype(np.int16)), ("action", ep["action"].astype(np.float64)),
                     ("proprio", ep["proprio"].astype(np.float16)), ("input_ids", ep["input_ids"].astype(np.int64)),
                     ("action", ep["action"].tolist())):
        with pytest.raises(ValueError, match="dtype"):
            w.add_episode(**{**ep, key: bad})
    with pytest.raises(ValueError, match="no episode"):
        EpisodeStoreWriter(tmp_path / "empty").close()
    w.add_episode(**ep)
    with pytest.raises(ValueError, match="differ"):
        w.add_episode(**_episodes((2,), hw=(6, 7))[0])
    with pytest.raises(ValueError, match="differ"):
        w.add_episode(**_episodes((2,), action_dim=6)[0])
    w.close()
    with pytest.raises(ValueError, match="twice"):
        w.close()
    with pytest.raises(ValueError, match="after close"):
        w.add_episode(**ep)
    with pytest.raises(ValueError, match="already holds"):
        EpisodeStoreWriter(tmp_path / "a")


def test_store_refusals(tmp_path):
    import shutil

    from src.data.episode_store import EpisodeStore

    good = _write(tmp_path / "good", _episodes((2, 3, 1)), shard_bytes=300)

    def broken(name):
        shutil.copytree(good.path, tmp_path / name)
        return str(tmp_path / name)

    p = broken("offsets_not_monotone")
    np.save(os.path.join(p, "episode_offsets.npy"), np.asarray([0, 5, 5, 6], np.int64))
    with pytest.raises(ValueError, match="rise strictly"):
        EpisodeStore(p)
    p = broken("offsets_end")
    np.save(os.path.join(p, "episode_offsets.npy"), np.asarray([0, 2, 5, 7], np.int64))
    with pytest.raises(ValueError, match="rise strictly"):
        EpisodeStore(p)
    p = broken("shard_rows")
    m = json.load(open(os.path.join(p, "meta.json")))
    last = m["shards"][-1]
    np.save(os.path.join(p, last["file"]), np.zeros((last["rows"] + 1, 1, 5, 7, 3), np.uint8))
    with pytest.raises(ValueError, match="must be uint8"):
        EpisodeStore(p)
    p = broken("shard_missing_rows")
    m = json.load(open(os.path.join(p, "meta.json")))
    m["shards"] = m["shards"][:-1]
    json.dump(m, open(os.path.join(p, "meta.json"), "w"))
    with pytest.raises(ValueError, match="frame shards hold"):
        EpisodeStore(p)
    p = broken("no_action")
    os.remove(os.path.join(p, "action.npy"))
    with pytest.raises(ValueError, match="action.npy is missing"):
        EpisodeStore(p)
    p = broken("action_dtype")
    np.save(os.path.join(p, "action.npy"), good.action.astype(np.float64))
    with pytest.raises(ValueError, match="action.npy must be float32"):
        EpisodeStore(p)
    # against the config it is used with
    good.check_dims(7, 7, 12, 1)
    for dims in ((6, 7, 12, 1), (7, 8, 12, 1), (7, 7, 276, 1), (7, 7, 12, 2)):
        with pytest.raises(ValueError, match="do not match"):
            good.check_dims(*dims)


# ---- chunking --------------------------------------------------------------------------------------------------------
def test_index_rules_by_hand():
    from pizero_native.episodes import chunk_rows

    # (t, s, e, W, H) -> (obs rows, action rows, pad mask), written out by hand
    cases = {
        (10, 10, 11, 1, 1): ([10], [10], [1]),  # an episode of one step
        (10, 10, 11, 2, 4): ([10, 10], [10, 10, 10, 10], [1, 0, 0, 0]),
        (4, 4, 6, 1, 4): ([4], [4, 5, 5, 5], [1, 1, 0, 0]),  # two steps
        (5, 4, 6, 2, 4): ([4, 5], [5, 5, 5, 5], [1, 0, 0, 0]),
        (5, 4, 6, 2, 1): ([4, 5], [5], [1]),
        (4, 4, 6, 2, 1): ([4, 4], [4], [1]),
        (0, 0, 5, 2, 4): ([0, 0], [0, 1, 2, 3], [1, 1, 1, 1]),  # five steps
        (1, 0, 5, 2, 4): ([0, 1], [1, 2, 3, 4], [1, 1, 1, 1]),
        (2, 0, 5, 1, 4): ([2], [2, 3, 4, 4], [1, 1, 1, 0]),
        (4, 0, 5, 2, 4): ([3, 4], [4, 4, 4, 4], [1, 0, 0, 0]),
        (4, 0, 5, 1, 1): ([4], [4], [1]),
        (7, 3, 8, 2, 4): ([6, 7], [7, 7, 7, 7], [1, 0, 0, 0]),  # five steps that do not start at row 0
        (3, 3, 8, 2, 4): ([3, 3], [3, 4, 5, 6], [1, 1, 1, 1]),
    }
    for (t, s, e, W, H), (obs, act, mask) in cases.items():
        o, a, m = chunk_rows(t, s, e, W, H)
        assert (o.tolist(), a.tolist(), m.astype(int).tolist()) == (obs, act, mask), (t, s, e, W, H)
        ro, ra, rm = R.sample_rows(t, s, e, W, H)
        assert (ro, ra, [int(x) for x in rm]) == (obs, act, mask), (t, s, e, W, H)


# ---- sampler ---------------------------------------------------------------------------------------------------------
def _sampler(s, B=4, seed=3, rank=0, world=1, **filters):
    from pizero_native.augment import EPISODE_STREAM
    from pizero_native.episodes import EpisodeSampler

    return EpisodeSampler(s.episode_offsets, s.eligible_episodes(**filters), B, seed, rank, world, EPISODE_STREAM)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sampler_epoch(store, world):
    from pizero_native.augment import EPISODE_STREAM

    s, _ = store
    off = s.episode_offsets
    ok = R.eligible(off, s.labeled, s.action, s.proprio)
    n = R.epoch_length(off, ok, world)
    seen = []
    for rank in range(world):
        sm = _sampler(s, rank=rank, world=world)
        rows = sm.epoch(0)
        own = R.rank_frames(off, ok, rank, world)
        assert sm.frames_per_epoch == n and len(rows) == n
        assert len(set(rows.tolist())) == n  # without replacement
        assert set(rows.tolist()) <= set(own)
        assert sm.episodes.tolist() == R.rank_episodes(ok, rank, world)
        assert rows.tolist() == R.epoch_rows(off, ok, 3, 0, rank, world, EPISODE_STREAM)
        seen.append(set(sm.episodes.tolist()))
    for i in range(world):
        for j in range(i + 1, world):
            assert not seen[i] & seen[j]
    assert set().union(*seen) == set(range(len(LENGTHS)))


def test_sampler_seek_straddle_seed_rank_and_global_generators(store):
    from pizero_native.augment import EPISODE_STREAM, EPISODE_VAL_STREAM, PREFIX_STREAM

    s, _ = store
    assert len({0, EPISODE_STREAM, EPISODE_VAL_STREAM, PREFIX_STREAM}) == 4
    ts, ns = torch.get_rng_state(), np.random.get_state()
    B = 5
    sm = _sampler(s, B=B, world=2, rank=1)
    n = sm.frames_per_epoch
    assert n == 12  # rank 0's episodes 0, 2, 4, 6 hold 1 + 5 + 4 + 2 frames, rank 1's 14: some batch of 5 straddles
    run = [sm.batch(k) for k in range(3 * n // B + 2)]
    straddling = [k for k in range(len(run)) if (k * B) // n != (k * B + B - 1) // n]
    assert straddling
    ok = R.eligible(s.episode_offsets, s.labeled, s.action, s.proprio)
    for k in [0, 1, straddling[0], straddling[-1], len(run) - 1]:
        fresh = _sampler(s, B=B, world=2, rank=1)  # nothing cached: as after a seek in a new process
        assert np.array_equal(fresh.batch(k), run[k]), k
        assert np.array_equal(run[k], R.batch_rows(s.episode_offsets, ok, 3, k, 1, 2, B, EPISODE_STREAM)), k
    flat = np.concatenate(run)
    assert np.array_equal(flat[:n], sm.epoch(0)) and np.array_equal(flat[n: 2 * n], sm.epoch(1))
    assert not np.array_equal(sm.epoch(0), sm.epoch(1))
    assert not np.array_equal(_sampler(s, B=B, seed=4, world=2, rank=1).batch(0), run[0])
    from pizero_native.augment import generator

    draws = [generator(3, 0, r, stream=st).permutation(14).tolist()
             for r, st in ((0, EPISODE_STREAM), (1, EPISODE_STREAM), (1, EPISODE_VAL_STREAM))]
    assert draws[0] != draws[1] and draws[1] != draws[2]  # another rank, another stream: other draws
    one = _sampler(s, world=1)
    assert not np.array_equal(one.epoch(0), _sampler(s, world=1, seed=5).epoch(0))
    assert torch.equal(torch.get_rng_state(), ts)
    ns2 = np.random.get_state()
    assert ns[0] == ns2[0] and np.array_equal(ns[1], ns2[1]) and ns[2:] == ns2[2:]


def test_filters(store):
    s, _ = store
    ok = s.eligible_episodes(skip_unlabeled=True, max_action=3.0)
    assert ok.tolist() == R.eligible(s.episode_offsets, s.labeled, s.action, s.proprio, True, 3.0)
    assert ok.tolist() == [e not in (3, 5) for e in range(len(LENGTHS))]
    sm = _sampler(s, skip_unlabeled=True, max_action=3.0)
    rows = np.concatenate([sm.epoch(j) for j in range(3)])
    assert not set(s.episode_of[rows].tolist()) & {3, 5}
    assert s.eligible_episodes().all()  # validation does not filter by label unless asked
    assert s.eligible_episodes(max_proprio=2.5).all() and not s.eligible_episodes(max_proprio=1e-3).any()
    with pytest.raises(ValueError, match="no eligible episode"):
        _sampler(s, max_action=1e-3)
    with pytest.raises(ValueError, match="cannot be dealt"):
        _sampler(s, world=7, rank=0, skip_unlabeled=True, max_action=3.0)


# ---- ABI and wrappers ------------------------------------------------------------------------------------------------
def test_abi_still_22_and_new_symbols():
    import pizero_native
    from pizero_native._lib import ABI_VERSION, SIGNATURES

    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    assert ABI_VERSION == 22 and "#define PZ_ABI_VERSION 22" in hdr
    L = pizero_native.lib()
    assert L.pz_abi_version() == 22
    for sym in ("pz_episode_gather_frames", "pz_episode_gather_rows"):
        assert re.search(rf"\bint {sym}\(", hdr), sym
        assert hasattr(L, sym) and sym in SIGNATURES
    assert len(SIGNATURES["pz_episode_gather_frames"]) == 9 and len(SIGNATURES["pz_episode_gather_rows"]) == 21
    # the C entry points refuse bad dimensions and null pointers before any launch (no device needed)
    assert L.pz_episode_gather_frames(None, 4, 1, 8, 8, None, 2, None, None) == 1
    assert b"null pointer" in L.pz_last_error()
    buf = np.zeros(64, np.uint8).ctypes.data
    assert L.pz_episode_gather_frames(buf, 4, 1, 0, 8, None, 2, buf, None) == 1
    assert b"must be positive" in L.pz_last_error()
    assert L.pz_episode_gather_frames(buf, 4, 1, 8, 8, None, 5, buf, None) == 1
    assert b"identity" in L.pz_last_error()
    assert L.pz_episode_gather_rows(buf, buf, buf, buf, buf, None, 4, 2, 7, 7, 12, 2, 1, 4, 0, buf, buf, buf, buf, buf,
                                    None) == 1
    assert b"null input" in L.pz_last_error()
    assert L.pz_episode_gather_rows(buf, buf, buf, buf, buf, buf, 4, 2, 7, 7, 12, 2, 0, 4, 0, buf, buf, buf, buf, buf,
                                    None) == 1
    assert b"must lie in" in L.pz_last_error()


def test_wrappers_refuse_on_the_host(monkeypatch):
    """every refusal below is raised before anything is uploaded or launched: the tensors are host tensors, and the
    native call is replaced by one that fails the test"""
    from pizero_native import ops

    def no_launch(*a, **k):
        raise AssertionError("reached the native call")

    monkeypatch.setattr(ops, "call", no_launch)
    N, E, A, P, L = 6, 2, 7, 3, 12
    store = torch.zeros(N, 2, 4, 4, 3, dtype=torch.uint8)
    i64 = lambda *v: np.asarray(v, np.int64)  # noqa: E731
    for bad in (i64(0, N), i64(-1, 2), i64(2 ** 40)):
        with pytest.raises(ValueError, match=r"must lie in \[0, 6\)"):
            ops.episode_gather_frames(store, bad)
    for bad in (np.asarray([0, 1], np.int32), [0, 1], torch.tensor([0, 1]), i64(), np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError, match="int64 numpy"):
            ops.episode_gather_frames(store, bad)
    with pytest.raises(ValueError, match="contiguous torch.uint8"):
        ops.episode_gather_frames(store.float(), i64(0))
    with pytest.raises(ValueError, match="contiguous torch.uint8"):
        ops.episode_gather_frames(store.permute(0, 1, 3, 2, 4), i64(0))
    with pytest.raises(ValueError, match=r"\[N, C, H, W, 3\]"):
        ops.episode_gather_frames(torch.zeros(N, 2, 4, 3, 4, dtype=torch.uint8), i64(0))
    with pytest.raises(ValueError, match="out must have shape"):  # short output
        ops.episode_gather_frames(store, i64(0, 1), out=torch.zeros(3, 3, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="must be in the memory of"):  # all else in order: only the device is missing
        ops.episode_gather_frames(store, i64(0, 1))

    act, pro = torch.zeros(N, A), torch.zeros(N, P)
    eo, off = torch.zeros(N, dtype=torch.int32), torch.tensor([0, 2, N])
    tok = torch.zeros(E, L, dtype=torch.int32)
    args = lambda **k: {**dict(action=act, proprio=pro, episode_of=eo, episode_offsets=off, tokens=tok,  # noqa: E731
                               idx=i64(0, 5), window=1, horizon=4, pad_id=0), **k}
    for bad in (i64(0, N), i64(-1)):
        with pytest.raises(ValueError, match=r"must lie in \[0, 6\)"):
            ops.episode_gather_rows(**args(idx=bad))
    with pytest.raises(ValueError, match="int64 numpy"):
        ops.episode_gather_rows(**args(idx=np.asarray([0.0])))
    for key, bad in (("action", act.double()), ("proprio", pro.half()), ("episode_of", eo.long()),
                     ("episode_offsets", off.int()), ("tokens", tok.long())):
        with pytest.raises(ValueError, match=f"{key} must be a contiguous"):
            ops.episode_gather_rows(**args(**{key: bad}))
    with pytest.raises(ValueError, match="proprio must have shape"):
        ops.episode_gather_rows(**args(proprio=torch.zeros(N - 1, P)))
    with pytest.raises(ValueError, match="E \\+ 1"):
        ops.episode_gather_rows(**args(episode_offsets=torch.tensor([0, N])))
    with pytest.raises(ValueError, match="window and horizon"):
        ops.episode_gather_rows(**args(horizon=0))
    good = {"action": torch.zeros(2, 4, A), "proprio": torch.zeros(2, 1, P),
            "action_pad_mask": torch.zeros(2, 4, dtype=torch.uint8), "input_ids": torch.zeros(2, L, dtype=torch.int64),
            "attention_mask": torch.zeros(2, L, dtype=torch.int64)}
    with pytest.raises(ValueError, match="must have shape"):  # short output
        ops.episode_gather_rows(**args(out={**good, "action": torch.zeros(2, 3, A)}))
    with pytest.raises(ValueError, match="must be a contiguous torch.int64"):
        ops.episode_gather_rows(**args(out={**good, "input_ids": torch.zeros(2, L, dtype=torch.int32)}))
    with pytest.raises(ValueError, match="exactly"):
        ops.episode_gather_rows(**args(out={k: v for k, v in good.items() if k != "proprio"}))
    with pytest.raises(ValueError, match="must be in the memory of"):
        ops.episode_gather_rows(**args(out=good))


# ---- config and tool -------------------------------------------------------------------------------------------------
def test_config_refusals_and_bridge_yaml(store, tmp_path):
    from pizero_native.episodes import IGNORED_KEYS, REFUSED_KEYS, from_config
    from src.utils.config import cfg_get, load_config

    s, _ = store
    base = dict(cond_steps=1, horizon_steps=4, action_dim=7, proprio_dim=7, max_seq_len=12, num_images=1, seed=1,
                pad_token_id=0)
    cfg = lambda **k: {**base, "data": {"train": {"episode_store": s.path, **k}}}  # noqa: E731
    assert from_config(base, "train", 4, 0, 1, "cpu") is None
    assert from_config({**base, "data": {"train": {"episode_store": None}}}, "train", 4, 0, 1, "cpu") is None
    assert from_config(cfg(), "val", 4, 0, 1, "cpu") is None
    assert "goal_relabeling_strategy" in REFUSED_KEYS and "subsample_length" in REFUSED_KEYS
    for key in REFUSED_KEYS:
        with pytest.raises(ValueError, match=key):
            from_config(cfg(**{key: "uniform"}), "train", 4, 0, 1, "cpu")
    with pytest.raises(ValueError, match="dataset_mix"):
        from_config(cfg(dataset_mix=["bridge", "fractal"]), "train", 4, 0, 1, "cpu")
    with pytest.raises(ValueError, match="window_size"):
        from_config(cfg(window_size=2), "train", 4, 0, 1, "cpu")
    with pytest.raises(ValueError, match="action_horizon"):
        from_config(cfg(action_horizon=8), "train", 4, 0, 1, "cpu")
    with pytest.raises(ValueError, match="do not match"):
        from_config({**cfg(), "max_seq_len": 276}, "train", 4, 0, 1, "cpu")
    with pytest.raises(ValueError, match="do not match"):
        from_config({**cfg(), "num_images": 2}, "train", 4, 0, 1, "cpu")
    with pytest.raises(ValueError, match="pad token"):
        from_config({**cfg(), "pad_token_id": 1}, "train", 4, 0, 1, "cpu")
    assert "traj_transform_threads" in IGNORED_KEYS
    # bridge.yaml: no data node is resolved (the keys are there as comments), so nothing bench.py reads has changed
    os.environ.setdefault("VLA_LOG_DIR", "x")
    os.environ.setdefault("TRANSFORMERS_CACHE", "x")
    path = os.path.join(ROOT, "open-pi-zero_amd", "config", "train", "bridge.yaml")
    y = load_config(path)
    assert cfg_get(y, "data") is None and cfg_get(y, "data.train.episode_store") is None
    text = open(path).read()
    for key in ("episode_store", "frames_placement", "device_store_max_gb", "skip_unlabeled", "max_action",
                "action_normalization_type", "window_size", "action_horizon"):
        assert re.search(rf"^#\s+{key}:", text, flags=re.M), key


def test_make_episode_store_tool(tmp_path):
    import importlib.util

    from src.data.episode_store import EpisodeStore

    spec = importlib.util.spec_from_file_location("make_episode_store",
                                                  os.path.join(ROOT, "tools", "make_episode_store.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    eps = _episodes((2, 3, 1), unlabeled=(1,))
    os.makedirs(tmp_path / "in")
    for i, ep in enumerate(eps):
        np.savez(tmp_path / "in" / f"ep_{i:03d}.npz", **ep)
    assert tool.main([str(tmp_path / "in"), str(tmp_path / "out")]) == 0
    s = EpisodeStore(tmp_path / "out")
    assert s.num_episodes == 3 and s.labeled.tolist() == [True, False, True]
    assert np.array_equal(s.read_frames(np.arange(6)), np.concatenate([e["frames"] for e in eps]))
    args = ["--synthetic", "5,2,4,8,8", "--token-len", "12", "--image-tokens", "4", "--image-token-index", "1000",
            "--vocab-size", "1024", "--unlabeled-every", "2"]
    assert tool.main(args + [str(tmp_path / "syn")]) == 0
    assert tool.main(args + [str(tmp_path / "syn2")]) == 0
    a, b = EpisodeStore(tmp_path / "syn"), EpisodeStore(tmp_path / "syn2")
    assert a.num_episodes == 5 and a.frame_shape == (1, 8, 8, 3) and a.labeled.tolist() == [1, 0, 1, 0, 1]
    assert 2 <= np.diff(a.episode_offsets).min() and np.diff(a.episode_offsets).max() <= 4
    assert np.array_equal(a.action, b.action) and np.array_equal(a.read_frames(np.arange(3)), b.read_frames(np.arange(3)))
