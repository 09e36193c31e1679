"""pz_episode_gather_frames / pz_episode_gather_rows on the MI355X against the numpy restatement.

Both kernels only move bytes, so every comparison is bit equality (tolerance zero).  Every output is allocated inside
a larger buffer pre-filled with a guard byte, and the bands around it are checked afterwards."""

import numpy as np
import pytest
import torch

from tests import episodes_ref as R

pytestmark = pytest.mark.gpu

GUARD = 0xA5
BAND = 4096  # bytes, a multiple of 16: the output keeps the alignment of the allocation


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _guarded(shape, dtype, offset=0):
    """(view of `shape` inside a guard-filled byte buffer, the buffer, first byte, byte count); ``offset`` shifts the
    view off the 16-byte alignment"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((BAND + offset + n + BAND,), GUARD, dtype=torch.uint8, device="cuda")
    view = buf[BAND + offset: BAND + offset + n].view(dtype).view(*shape)
    return view, buf, BAND + offset, n


def _bands_intact(buf, first, n):
    return bool((buf[:first] == GUARD).all()) and bool((buf[first + n:] == GUARD).all())


def _frames(N, C, H, W, seed):
    f = np.random.default_rng(seed).integers(0, 256, (N, C, H, W, 3), dtype=np.uint8)
    f[N // 2, :, :, :, 0], f[N // 2, :, :, :, 1], f[N // 2, :, :, :, 2] = 11, 22, 33  # swapped planes would show
    return f


def _idx(N, B, seed):
    """rows with duplicates, row 0 and row N - 1 (as far as B allows), the constant frame among them"""
    r = np.random.default_rng(seed).integers(0, N, B).astype(np.int64)
    fixed = [N - 1, 0, N // 2, N - 1]
    r[: min(B, 4)] = fixed[: min(B, 4)]
    return r


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (8, 8), (33, 33), (224, 224)])
@pytest.mark.parametrize("C", [1, 2])
def test_gather_frames(hw, C):
    """(1, 1): H W < 16; (5, 7), (33, 33): H W % 16 != 0, so frame and plane bases are unaligned and the last group is
    partial; (8, 8): the vector path with four groups per plane; (224, 224): it over many blocks"""
    from pizero_native import ops

    H, W = hw
    N = 7
    frames = _frames(N, C, H, W, seed=H * 10 + C)
    store = torch.from_numpy(frames).cuda()
    for B in (1, 3, 17):
        idx = _idx(N, B, seed=B)
        want = R.gather_frames(frames, idx)
        got = ops.episode_gather_frames(store, idx)
        assert got.shape == (B * C, 3, H, W) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want), (hw, C, B)
        out, buf, first, n = _guarded((B * C, 3, H, W), torch.uint8)
        assert ops.episode_gather_frames(store, idx, out=out) is out
        assert np.array_equal(out.cpu().numpy(), want) and _bands_intact(buf, first, n), (hw, C, B)
        # the identity mode on the pre-gathered staging buffer gives the same bytes
        staged = torch.from_numpy(frames[idx]).cuda()
        assert torch.equal(ops.episode_gather_frames(staged, None), got)
    if B >= 3:
        assert (want[2 * C, 0] == 11).all() and (want[2 * C, 1] == 22).all() and (want[2 * C, 2] == 33).all()


def test_gather_frames_unaligned_buffers():
    """an aligned geometry (8 x 8) whose store or output does not start on 16 bytes takes the byte path: same bytes"""
    from pizero_native import ops

    N, C, H, W = 5, 2, 8, 8
    frames = _frames(N, C, H, W, seed=3)
    idx = _idx(N, 6, seed=1)
    want = R.gather_frames(frames, idx)
    store, sbuf, _, _ = _guarded((N, C, H, W, 3), torch.uint8, offset=3)
    store.copy_(torch.from_numpy(frames))
    assert store.data_ptr() % 16 != 0
    assert np.array_equal(ops.episode_gather_frames(store, idx).cpu().numpy(), want)
    out, buf, first, n = _guarded((6 * C, 3, H, W), torch.uint8, offset=5)
    ops.episode_gather_frames(torch.from_numpy(frames).cuda(), idx, out=out)
    assert np.array_equal(out.cpu().numpy(), want) and _bands_intact(buf, first, n)


LENGTHS = (1, 2, 5, 3)


def _rows_store(A, P, L, seed):
    g = np.random.default_rng(seed)
    N, E = sum(LENGTHS), len(LENGTHS)
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    # every value names its own row, so a value from a neighbouring episode cannot pass for the right one
    action = (np.arange(N)[:, None] * 100 + np.arange(A)[None] + g.random((N, A))).astype(np.float32)
    proprio = (-np.arange(N)[:, None] * 100 - np.arange(P)[None] - g.random((N, P))).astype(np.float32)
    tokens = g.integers(1, 1000, (E, L)).astype(np.int32)
    pad = 0
    for e in range(E):  # padding of another length per episode; episode 1 has none
        tokens[e, L - (e * 3 + 2):] = pad if e != 1 else tokens[e, 0]
    tokens[2, 1] = pad  # and a pad id in the middle
    episode_of = np.repeat(np.arange(E, dtype=np.int32), LENGTHS)
    return action, proprio, off, tokens, episode_of, pad


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("H", [1, 4, 7])
@pytest.mark.parametrize("dims", [(7, 3, 12), (3, 7, 276)])
def test_gather_rows(W, H, dims):
    """samples at every row of four episodes laid end to end (H = 7 is longer than any of them)"""
    from pizero_native import ops

    A, P, L = dims
    action, proprio, off, tokens, episode_of, pad = _rows_store(A, P, L, seed=A)
    N = len(action)
    cu = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dev = [cu(action), cu(proprio), cu(episode_of), cu(off), cu(tokens)]
    idx = np.concatenate([np.arange(N), [N - 1, 0, 3]]).astype(np.int64)
    B = len(idx)
    want = R.gather_rows(action, proprio, off, tokens, idx, W, H, pad)
    got = ops.episode_gather_rows(*dev, idx, W, H, pad)
    shapes = {"action": ((B, H, A), torch.float32), "proprio": ((B, W, P), torch.float32),
              "action_pad_mask": ((B, H), torch.uint8), "input_ids": ((B, L), torch.int64),
              "attention_mask": ((B, L), torch.int64)}
    assert set(got) == set(shapes)
    for k, (shape, dt) in shapes.items():
        assert got[k].shape == shape and got[k].dtype == dt, k
        assert np.array_equal(got[k].cpu().numpy().view(np.uint8), want[k].view(np.uint8)), k
    # no value from a neighbouring episode: the hundreds digit of every gathered value is a row of the sample's episode
    a_rows = np.floor(got["action"].cpu().numpy()[..., 0] / 100).astype(int)
    p_rows = np.floor(-got["proprio"].cpu().numpy()[..., 0] / 100).astype(int)
    for b, t in enumerate(idx):
        e = episode_of[t]
        assert ((a_rows[b] >= off[e]) & (a_rows[b] < off[e + 1])).all(), (b, t)
        assert ((p_rows[b] >= off[e]) & (p_rows[b] < off[e + 1])).all(), (b, t)
    # the masks are exact: every sample at an episode's last row has one valid action, and the pad id is not attended
    last = np.isin(idx, off[1:] - 1)
    assert (got["action_pad_mask"].cpu().numpy()[last].sum(1) == 1).all()
    assert np.array_equal(got["attention_mask"].cpu().numpy(), (tokens[episode_of[idx]] != pad).astype(np.int64))
    # into guarded buffers
    outs, bufs = {}, {}
    for k, (shape, dt) in shapes.items():
        outs[k], *bufs[k] = _guarded(shape, dt)
    ops.episode_gather_rows(*dev, idx, W, H, pad, out=outs)
    for k in shapes:
        assert torch.equal(outs[k], got[k]) and _bands_intact(*bufs[k]), k


@pytest.mark.parametrize("kind", ["bound", "gaussian"])
def test_normalise_at_load_is_normalise_after_the_gather(kind):
    """gathering from the array normalised once == normalising what is gathered from the raw array, bit for bit"""
    from pizero_native import ops

    A, P, L, W, H = 7, 7, 12, 2, 4
    action, proprio, off, tokens, episode_of, pad = _rows_store(A, P, L, seed=5)
    action, proprio = action / 100, proprio / 100  # some values inside the clip, some outside
    st = R.statistics(action, proprio, len(LENGTHS))
    keys = ("p01", "p99") if kind == "bound" else ("mean", "std")
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    sa = [cu(np.asarray(st["action"][k], np.float32)) for k in keys]
    sp = [cu(np.asarray(st["proprio"][k], np.float32)) for k in keys]
    rest = [cu(episode_of), cu(off), cu(tokens)]
    idx = np.arange(len(action), dtype=np.int64)
    raw = ops.episode_gather_rows(cu(action), cu(proprio), *rest, idx, W, H, pad)
    pre = ops.episode_gather_rows(ops.action_normalize(cu(action), *sa, kind, n_pass=1),
                                  ops.proprio_normalize(cu(proprio), *sp, kind), *rest, idx, W, H, pad)
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(pre["action"]), bits(ops.action_normalize(raw["action"], *sa, kind, n_pass=1)))
    assert torch.equal(bits(pre["proprio"]), bits(ops.proprio_normalize(raw["proprio"], *sp, kind)))
    assert torch.equal(pre["action"][..., -1], raw["action"][..., -1])  # the gripper passes through
    assert not torch.equal(pre["action"][..., 0], raw["action"][..., 0])
    # and they are the restatement's bits
    want = R.gather_rows(R.normalize_f32(action, st["action"], kind, 1), R.normalize_f32(proprio, st["proprio"], kind),
                         off, tokens, idx, W, H, pad)
    assert np.array_equal(pre["action"].cpu().numpy().view(np.int32), want["action"].view(np.int32))
    assert np.array_equal(pre["proprio"].cpu().numpy().view(np.int32), want["proprio"].view(np.int32))
