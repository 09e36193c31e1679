"""Build an episode store (open-pi-zero_amd/src/data/episode_store.py) for TrainAgent.

    python tools/make_episode_store.py IN_DIR OUT_DIR [--pad-token-id 0] [--shard-mb 256]
    python tools/make_episode_store.py --synthetic E,Tmin,Tmax,H,W OUT_DIR [--seed 0] [--cameras 1] ...

IN_DIR holds one ``.npz`` per episode (taken in sorted order) with
  frames     uint8 [T, C, H, W, 3] or [T, H, W, 3]       action   float32 [T, A], raw robot units
  proprio    float32 [T, P], raw robot units              input_ids int32 [L], the full model prompt, tokenised
and optionally ``labeled`` (a scalar, default true: an episode without an instruction must say ``labeled=False``, the
flag is stored, not guessed from the tokens).  Then point the config at the store:
``data.train.episode_store: OUT_DIR`` (and ``env.adapter.dataset_statistics_path: OUT_DIR/statistics.json`` for
inference with the same statistics).

``--synthetic`` writes E counter-generated episodes of Tmin..Tmax steps with H x W frames instead (tests, benchmarks).
There is no RLDS converter: reading RLDS needs TensorFlow.
"""

from __future__ import annotations

import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-pi-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("paths", nargs="+", help="IN_DIR OUT_DIR, or OUT_DIR alone with --synthetic")
    ap.add_argument("--synthetic", default=None, metavar="E,Tmin,Tmax,H,W")
    ap.add_argument("--pad-token-id", type=int, default=0)
    ap.add_argument("--shard-mb", type=float, default=256.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cameras", type=int, default=1)
    ap.add_argument("--action-dim", type=int, default=7)
    ap.add_argument("--proprio-dim", type=int, default=7)
    ap.add_argument("--token-len", type=int, default=276)
    ap.add_argument("--image-tokens", type=int, default=256)
    ap.add_argument("--image-token-index", type=int, default=257152)
    ap.add_argument("--vocab-size", type=int, default=257216)
    ap.add_argument("--unlabeled-every", type=int, default=0, help="synthetic: every n-th episode has no instruction")
    a = ap.parse_args(argv)

    import numpy as np

    from src.data.episode_store import EpisodeStore, EpisodeStoreWriter, synthetic_episode

    if (a.synthetic is None) != (len(a.paths) == 2):
        ap.error("give IN_DIR OUT_DIR, or --synthetic E,Tmin,Tmax,H,W with OUT_DIR alone")
    out = a.paths[-1]
    w = EpisodeStoreWriter(out, pad_token_id=a.pad_token_id, shard_bytes=int(a.shard_mb * (1 << 20)))
    if a.synthetic is not None:
        try:
            E, tmin, tmax, H, W = (int(x) for x in a.synthetic.split(","))
        except ValueError:
            ap.error("--synthetic takes five integers: E,Tmin,Tmax,H,W")
        if E < 1 or not 1 <= tmin <= tmax or H < 1 or W < 1:
            ap.error("--synthetic: E, H, W must be positive and 1 <= Tmin <= Tmax")
        lengths = np.random.Generator(np.random.Philox(key=a.seed)).integers(tmin, tmax + 1, E)
        for e in range(E):
            ep = synthetic_episode(e, int(lengths[e]), H, W, cameras=a.cameras, action_dim=a.action_dim,
                                   proprio_dim=a.proprio_dim, token_len=a.token_len, image_tokens=a.image_tokens,
                                   image_token_index=a.image_token_index, vocab_size=a.vocab_size,
                                   pad_token_id=a.pad_token_id, seed=a.seed,
                                   labeled=not (a.unlabeled_every and (e + 1) % a.unlabeled_every == 0))
            w.add_episode(**ep)
    else:
        files = sorted(glob.glob(os.path.join(a.paths[0], "*.npz")))
        if not files:
            raise SystemExit(f"{a.paths[0]} holds no .npz file")
        for f in files:
            with np.load(f) as z:
                missing = [k for k in ("frames", "action", "proprio", "input_ids") if k not in z]
                if missing:
                    raise SystemExit(f"{f}: missing {missing}")
                labeled = bool(z["labeled"]) if "labeled" in z else True
                try:
                    w.add_episode(z["frames"], z["action"], z["proprio"], z["input_ids"], labeled=labeled)
                except ValueError as exc:
                    raise SystemExit(f"{f}: {exc}") from None
    w.close()
    s = EpisodeStore(out)  # opens and validates what was written
    print(f"{out}: {s.num_episodes} episodes, {s.num_transitions} steps, frames {list(s.frame_shape)}, "
          f"{len(s.shards)} shard(s), action_dim {s.action_dim}, proprio_dim {s.proprio_dim}, tokens {s.token_len}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
