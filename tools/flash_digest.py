"""SHA-256 digests of everything the fused attention entry points write, on fixed seeded inputs.

    python tools/flash_digest.py > new.txt
    PZ_LIB_PATH=libpizero_hip_parent.so python tools/flash_digest.py > parent.txt && diff parent.txt new.txt

One line per case and output (O per output group, lse, delta, dQ, dK, dV; with the key split, O is the combined
one).  Two builds of csrc/pz_flash.hip that compute the same bits print the same text, so a refactor of the kernels
is checked by a diff; the kernels use no atomics, so two runs of one build must agree too.  The cases are the
smallest that reach every kernel form of pz_flash_fwd / pz_flash_bwd and its ragged edges:

  joint layout (geometries J3 / J4 of tests/flash_ref.py: one key past a block, cnt on the 32- / 64-key edges),
  head dims 16, 32, 256 and 72: block mask on / off x soft-cap 50 / 0 x 1 / 3 output groups x key split on / off,
  backward with the workspace (dK/dV query split and its reduce).  Head 72 runs three times: step-staged
  (PZ_FLASH_RESIDENT=0), resident (PZ_FLASH_UNIT=0) and one workgroup per unit (PZ_FLASH_UNIT=1, the masked form);
  SigLIP layout (fused q|k|v rows, 3 heads x 72, 200 and 256 tokens, plain): step-staged, resident, one workgroup
  per unit (PZ_FLASH_SIG=0: the plain form) and the default route.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-pi-zero_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from flash_ref import JOINT  # noqa: E402
from pizero_native import ops  # noqa: E402

DEV = "cuda"
KNOBS = ("PZ_FLASH_RESIDENT", "PZ_FLASH_UNIT", "PZ_FLASH_SIG")


def set_env(env):
    for k in KNOBS:  # read per call by the library
        os.environ.pop(k, None)
    os.environ.update(env)


def randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def emit(name, **outs):
    torch.cuda.synchronize()
    for what, t in outs.items():
        ts = t if isinstance(t, (list, tuple)) else [t]
        h = hashlib.sha256()
        for x in ts:
            h.update(x.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
        print(f"{name} {what} {h.hexdigest()}", flush=True)


def joint(name, jid, hd, nh, mode, cap, n_groups, key_split):
    geo = JOINT[jid]
    P, C, Hc, B = geo["P"], geo["C"], geo["Hc"], len(geo["cnt"])
    L = P + C + Hc
    Lp = (L + 7) // 8 * 8
    g = torch.Generator().manual_seed(1000 * hd + 10 * nh + int(jid[1:]))
    Q, K, V = randn(g, B, L * nh, hd), randn(g, B, Lp, hd), randn(g, B, Lp, hd)
    spans = {3: [(0, P), (P, C), (P + C, Hc)], 1: [(0, L)]}[n_groups]
    Os = [torch.zeros(B * T, nh * hd, dtype=torch.bfloat16, device=DEV) for _, T in spans]
    dOs = [randn(g, B * T, nh * hd) for _, T in spans]
    groups = [(off * nh, o, T * nh * hd, hd) for (off, T), o in zip(spans, Os)]
    lse = torch.zeros(B, L * nh, device=DEV)
    delta = torch.zeros_like(lse)
    dQ, dK, dV = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
    cnt = torch.tensor(geo["cnt"], dtype=torch.int32, device=DEV)
    mask = dict(mask_mode=1, cnt=cnt, prefix=P, cond=C) if mode == 1 else {}

    def args(**kw):
        return ops.flash_args(B, 1, L * nh, L, hd, Q, (hd, L * nh * hd, 0), K, (hd, Lp * hd, 0), V, (hd, Lp * hd, 0),
                              groups, 0, lse, hd ** -0.5, cap=cap, rows_per_token=nh, **mask, **kw)

    ops.flash_fwd(args(key_split=key_split))
    emit(name, O=Os, lse=lse)
    if not key_split:  # the backward does not depend on how the forward split its keys
        ops.flash_bwd(args(dgroups=dOs, delta=delta, dq=dQ, dk=dK, dv=dV))
        emit(name, delta=delta, dQ=dQ, dK=dK, dV=dV)


def siglip(name, nh, hd, N, cap=0.0):
    B = 2
    g = torch.Generator().manual_seed(7200 + N)
    qkv = randn(g, B * N, 3 * nh * hd, scale=1.5)
    dO = randn(g, B * N, nh * hd)
    O = torch.zeros(B * N, nh * hd, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B * nh, N, device=DEV)
    delta = torch.zeros_like(lse)
    dqkv = torch.zeros_like(qkv)
    a = ops.siglip_flash_args(qkv, O, lse, B, nh, hd, N)
    a.cap = cap
    ops.flash_fwd(a)
    emit(name, O=O, lse=lse)
    a = ops.siglip_flash_args(qkv, O, lse, B, nh, hd, N, dO=dO, delta=delta, dqkv=dqkv)
    a.cap = cap
    ops.flash_bwd(a)
    emit(name, delta=delta, dqkv=dqkv)


def main():
    routes72 = [("staged", {"PZ_FLASH_RESIDENT": "0"}), ("resident", {"PZ_FLASH_UNIT": "0"}),
                ("unit", {"PZ_FLASH_UNIT": "1", "PZ_FLASH_SIG": "0"})]
    for hd, nh, routes in ((16, 2, [("staged", {})]), (32, 2, [("staged", {})]), (256, 8, [("staged", {})]),
                           (72, 2, routes72)):
        for route, env in routes:
            set_env(env)
            for jid in ("J3", "J4"):
                for mode in (1, 0):
                    for cap in (50.0, 0.0):
                        for n_groups in (1, 3):
                            for key_split in (False, True):
                                joint(f"joint-hd{hd}-{route}-{jid}-mask{mode}-cap{cap:g}-g{n_groups}-split{int(key_split)}",
                                      jid, hd, nh, mode, cap, n_groups, key_split)
    for route, env in routes72 + [("default", {})]:
        set_env(env)
        for N in (200, 256):
            siglip(f"siglip-hd72-{route}-N{N}-plain", 3, 72, N)
            if route == "unit":
                siglip(f"siglip-hd72-{route}-N{N}-cap50", 3, 72, N, cap=50.0)
    set_env({})


if __name__ == "__main__":
    main()
