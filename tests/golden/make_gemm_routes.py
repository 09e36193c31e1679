"""Pin the GEMM planner's routing table: tests/golden/gemm_routes.json.

    env -i PATH=$PATH python tests/golden/make_gemm_routes.py            (no PZ_* variable set)
    env -i PATH=$PATH python tests/golden/make_gemm_routes.py --knobs    (gemm_routes_knobs.json)

--knobs sweeps the same grid once per setting of KNOBS (the planner's A/B switches) and stores, per setting, only the
routes that differ from gemm_routes.json.  Record either fixture from a build of the commit whose routes are to be
kept, never from the change under test.

pz_gemm_kernel_name is host-only logic, and without a device the planner assumes 256 compute units (the MI355X
count), so the table is the one the GPU machine routes by.  The fixture stores the axes, the unique kernel-name
strings and the routes as run-length pairs [name index, repeat, ...] in the order queries() yields them.

The sweep is the shape grid (rows x widths x depths x the four A/B layouts) at the default arguments, then one
block per further argument over the same shape grid: each epilogue on the layouts it is used with, the two fp8
modes, no workspace, batch, fp32 output and the rank extension.  Argument sets that pz_gemm rejects are skipped,
except W8A16 above 64 rows on a shape the row-slab kernel does not take: pz_gemm rejects those by the plan itself,
and test_gemm_routes_golden holds ops.rows_w8a16_ok to exactly that decision.
"""

from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "gemm_routes.json")

NONE, GELU, GEGLU, DGELU, DGEGLU = 0, 1, 2, 4, 6  # PZ_EPI_* (include/pz_abi.h)
NT, NN, TN, TT = (True, True), (True, False), (False, False), (False, True)  # (a_kcontig, b_kcontig)

AXES = {
    "M": [1, 4, 8, 16, 17, 50, 64, 65, 128, 256, 276, 320, 512, 768, 788, 789, 1024, 1025, 1280, 8192, 16384, 17664,
          35328, 70656],
    "N": [256, 520, 1000, 1024, 1152, 2048, 2560, 3456, 4096, 4304, 8192, 32768],
    "K": [320, 1024, 1152, 2048, 4096, 4304, 8192, 16384],
    "layouts": [list(NT), list(NN), list(TN), list(TT)],
    # one block per entry, each over the whole M x N x K grid: [epilogue, layouts, fp8_mode, workspace, batch,
    # c_fp32, K2]
    "blocks": [
        [NONE, [NT, NN, TN, TT], 0, True, 1, False, 0],
        [GELU, [NT], 0, True, 1, False, 0],
        [GEGLU, [NT, TT], 0, True, 1, False, 0],
        [DGELU, [NN], 0, True, 1, False, 0],
        [DGEGLU, [NN], 0, True, 1, False, 0],
        [NONE, [NT], 1, True, 1, False, 0],
        [GEGLU, [NT], 1, True, 1, False, 0],
        [NONE, [NT], 1, False, 1, False, 0],
        [NONE, [NT], 2, True, 1, False, 0],
        [GEGLU, [NT], 2, True, 1, False, 0],
        [NONE, [NT], 2, False, 1, False, 0],
        [NONE, [NT, NN, TN, TT], 0, False, 1, False, 0],
        [GEGLU, [NT], 0, False, 1, False, 0],
        [NONE, [NT, NN, TN, TT], 0, True, 8, False, 0],
        [NONE, [NT, NN, TN, TT], 0, True, 256, False, 0],
        [NONE, [NT, NN, TN, TT], 0, True, 1, True, 0],
        [NONE, [NT, NN, TN, TT], 0, True, 1, False, 16],
        [GEGLU, [NT], 0, True, 1, False, 16],
        [DGELU, [NN], 0, True, 1, False, 16],
    ],
}


# the planner's A/B switches ("Environment variables"), each swept over the whole grid by --knobs
KNOBS_OUT = os.path.join(HERE, "gemm_routes_knobs.json")
KNOBS = [
    {"PZ_GEMM_TAIL": "0"}, {"PZ_GEMM_ROWS": "0"}, {"PZ_GEMM_ROWS": "1"}, {"PZ_GEMM_TALL": "0"}, {"PZ_GEMM_TALL": "1"},
    {"PZ_ROWS_FIRST": "1"}, {"PZ_GEMV": "0"}, {"PZ_SK64_FUSED": "0"}, {"PZ_GEMV": "0", "PZ_SKINNY_MINNC": "4"},
    {"PZ_GEMV": "0", "PZ_SKINNY_MINNC": "8"}, {"PZ_ROWS_W": "4"}, {"PZ_ROWS_W": "8"}, {"PZ_ROWS_TNB": "1"},
    {"PZ_ROWS_TNB": "2"}, {"PZ_ROWS_TNB": "4"},
]


def accepted(M, N, K, akc, bkc, epi, fp8, batch, c_fp32, K2):
    """pz_gemm's argument checks, as far as the swept arguments reach them"""
    if K % 8 != 0 and (akc or bkc):
        return False
    if (not akc and M % 8 != 0) or (not bkc and N % 8 != 0):
        return False
    if epi == GEGLU and not (bkc and batch == 1 and not c_fp32 and N % 8 == 0):
        return False
    if epi != NONE and batch != 1:
        return False
    if epi >= DGELU and c_fp32:
        return False
    if fp8 and not (akc and bkc and batch == 1 and K2 == 0):
        return False
    if fp8 == 1 and not (epi <= GEGLU and K % 16 == 0):
        return False
    if fp8 == 2 and not (K % 64 == 0 and not c_fp32 and epi < DGELU):
        return False
    if K2 and batch != 1:
        return False
    return True


def queries(axes=AXES):
    """(M, N, K, keyword arguments of ops.gemm_kernel_name) in fixture order"""
    for epi, layouts, fp8, ws, batch, c_fp32, K2 in axes["blocks"]:
        for akc, bkc in layouts:
            for M in axes["M"]:
                for N in axes["N"]:
                    for K in axes["K"]:
                        if not accepted(M, N, K, akc, bkc, epi, fp8, batch, c_fp32, K2):
                            continue
                        kw = dict(a_kc=bool(akc), b_kc=bool(bkc), epi=epi, batch=batch, c_fp32=bool(c_fp32),
                                  fp8_mode=fp8, K2=K2)
                        kw["geglu_inter"] = N // 2 if epi == GEGLU else (N if epi == DGEGLU else 0)
                        if not ws:
                            kw["workspace_bytes"] = 0
                        yield M, N, K, kw


def route_names(axes=AXES):
    from pizero_native import ops

    return [ops.gemm_kernel_name(M, N, K, **kw) for M, N, K, kw in queries(axes)]


def decode(fx):
    """the fixture's kernel name per query"""
    out = []
    for ix, n in zip(fx["routes_rle"][0::2], fx["routes_rle"][1::2]):
        out.extend([fx["names"][ix]] * n)
    return out


def knob_runs(default, got, index):
    """the routes that differ from the default table, as runs [first query, name index, repeat, ...]"""
    runs = []
    for i, (d, g) in enumerate(zip(default, got)):
        if g == d:
            continue
        if runs and runs[-3] + runs[-1] == i and runs[-2] == index[g]:
            runs[-1] += 1
        else:
            runs += [i, index[g], 1]
    return runs


def apply_runs(default, names, runs):
    """the routing table of one knob setting: the default one with the setting's runs written over it"""
    out = list(default)
    for i, ix, n in zip(runs[0::3], runs[1::3], runs[2::3]):
        out[i:i + n] = [names[ix]] * n
    return out


def main_knobs():
    """gemm_routes_knobs.json: the same grid under each A/B setting of KNOBS, stored against gemm_routes.json"""
    default = decode(json.load(open(OUT)))
    assert route_names() == default, "the default routes differ from gemm_routes.json"
    tables = []
    for env in KNOBS:
        os.environ.update(env)
        tables.append(route_names())
        for k in env:
            del os.environ[k]
    names = sorted(set(n for t in tables for n in t))
    index = {n: i for i, n in enumerate(names)}
    settings = []
    for env, t in zip(KNOBS, tables):
        runs = knob_runs(default, t, index)
        assert apply_runs(default, names, runs) == t
        settings.append({"env": env, "changed": sum(runs[2::3]), "runs": runs})
        print(f"{env}: {settings[-1]['changed']} of {len(t)} routes differ from the default")
    with open(KNOBS_OUT, "w") as f:
        json.dump({"queries": len(default), "names": names, "settings": settings}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(KNOBS)} settings, {os.path.getsize(KNOBS_OUT)} bytes -> {KNOBS_OUT}")


def main():
    knobs = sorted(k for k in os.environ if k.startswith("PZ_"))
    if knobs:
        sys.exit(f"unset {knobs} first: the fixture holds the default routes")
    sys.path[:0] = [ROOT, os.path.join(ROOT, "open-pi-zero_amd")]
    if "--knobs" in sys.argv:
        return main_knobs()
    got = route_names()
    names = sorted(set(got))
    index = {n: i for i, n in enumerate(names)}
    rle = []
    for n in got:
        if rle and rle[-2] == index[n]:
            rle[-1] += 1
        else:
            rle += [index[n], 1]
    fx = {"axes": AXES, "queries": len(got), "names": names, "routes_rle": rle}
    assert decode(fx) == got
    with open(OUT, "w") as f:
        json.dump(fx, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(got)} queries, {len(names)} kernel names, {os.path.getsize(OUT)} bytes -> {OUT}")


if __name__ == "__main__":
    main()
