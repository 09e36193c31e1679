"""The C-ABI library loads without a GPU and exports every symbol include/pz_abi.h declares."""

import os
import re

from tests.conftest import ROOT


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pz_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert "pz_gemm" in syms and "pz_attn_softmax" in syms and "pz_adamw" in syms
    assert len(syms) >= 30


def test_library_exports_all_declared_symbols():
    import pizero_native
    from pizero_native._lib import SIGNATURES

    L = pizero_native.lib()
    for s in declared_symbols():
        assert hasattr(L, s), s
        assert s in SIGNATURES, f"{s} has no ctypes signature"
    from pizero_native._lib import ABI_VERSION

    hdr = open(os.path.join(ROOT, "include", "pz_abi.h")).read()
    assert f"#define PZ_ABI_VERSION {ABI_VERSION}" in hdr
    assert L.pz_abi_version() == ABI_VERSION


def test_error_path_without_gpu():
    """A host-side argument check fails before any launch and reports a message."""
    import ctypes

    import pizero_native
    from pizero_native._lib import GemmArgs

    a = GemmArgs()
    rc = pizero_native.lib().pz_gemm(ctypes.byref(a), None)
    assert rc == 1
    assert b"bad dims" in pizero_native.lib().pz_last_error()


def test_gemm_planner_routes_without_gpu():
    """pz_gemm_kernel_name is host logic (no device needed): the row-slab kernel takes the measured-faster
    64 < M <= 512 forward shapes (pz_gemm_host.hip plan_rows), the tile kernels keep the rest."""
    from pizero_native import ops

    geglu = ops.PZ_EPI_GEGLU
    assert ops.gemm_kernel_name(256, 3456, 1152).startswith("gemm_rows_kernel<8, 4, 4")  # B=1 SigLIP q|k|v
    assert ops.gemm_kernel_name(320, 8192, 1024, epi=geglu, geglu_inter=4096).startswith("gemm_rows_kernel<4")
    assert not ops.gemm_kernel_name(256, 4304, 1152).startswith("gemm_rows")  # SigLIP fc1
    assert not ops.gemm_kernel_name(256, 1152, 4304).startswith("gemm_rows")  # SigLIP fc2
    assert not ops.gemm_kernel_name(276, 32768, 2048, epi=geglu, geglu_inter=16384).startswith("gemm_rows")
    # tall-tile kernel where it measured faster: B = 1 Gemma down, SigLIP fc2; not the B = 1 gate|up (slower inside
    # the chunk), not the action expert's 320-row down (K = 4096), not C5's 788 rows, not the training rows
    assert ops.gemm_kernel_name(276, 32768, 2048, epi=geglu, geglu_inter=16384).startswith("gemm8p_kernel")
    assert ops.gemm_kernel_name(276, 2048, 16384).startswith("gemm_tall_kernel<5, 2")
    assert ops.gemm_kernel_name(256, 1152, 4304).startswith("gemm_tall_kernel<4, 2")
    assert not ops.gemm_kernel_name(320, 1024, 4096).startswith("gemm_tall")
    assert not ops.gemm_kernel_name(789, 32768, 2048, epi=geglu, geglu_inter=16384).startswith("gemm_tall")
    assert not ops.gemm_kernel_name(35328, 2048, 16384).startswith("gemm_tall")
    assert not ops.gemm_kernel_name(64, 1024, 1024).startswith("gemm_rows")  # few-row paths keep M <= 64
    assert not ops.gemm_kernel_name(17664, 2560, 2048).startswith("gemm_rows")  # training rows: 8-phase
    assert not ops.gemm_kernel_name(320, 1024, 2048, a_kc=False).startswith("gemm_rows")  # k-strided A
    assert ops.gemm_kernel_name(16384, 1152, 1152).startswith("gemm8p_kernel")
    # fewer 256-tiles than CUs at K <= 4096 and >= 1024 rows (the action expert at micro-batch 256): 128-tile kernel
    assert ops.gemm_kernel_name(1280, 2560, 1024).startswith("gemm_kernel<")
    assert ops.gemm_kernel_name(8192, 1024, 1280, a_kc=False, b_kc=False).startswith("gemm_kernel<")
    assert ops.gemm_kernel_name(1280, 1024, 8192, b_kc=False).startswith("gemm8k_kernel")  # K 8192: 256 + tail


def _load_make_gemm_routes():
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_gemm_routes",
                                                  os.path.join(ROOT, "tests", "golden", "make_gemm_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gemm_routes_golden(monkeypatch):
    """The planner's whole routing table (tests/golden/gemm_routes.json, written by make_gemm_routes.py from the
    library as it stood before the concluded A/B knobs were retired) with no PZ_* variable set: every kernel name,
    tile count and split count of ~75,000 argument sets is unchanged.  ops.rows_w8a16_ok, the Python mirror of
    plan_rows that decides whether activations above 64 rows stay bf16, agrees with the planner on every W8A16
    query above 64 rows."""
    import json

    from pizero_native import ops

    for k in [k for k in os.environ if k.startswith("PZ_")]:
        monkeypatch.delenv(k)
    mk = _load_make_gemm_routes()
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")))
    want = mk.decode(fx)
    qs = list(mk.queries(fx["axes"]))
    assert len(qs) == len(want) == fx["queries"]
    bad, mirror = [], []
    for (M, N, K, kw), w in zip(qs, want):
        got = ops.gemm_kernel_name(M, N, K, **kw)
        if got != w:
            bad.append((M, N, K, kw, got, w))
        if kw["fp8_mode"] == 2 and M > 64 and K % 64 == 0:
            ncols = kw["geglu_inter"] if kw["epi"] == ops.PZ_EPI_GEGLU else N
            if ops.rows_w8a16_ok(M, K, ncols) != got.startswith("gemm_rows_kernel"):
                mirror.append((M, N, K, kw, got))
    assert not bad, f"{len(bad)} of {len(qs)} routes changed, first: {bad[:5]}"
    assert not mirror, f"ops.rows_w8a16_ok disagrees with the planner on {len(mirror)} shapes, first: {mirror[:5]}"


def test_gemm_routes_knobs_golden(monkeypatch):
    """The routing table under each of the planner's A/B switches (tests/golden/gemm_routes_knobs.json, written by
    make_gemm_routes.py --knobs from the library as it stood before the planner moved to pz_gemm_host.hip and every
    switch read moved into make_plan): for each setting, every kernel name of the whole grid, stored as the routes
    that differ from the default table."""
    import json

    from pizero_native import ops

    for k in [k for k in os.environ if k.startswith("PZ_")]:
        monkeypatch.delenv(k)
    mk = _load_make_gemm_routes()
    fx0 = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")))
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes_knobs.json")))
    default = mk.decode(fx0)
    qs = list(mk.queries(fx0["axes"]))
    assert len(qs) == len(default) == fx["queries"]
    assert [s["env"] for s in fx["settings"]] == mk.KNOBS
    for s in fx["settings"]:
        want = mk.apply_runs(default, fx["names"], s["runs"])
        assert sum(w != d for w, d in zip(want, default)) == s["changed"] > 0
        for k, v in s["env"].items():
            monkeypatch.setenv(k, v)
        bad = [(M, N, K, kw, got, w) for (M, N, K, kw), w in zip(qs, want)
               if (got := ops.gemm_kernel_name(M, N, K, **kw)) != w]
        for k in s["env"]:
            monkeypatch.delenv(k)
        assert not bad, f"{s['env']}: {len(bad)} of {len(qs)} routes changed, first: {bad[:5]}"


def test_env_knob_census():
    """Every PZ_* environment variable that the library (getenv) or the Python package (os.environ) reads is a row
    of DESIGN.md's "Environment variables" table, and the table lists no variable that nothing reads."""
    read = set()
    pkg = os.path.join(ROOT, "open-pi-zero_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith((".hip", ".h", ".py")):
                continue
            src = open(os.path.join(d, f)).read()
            read |= set(re.findall(r'getenv\(\s*"(PZ_[A-Z0-9_]+)"', src))
            read |= set(re.findall(r'os\.environ(?:\.get\(|\.setdefault\(|\.pop\(|\[)\s*"(PZ_[A-Z0-9_]+)"', src))
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = doc.split("### Environment variables", 1)[1].split("\n## ", 1)[0]
    table = set(re.findall(r"^\| `(PZ_[A-Z0-9_]+)` \|", sec, flags=re.M))
    assert len(read) >= 10, read
    assert read == table, f"read but not in DESIGN.md: {sorted(read - table)}; listed but never read: {sorted(table - read)}"
