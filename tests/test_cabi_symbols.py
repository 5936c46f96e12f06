"""CPU: the C-ABI library builds, loads and exports every symbol include/lade_hip.h declares;
argument validation works without a GPU (no compute calls)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "lade_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lade_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from lookaheaddecoding_amd import cabi
    if not os.path.exists(cabi.LIB_PATH):
        g.build()
    return cabi.load_library()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from lookaheaddecoding_amd import cabi
    syms = declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in lade_hip.h but not exported"
        assert s in cabi.SIGNATURES, f"{s} has no ctypes signature"
    assert sorted(cabi.SIGNATURES) == syms
    assert lib.lade_version() == cabi.ABI_VERSION == 5


def test_attn_args_has_the_size_the_library_was_compiled_with():
    """csrc/attn.hip pins sizeof(lade_attn_args) with a static_assert on the same number: 7 pointers, 2 x int64, 6 x int32, float, the 9 x int32 mask
    and wg_rows, padded to 8 bytes.  A field added or dropped on one side only fails here or at compile time."""
    from lookaheaddecoding_amd import cabi
    src = open(os.path.join(ROOT, "lookaheaddecoding_amd", "csrc", "attn.hip")).read()
    pinned = re.findall(r"static_assert\(sizeof\(lade_attn_args\) == (\d+),", src)
    assert pinned == ["144"]
    assert C.sizeof(cabi.AttnArgs) == 144
    assert cabi.AttnArgs._fields_[-1][0] == "wg_rows"


def test_argument_validation_returns_error_codes_not_crashes(lib):
    from lookaheaddecoding_amd import cabi
    a = cabi.AttnArgs()
    rc = lib.lade_attn_fwd(C.byref(a), None)
    assert rc == -1 and b"null" in lib.lade_last_error_string()
    rc = lib.lade_argmax_rows(None, 10, 1, 10, 0, None, None)
    assert rc == -1
    rc = lib.lade_pool_lookup(None, None, 10, 0, 3, None, None, None, None)
    assert rc == -1 and b"lade_pool_lookup" in lib.lade_last_error_string()


def test_merged_entry_points_take_exactly_one_source(lib):
    """lade_rope_kv_append (qkv | parts), lade_add_rmsnorm (r | parts) and lade_silu_mul (gu | parts): both sources or neither is LADE_E_ARG
    with the function's name, before any launch (dummy non-null pointers, no GPU)"""
    from lookaheaddecoding_amd import cabi
    p = 1 << 20
    for qkv, parts in ((p, p), (None, None)):
        rc = lib.lade_rope_kv_append(qkv, parts, 2, 4096, p, p, p, p, p, p, 4, 0, None, 2, 1, 64, 64, 64, cabi.LADE_BF16, None, None)
        assert rc == -1 and b"lade_rope_kv_append: exactly one" in lib.lade_last_error_string()
    for r, parts in ((p, p), (None, None)):
        for sel, src_rows in ((None, 0), (p, 4)):
            rc = lib.lade_add_rmsnorm(p, r, parts, 2, 4096, sel, src_rows, p, p, 4, 1024, 1e-5, cabi.LADE_BF16, None)
            assert rc == -1 and b"lade_add_rmsnorm: exactly one" in lib.lade_last_error_string()
    for gu, parts in ((p, p), (None, None)):
        rc = lib.lade_silu_mul(gu, parts, 2, 4096, p, 4, 512, 0, cabi.LADE_BF16, None)
        assert rc == -1 and b"lade_silu_mul: exactly one" in lib.lade_last_error_string()
    # the partials of the two glue calls are 16-bit only (LADE_E_DTYPE, after the argument checks), need n_parts >= 1, and a row selection
    # needs the number of source rows
    assert lib.lade_add_rmsnorm(p, None, p, 2, 4096, None, 0, p, p, 4, 1024, 1e-5, cabi.LADE_F32, None) == -2
    assert lib.lade_silu_mul(None, p, 2, 4096, p, 4, 512, 0, cabi.LADE_F32, None) == -2
    assert lib.lade_add_rmsnorm(p, None, p, 0, 4096, None, 0, p, p, 4, 1024, 1e-5, cabi.LADE_BF16, None) == -1
    assert lib.lade_silu_mul(None, p, 0, 4096, p, 4, 512, 0, cabi.LADE_BF16, None) == -1
    assert lib.lade_add_rmsnorm(p, p, None, 0, 0, p, 0, p, p, 4, 1024, 1e-5, cabi.LADE_BF16, None) == -1
    assert b"src_rows" in lib.lade_last_error_string()
    assert lib.lade_add_rmsnorm(p, p, None, 0, 0, None, 0, p, p, 0, 1024, 1e-5, cabi.LADE_BF16, None) == 0      # no rows: nothing to launch


def test_a_failure_inside_a_gemm_launch_keeps_its_own_code_and_message(lib):
    """the shape (160 rows x 256 weight rows, one wave holding five m-blocks) IS in the table, but 8 stages x 52 KB exceed the LDS: launch_gemm's
    own message must reach the caller instead of being retried in the other groups of the table and overwritten by "no kernel for ..."
    (the check runs before any launch: dummy non-null pointers, no GPU)"""
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    M, N, K = 160, 256, 64
    rc = lib.lade_gemm_skinny(p, K, p, K, p, N, None, M, N, K, 1, 256, 5, 5, 1, 8, 0, 0, None)
    msg = lib.lade_last_error_string()
    assert rc == -1, (rc, msg)                     # LADE_E_ARG
    assert b"does not fit" in msg and b"no kernel for" not in msg, msg
    # ... and a wave grid that no group of the table holds still says so
    rc = lib.lade_gemm_skinny(p, K, p, K, p, N, None, M, N, K, 1, 256, 5, 5, 4, 0, 0, 0, None)
    assert rc == -1 and b"no kernel for" in lib.lade_last_error_string()


def test_missing_library_fails_loudly(tmp_path):
    from lookaheaddecoding_amd import cabi
    old = cabi._lib
    cabi._lib = None
    try:
        with pytest.raises(cabi.LadeHipError):
            cabi.load_library(str(tmp_path / "nope.so"))
    finally:
        cabi._lib = old


def test_engine_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from lookaheaddecoding_amd import cabi
    from lookaheaddecoding_amd.engine import StepEngine
    from lookaheaddecoding_amd.weights import make_config, random_weights_numpy
    cfg = make_config("tiny-d64")
    w = {k: torch.as_tensor(v) for k, v in random_weights_numpy(cfg).items()}
    with pytest.raises(cabi.LadeHipError):
        StepEngine(cfg, w, dtype=torch.float32)
