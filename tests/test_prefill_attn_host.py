"""CPU: which steps go to the one-pass prefill attention kernel (tuning.use_prefill_attn, a pure function of the step), the effect of
LADE_DEBUG=prefill_attn=0, and the flop / byte / split formulas of tools/prefill_attn_bench.py against hand-computed values."""
import importlib.util
import os

import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("prefill_attn_bench", os.path.join(ROOT, "tools", "prefill_attn_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_selection_rule(monkeypatch):
    from lookaheaddecoding_amd.tuning import use_prefill_attn
    monkeypatch.setenv("LADE_DEBUG", "prefill_attn=1")          # the kernel is behind the switch; this is the rule with the switch on
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    # causal chunks above the last GEMM row class, in the 16-bit dtypes: the new kernel
    for T in (257, 440, 512, 952, 2048, 2303):
        assert use_prefill_attn(T, True, bf) and use_prefill_attn(T, True, f16)
    # everything else stays on lade_attn_fwd + lade_attn_combine: chunks of up to 256 rows (one-token steps of plain decoding included) ...
    for T in (1, 60, 64, 240, 256):
        assert not use_prefill_attn(T, True, bf) and not use_prefill_attn(T, True, f16)
    # ... lookahead steps of any width (the reference's default W=60 N=8 G=60 step has 840 rows) ...
    for T in (60, 240, 840):
        assert not use_prefill_attn(T, False, bf)
    # ... fp32, and steps whose cache length lives on the device
    assert not use_prefill_attn(2048, True, f32)
    assert not use_prefill_attn(2048, True, bf, dyn_P=True)
    # the threshold is the engine's last row class, not a constant of its own
    assert use_prefill_attn(200, True, bf, last_row_class=192) and not use_prefill_attn(192, True, bf, last_row_class=192)


def test_selection_rule_needs_a_grid_that_covers_the_chip(monkeypatch):
    """no KV split in the one-pass kernel: a chunk whose 256-row blocks x KV heads do not cover the CUs stays on the split-KV pair, unless the
    pair's own 128-row blocks number at most an eighth of them (models of two or three heads: the parity shapes, a documented loss)"""
    from lookaheaddecoding_amd.tuning import prefill_attn_grid, use_prefill_attn
    monkeypatch.setenv("LADE_DEBUG", "prefill_attn=1")
    bf = torch.bfloat16
    assert prefill_attn_grid(2048, 32, 32) == 256 and prefill_attn_grid(512, 32, 32) == 64 and prefill_attn_grid(2065, 32, 32) == 288
    assert prefill_attn_grid(512, 64, 8) == 128 and prefill_attn_grid(1024, 64, 8) == 256 and prefill_attn_grid(2048, 32, 4) == 256
    assert prefill_attn_grid(2048, 40, 40) == 320 and prefill_attn_grid(257, 2, 1) == 3
    sel = lambda T, H, Hkv: use_prefill_attn(T, True, bf, H=H, Hkv=Hkv, n_cu=256)
    assert sel(2048, 32, 32) and sel(2065, 32, 32) and sel(2303, 32, 32)           # 7B: 2048-row chunks and bench.py's single 2065-row pass
    assert not sel(512, 32, 32) and not sel(1024, 32, 32)                          # 64 / 128 work-groups on 256 CUs
    assert sel(2048, 40, 40) and not sel(1024, 40, 40)                             # 13B
    assert sel(2048, 64, 8) and sel(1024, 64, 8) and not sel(512, 64, 8)           # 70B: 8 heads per KV head stack in the row space
    assert sel(2048, 32, 4) and not sel(1024, 32, 4) and not sel(512, 32, 4)       # TinyLlama
    assert sel(512, 2, 2) and sel(440, 2, 1) and sel(2048, 2, 2) and sel(952, 2, 1)   # the parity shapes: at most 32 blocks of the pair
    assert not sel(2048, 8, 8) and not sel(2048, 4, 4) and not sel(2048, 12, 12) and not sel(2048, 14, 2)   # real small models stay on the pair
    assert not use_prefill_attn(2048, True, bf, switch="0", H=32, Hkv=32)
    assert not use_prefill_attn(256, True, bf, H=2, Hkv=2)


def test_engine_threshold_is_the_last_row_class():
    from lookaheaddecoding_amd.engine import StepEngine
    assert StepEngine.ROW_CLASSES[-1] == 256


def test_the_kernel_is_behind_the_debug_switch(monkeypatch):
    """not the default: without LADE_DEBUG=prefill_attn=1 every step launches the split-KV pair, as before the kernel existed"""
    from lookaheaddecoding_amd.tuning import use_prefill_attn
    monkeypatch.delenv("LADE_DEBUG", raising=False)
    assert not use_prefill_attn(2048, True, torch.bfloat16) and not use_prefill_attn(2048, True, torch.bfloat16, H=32, Hkv=32)
    monkeypatch.setenv("LADE_DEBUG", "prefill_attn=0")
    assert not use_prefill_attn(2048, True, torch.bfloat16)
    monkeypatch.setenv("LADE_DEBUG", "fuse_tail=1,prefill_attn=0")
    assert not use_prefill_attn(512, True, torch.float16)
    monkeypatch.setenv("LADE_DEBUG", "fuse_tail=1")                      # other switches do not turn it on
    assert not use_prefill_attn(2048, True, torch.bfloat16)
    monkeypatch.setenv("LADE_DEBUG", "fuse_tail=1,prefill_attn=1")
    assert use_prefill_attn(2048, True, torch.bfloat16) and not use_prefill_attn(256, True, torch.bfloat16)
    # an explicit switch value wins over the environment (the bench tool's arms)
    assert not use_prefill_attn(2048, True, torch.bfloat16, switch="0") and use_prefill_attn(2048, True, torch.bfloat16, switch="1")


def test_bench_formulas():
    b = _bench()
    # one row, no cache: one key, QK^T 2 d + PV 2 d flops per head
    assert b.causal_flops(1, 0, 1, 128) == 4 * 128
    # T = 3 on P = 2: rows see 3, 4, 5 keys = 12 (row, key) pairs = T P + T (T + 1) / 2 = 6 + 6
    assert b.causal_flops(3, 2, 2, 64) == 4 * 64 * 2 * 12
    # the issue's formula at the review's point: 2065 tokens in one causal pass on the 7B heads
    assert b.causal_flops(2065, 0, 32, 128) == 4 * 128 * 32 * (2065 * 2066 // 2) == 34_949_447_680
    # 86.7 us for those flops is the 0.40 PFLOP/s = 16 % of peak the review quotes
    assert abs(b.causal_flops(2065, 0, 32, 128) / 86.7e-6 / b.PEAK_FLOPS - 0.161) < 0.002
    # T = 2048 at P = 6144 on the 70B heads
    assert b.causal_flops(2048, 6144, 64, 128) == 4 * 128 * 64 * (2048 * 6144 + 2048 * 2049 // 2)
    # bytes: K and V^T of P + T keys once per KV head, q and out once, 2 bytes each
    assert b.io_bytes(2048, 6144, 64, 8, 128) == 2 * (2 * 8 * 8192 * 128 + 2 * 64 * 2048 * 128)
    assert b.io_bytes(1, 0, 1, 1, 64) == 2 * (2 * 64 + 2 * 64)
    assert b.HEAD_SETS == {"7b": (32, 32, 128), "13b": (40, 40, 128), "70b": (64, 8, 128), "tinyllama": (32, 4, 64)}
    assert set(b.POINTS) == {(2048, P) for P in (0, 2048, 6144, 14336, 30720)} | {(T, P) for T in (512, 1024) for P in (0, 6144)}


def test_bench_split_rule_is_the_engines():
    """arm A launches what KernelDecisions.n_splits_for decides for a chunk above the last row class: ops.choose_splits on the 128-row
    work-group, never the single-launch form, a 1024-key floor, at most 32 splits"""
    b = _bench()
    from lookaheaddecoding_amd import ops
    for (H, Hkv, T, S) in ((32, 32, 2048, 8192), (64, 8, 2048, 8192), (32, 4, 512, 512), (40, 40, 1024, 7168)):
        assert b.engine_splits(H, Hkv, T, S) == min(ops.choose_splits(H, H // Hkv, T, max(S, 1024), 256, allow_single=False, block_rows=0, mode=0), 32)
    assert b.engine_splits(32, 4, 300, 300) == b.engine_splits(32, 4, 300, 1024)          # the 1024-key floor
