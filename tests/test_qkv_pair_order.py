"""CPU: the row order in which the fused qkv kernel streams its weight (lade_qkv_pair_row, csrc/gemm_decl.hpp).  The kernel applies the map where
its weight DMA forms addresses - the stored weight is never permuted, so there is no second layout to invert - and its epilogue relies on three
properties of the map, checked here for every head shape the kernel accepts:
  * it is a permutation of the rows, and the identity on v rows: streaming in tile order reads every weight row exactly once;
  * in a 32-row block of a q or k head, rows r < 16 and r + 16 are a rotation pair (i, i + d/2) - in an MFMA 32 x 32 output tile a lane holds
    rows 8 g4 + 4 hi + e, so accumulators e and e + 8 are that pair;
  * 8 consecutive tile rows are 8 consecutive weight rows: a 1-KiB DMA piece of the K-tile-major weight stays one contiguous KiB."""
import pytest

from lookaheaddecoding_amd import cabi, ops


@pytest.mark.parametrize("H,Hkv,d", [(4, 4, 128), (4, 2, 128), (4, 4, 64), (2, 1, 32), (32, 32, 128), (64, 8, 128), (3, 1, 256), (5, 5, 96)])
def test_pair_order(H, Hkv, d):
    N = (H + 2 * Hkv) * d
    rows = [ops.qkv_pair_row(n, H, Hkv, d) for n in range(N)]
    assert sorted(rows) == list(range(N))
    v0 = (H + Hkv) * d
    assert rows[v0:] == list(range(v0, N))
    for n0 in range(0, v0, 32):
        h, b = n0 // d, (n0 % d) // 32
        for r in range(16):
            assert rows[n0 + r] == h * d + 16 * b + r and rows[n0 + 16 + r] == rows[n0 + r] + d // 2
    for n0 in range(0, N, 8):
        assert rows[n0:n0 + 8] == list(range(rows[n0], rows[n0] + 8))
    # scattering by the inverse restores the order: what tile-order outputs need to land in [q | k | v] order
    inv = [0] * N
    for n, r in enumerate(rows):
        inv[r] = n
    assert [rows[inv[r]] for r in range(N)] == list(range(N))


def test_out_of_range_arguments_are_refused():
    for n, H, Hkv, d in ((0, 4, 4, 48), (-1, 4, 4, 64), (12 * 64, 4, 4, 64), (0, 0, 4, 64)):
        with pytest.raises(cabi.LadeHipError):
            ops.qkv_pair_row(n, H, Hkv, d)


def test_the_flag_is_a_property_of_the_decision_and_travels_in_the_tune_file(tmp_path):
    """GemmCfg.rope_fusable: two splits in a built shape; the row class's flag is a key of its own in the tune file (`wqkv_rope`), written only
    where set, so tables from before the fused launch load and save unchanged"""
    import json
    import torch
    from lookaheaddecoding_amd.engine import StepEngine
    from lookaheaddecoding_amd.tuning import GemmCfg, KernelDecisions
    assert GemmCfg(2, 96, 2, 1, 1).rope_fusable and GemmCfg(4, 96, 2, 2, 1, 3).rope_fusable and GemmCfg(3, 96, 2, 3, 1).rope_fusable
    for c in (GemmCfg(2, 96, 3, 1, 1), GemmCfg(2, 128, 2, 1, 1), GemmCfg(2, 96, 2, 2, 1), GemmCfg(5, 96, 2, 5, 1), GemmCfg(2, 96, 2, 1, 0)):
        assert not c.rope_fusable, c

    class Stub(KernelDecisions):
        custom_gemm, attn_default, dtype, d, has_epilogue, _ntk, skip_attn = True, (0, 128, 0), torch.bfloat16, 128, False, None, False

        def __init__(self, path):
            self.gemm_cfg, self.attn_cfg, self.qkv_rope, self._refined, self.tune_loaded, self.tune_source = {}, {}, {}, set(), [], None
            self.tune_file = path

        def _tune_header(self):
            return {"version": 1}

        def _tune_key(self):
            return "model"

    path = str(tmp_path / "t.json")
    a = Stub(path)
    for m in (32, 64):
        for n in a.LAYER_GEMMS:
            a.gemm_cfg[(n, m)] = GemmCfg(m // 32, 96, 2, 1, 1)
        a._refined.add(m)
    a.qkv_rope[64] = True
    a.save_tune_file()
    rows = json.load(open(path))["models"]["model"]
    assert rows["64"]["wqkv_rope"] == 1 and "wqkv_rope" not in rows["32"]
    b = Stub(path)
    b._load_tune_file(path)
    assert b.qkv_rope == {64: True} and sorted(b.tune_loaded) == [32, 64]
    cfg = b.gemm_cfg[("wqkv", 64)]
    assert b.use_qkv_rope(64, cfg) and not b.use_qkv_rope(32, b.gemm_cfg[("wqkv", 32)]) and not b.use_qkv_rope(None, cfg)
    for attr, val in (("has_epilogue", True), ("_ntk", {}), ("dtype", torch.float32), ("d", 80), ("skip_attn", "all")):
        c = Stub(path)
        c._load_tune_file(path)
        setattr(c, attr, val)
        assert not c.use_qkv_rope(64, cfg), attr
    assert not b.use_qkv_rope(64, cfg._replace(n_split=4))
    assert StepEngine.use_qkv_rope is KernelDecisions.use_qkv_rope
