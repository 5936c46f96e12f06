"""The kernel-decision table shipped with the package (lookaheaddecoding_amd/tuned/gfx950_256cu.json, tools/make_tune_table.py): well formed, written
for this library generation, complete for the BASELINE shapes - and every decision names a kernel the shape table builds."""
import json
import os
import re

from lookaheaddecoding_amd import cabi
from lookaheaddecoding_amd.engine import StepEngine

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "..", "lookaheaddecoding_amd", "tuned", "gfx950_256cu.json")


def _built_shapes():
    src = open(os.path.join(HERE, "..", "lookaheaddecoding_amd", "csrc", "gemm_kernel.hpp")).read()
    return {tuple(int(x) for x in m) for m in re.findall(r"SHAPE\(TT,(\d),(\d),(\d),(\d)\)", src)}


def test_shipped_table_is_for_this_library_and_names_built_kernels():
    doc = json.load(open(TABLE))
    assert doc["header"] == {"version": StepEngine.TUNE_FILE_VERSION, "abi": cabi.ABI_VERSION, "device": "gfx950", "n_cu": 256,
                             "row_classes": list(StepEngine.ROW_CLASSES)}
    shapes = _built_shapes()
    keys = [json.loads(k) for k in doc["models"]]
    assert [4096, 11008, 32, 32, 128, 32, 32000, "torch.bfloat16"] in [k[:8] for k in keys]          # BASELINE configs 2 / 3
    assert [5120, 13824, 40, 40, 128, 40, 32016, "torch.bfloat16"] in [k[:8] for k in keys]          # config 4
    n = 0
    assert [8192, 28672, 64, 8, 128, 80, 32000, "torch.bfloat16"] in [k[:8] for k in keys]           # config 5
    for key, ent in doc["models"].items():
        H, Hkv = json.loads(key)[2:4]
        assert sorted(int(m) for m in ent) == sorted(StepEngine.ROW_CLASSES)
        for m, row in ent.items():
            assert set(row) >= set(StepEngine.LAYER_GEMMS) | {"attn"}
            # the attention launch is frozen: 128-row work-groups, sqrt split rule - 64-row ones where >= 8 heads stack > 128 rows on a KV head
            assert row["attn"][:3] == [0, 64 if (H // Hkv >= 8 and (H // Hkv) * (int(m) - 31) > 128) else 128, 0], (key, m, row["attn"])
            for name in StepEngine.GEMM_NAMES:
                c = row.get(name)
                if c is None:
                    continue                                        # the library GEMM
                mb, bn, S, mt, nt, ring = c
                assert mb * 32 == int(m) and S >= 1 and ring in (0, 2, 3, 4, 5, 6, 8)
                if nt:
                    assert (mb // mt, mt, bn // 32 // nt, nt) in shapes, (name, m, c)
                n += 1
    assert n >= 60


def test_a_row_that_selects_a_fused_rope_attention_form_is_refused(tmp_path):
    """the attention triple keeps its leading slot (0 in every table written since round 6) so that old and new tables read alike; a row that
    asks for one of the removed fused RoPE + KV append forms there is an error, not a silently different launch"""
    import pytest
    from lookaheaddecoding_amd.tuning import KernelDecisions

    class Stub(KernelDecisions):
        ROW_CLASSES, GEMM_NAMES, LAYER_GEMMS = StepEngine.ROW_CLASSES, StepEngine.GEMM_NAMES, StepEngine.LAYER_GEMMS

        def __init__(self):
            self.gemm_cfg, self.attn_cfg, self._refined, self.tune_loaded, self.tune_source = {}, {}, set(), [], None

        def _tune_header(self):
            return {"version": 1}

        def _tune_key(self):
            return "model"

    m = str(StepEngine.ROW_CLASSES[0])
    for first, ok in ((0, True), (1, False), (2, False)):
        path = tmp_path / f"t{first}.json"
        path.write_text(json.dumps({"header": {"version": 1}, "models": {"model": {m: {"attn": [first, 128, 0]}}}}))
        eng = Stub()
        if ok:
            eng._load_tune_file(str(path))
            assert eng.attn_cfg == {int(m): (0, 128, 0)}
        else:
            with pytest.raises(cabi.LadeHipError, match="fused-RoPE"):
                eng._load_tune_file(str(path))
            assert eng.attn_cfg == {}


# ---- the host side of the kernel decisions: candidate sets, the tune file, the gate, the row-class lookup (no GPU) ----------------------

def _stub(header=None, key="model"):
    """a KernelDecisions with the handful of attributes the mixin reads, whose two tuning passes only record that they were called"""
    import torch
    from lookaheaddecoding_amd.tuning import KernelDecisions

    class Stub(KernelDecisions):
        custom_gemm, attn_default, tune_file, dtype, device = True, (0, 128, 0), None, torch.bfloat16, -1     # (device -1: a no-op device context)

        def __init__(self):
            self.gemm_cfg, self.attn_cfg, self._refined, self.tune_loaded, self.tune_source = {}, {}, set(), [], None
            self._ranked, self._refining, self.calls = {}, False, []

        def _tune_header(self):
            return header

        def _tune_key(self):
            return key

        def _tune(self, name, M):
            self.calls.append(("tune", name, M))
            return self.gemm_cfg.setdefault((name, self.row_class(M)), None)

        def _refine_in_step(self, mclass, allow_grow=False):
            self.calls.append(("refine", mclass, allow_grow))
    return Stub()


def _projection_shapes(model_key):
    hidden, inter, H, Hkv, d, _L, V = json.loads(model_key)[:7]
    return {"wqkv": ((H + 2 * Hkv) * d, hidden), "wo": (hidden, H * d), "wgu": (2 * inter, hidden), "wd": (hidden, inter), "lm_head": (V, hidden)}


def test_every_shipped_decision_is_among_the_candidates_the_tuners_enumerate():
    """the table was measured on an MI355X by the tuners before their candidate loops became functions: an independent witness of what they yield"""
    from lookaheaddecoding_amd.tuning import lm_head_candidates, ring_variants, splitk_candidates, swiglu_candidates
    n = 0
    for key, ent in json.load(open(TABLE))["models"].items():
        gu_layout = json.loads(key)[9]
        for m, row in ent.items():
            for name, (N, K) in _projection_shapes(key).items():
                if row.get(name) is None:
                    continue
                if name == "lm_head":
                    cands = lm_head_candidates(int(m))
                else:
                    shapes = splitk_candidates(int(m), N, K, 256) + (swiglu_candidates(int(m), N) if name == "wgu" and gu_layout == 1 else [])
                    cands = [c for s in shapes for c in ring_variants(s, in_step=True)]
                assert tuple(row[name]) in cands, (key, m, name, row[name])
                n += 1
    assert n == 119


def test_candidate_order_is_pinned():
    """min() over (ms, cfg) breaks ties by the tuple, the in-step list is cut at 18 and the ring pass takes the first three: order is behaviour"""
    from lookaheaddecoding_amd.tuning import GemmCfg, splitk_candidates
    # Llama-2-7B gate/up at the 64-row class: N = 2 x 11008 = 22016, K = 4096, 256 CUs.  The class's shapes are (mb, mt, nt, bns) =
    # (2,1,0,(128,256)) (2,2,0,(128,192,256)) (2,2,2,(192,256)) (2,1,1,(64,96)) (2,2,1,(96,)); S = round(256 k / ceil(N / bn)), k = 1, 2, 3, kept
    # when 2 <= S <= 16 (K / 64 = 64 >= 2 S and 64 S <= 2048 hold for all of those):
    #   bn 128: 172 blocks -> 1.49, 2.98, 4.47 -> {1, 3, 4} -> S = 3, 4            bn 256:  86 blocks -> 2.98, 5.95, 8.93 -> S = 3, 6, 9
    #   bn 192: 115 blocks -> 2.23, 4.45, 6.68 -> S = 2, 4, 7                      bn  64: 344 blocks -> 0.74, 1.49, 2.23 -> {1, 2} -> S = 2
    #   bn  96: 230 blocks -> 1.11, 2.23, 3.34 -> {1, 2, 3} -> S = 2, 3
    # per shape: (2 + 3) + (2 + 3 + 3) + (3 + 3) + (1 + 2) + 2 = 24; the first is shape 1 at bn 128, S 3, the last shape 5 at bn 96, S 3
    cands = splitk_candidates(64, 22016, 4096, 256)
    assert len(cands) == 24 and cands[0] == (2, 128, 3, 1, 0, 0) and cands[-1] == (2, 96, 3, 2, 1, 0)
    assert cands[:5] == [(2, 128, 3, 1, 0, 0), (2, 128, 4, 1, 0, 0), (2, 256, 3, 1, 0, 0), (2, 256, 6, 1, 0, 0), (2, 256, 9, 1, 0, 0)]
    assert all(isinstance(c, GemmCfg) for c in cands)

    # the in-step list: the incumbent (here the library), the ranking's first three that are kernels (A, B, D), then its best of the two smallest
    # split counts (2 -> C, 3 -> A again: adds nothing), each at ring 0, 3, 5, 6, 8 (+ 2 for stages >= 32 KB) where ring x stage <= 160 KB and
    # ring != the default min(4, 160 KB // stage).  Stages are (bn + 32 mb) x 128 B:
    #   A (2,64,3,1,1):  16 KB, default 4: 0 3 5 6 8      B (2,128,4,2,0): 24 KB, default 4: 0 3 5 6 (8 x 24 = 192 KB)
    #   D (2,192,7,2,0): 32 KB, default 4: 0 3 5 (5 x 32 = 160 KB fits) then 2      C (2,96,2,2,1): 20 KB, default 4: 0 3 5 6 8 (8 x 20 = 160 KB)
    # 1 + 5 + 4 + 4 + 5 = 19, cut at 18: C at 8 stages falls off
    A, B, D, C = GemmCfg(2, 64, 3, 1, 1), GemmCfg(2, 128, 4, 2, 0), GemmCfg(2, 192, 7, 2, 0), GemmCfg(2, 96, 2, 2, 1)
    eng = _stub()
    eng._ranked[("wgu", 64)] = [(0.10, A), (0.11, B), (0.12, D), (0.13, None), (0.14, C)]
    eng.gemm_cfg[("wgu", 64)] = None
    out = eng._step_candidates("wgu", 64)
    assert len(out) == 18 and out[0] is None and out[1] == A and out[-1] == (2, 96, 2, 2, 1, 6)
    assert out[10:14] == [(2, 192, 7, 2, 0, 0), (2, 192, 7, 2, 0, 3), (2, 192, 7, 2, 0, 5), (2, 192, 7, 2, 0, 2)]
    eng.gemm_cfg[("wgu", 64)] = B._replace(ring=6)            # an incumbent from the list comes first and is not repeated
    out = eng._step_candidates("wgu", 64)
    assert out[0] == (2, 128, 4, 2, 0, 6) and out.count(out[0]) == 1 and len(out) == 18 and out[-1] == (2, 96, 2, 2, 1, 8)


def test_the_shipped_table_round_trips_through_load_and_save_byte_for_byte(tmp_path):
    from lookaheaddecoding_amd.tuning import GemmCfg
    doc = json.load(open(TABLE))
    path = tmp_path / "again.json"
    for key in doc["models"]:
        eng = _stub(doc["header"], key)
        eng._load_tune_file(TABLE)
        assert sorted(eng.tune_loaded) == sorted(StepEngine.ROW_CLASSES) and eng.gemm_cfg
        assert all(c is None or type(c) is GemmCfg for c in eng.gemm_cfg.values())
        assert eng.save_tune_file(str(path)) == str(path)
    assert path.read_bytes() == open(TABLE, "rb").read()


def test_one_gate_takes_the_isolated_decisions_and_then_the_in_step_pass(monkeypatch):
    import torch
    capturing = [False]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
    four = [("tune", n, 64) for n in StepEngine.LAYER_GEMMS]
    eng = _stub()
    eng._decide(64)                                        # what forward() calls before it touches a workspace
    assert eng.calls == four + [("refine", 64, False)]
    for closed in ("refined", "refining", "no custom gemm"):
        eng = _stub()
        if closed == "refined":
            eng._refined.add(64)
        eng._refining, eng.custom_gemm = closed == "refining", closed != "no custom gemm"
        eng._decide(64)
        eng._decide(64, allow_grow=True)
        assert eng.attn_choice(60) == (0, 128, 0)
        eng.prepare([60])
        assert eng.calls == [], closed
    eng = _stub()
    assert eng.attn_choice(60) == (0, 128, 0) and eng.calls == four + [("refine", 64, False)]
    eng = _stub()
    eng.prepare([60, 64, 300])                             # (both of one class; 300 rows: above the last class)
    assert eng.calls == 2 * (four + [("refine", 64, True)])          # (the stub never closes a class)
    eng = _stub()
    table = eng.tune_all()
    assert eng.calls == [c for m in eng.ROW_CLASSES for c in [("tune", n, m) for n in eng.LAYER_GEMMS] + [("refine", m, True), ("tune", "lm_head", m)]]
    assert set(table) == {f"{n}:{m}" for n in eng.TUNE_NAMES for m in eng.ROW_CLASSES}
    # during a stream capture: a caller that only asks is answered from what is decided, a step goes on to _refine_in_step (which raises there)
    capturing[0] = True
    eng = _stub()
    assert eng.attn_choice(60) == (0, 128, 0) and eng.calls == []
    eng._decide(64)
    assert eng.calls == four + [("refine", 64, False)]


def test_row_class_lookup():
    eng = _stub()
    assert [eng.row_class(T) for T in (1, 32, 33, 128, 129, 160, 161, 256, 257)] == [32, 32, 64, 128, 160, 160, 192, 256, None]
