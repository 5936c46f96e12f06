"""GPU: the qkv GEMM that finishes RoPE + the KV append in its own launch (lade_gemm_qkv_rope) against the two launches it replaces -
lade_gemm_skinny(_kt) with two splits, then lade_rope_kv_append on the partials.  The yardstick is that pair, unchanged code: the rotated q,
the K rows and the V^T columns must be the same BITS, and no cache byte outside rows P .. P+T-1 may change (the caches start from a
sentinel and are compared whole, as 16-bit integers).  Shapes are the smallest at which the kernel can go wrong: hidden 256 (4 K tiles: two
per split), 4 heads of d = 128 (MHA: 16 whole 96-row blocks; GQA with 2 KV heads: a last block that is two thirds empty) and of d = 64, one and
two m-blocks with ragged last blocks (T = 1, 31, 33, 60, 64), the other two built wave grids (T = 92, 128), P = 70 (the V^T segment crosses a
64-key tile), gathered non-monotonic positions.  Then the hand-off itself: the same launch over and over on fresh inputs - the slots and the
ticket counters are reused, so a stale line or a counter left non-zero shows - eagerly and as three replays of one captured graph with P advancing
on the device.  Engine level: token streams and logits with the launch forced on and off; a Qwen-style layer never takes it."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

HIDDEN, S_MAX = 256, 192


def _bits(t):
    return t.contiguous().view(torch.int16)


def _shape(T):
    """(mb, mt) of the fused kernel's wave grid for a T-row step: the row class's two-split wqkv shape at 96-row weight blocks"""
    return (1, 1) if T <= 32 else (2, 1) if T <= 64 else (3, 3) if T <= 96 else (4, 2)


class _Case:
    def __init__(self, H, Hkv, d, dtype, seed, ktile=True):
        from lookaheaddecoding_amd import ops
        from lookaheaddecoding_amd.engine import rope_tables
        self.H, self.Hkv, self.d, self.dtype = H, Hkv, d, dtype
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        self.rnd = random.Random(seed)
        self.N = (H + 2 * Hkv) * d
        w = (torch.randn(self.N, HIDDEN, device="cuda", generator=self.g) * 0.05).to(dtype)
        self.w = ops.to_ktile(w) if ktile else w
        self.cos, self.sin = rope_tables(d, 4096, 10000.0, dtype, "cuda")
        self.part = torch.empty(2 * 128 * (self.N + 96), dtype=torch.float32, device="cuda")
        self.part_ref = torch.empty(2 * 128 * self.N, dtype=torch.float32, device="cuda")
        self.tickets = torch.zeros(64, dtype=torch.int32, device="cuda")

    def caches(self):
        # a sentinel that no rounding produces by accident, the same in both caches of a pair
        kc = torch.full((self.Hkv, S_MAX, self.d), -7.75, dtype=self.dtype, device="cuda")
        vt = torch.full((self.Hkv, self.d, S_MAX), -7.75, dtype=self.dtype, device="cuda")
        return kc, vt

    def inputs(self, T):
        a = torch.randn(T, HIDDEN, device="cuda", generator=self.g).to(self.dtype)
        pos = torch.tensor([self.rnd.randrange(4000) for _ in range(T)], dtype=torch.int32, device="cuda")      # gathered, non-monotonic, repeats
        return a, pos

    def two_launches(self, a, pos, q, kc, vt, P, dyn_P=None, shape=None):
        from lookaheaddecoding_amd import ops
        T = a.shape[0]
        mb, mt = shape or _shape(T)
        ops.gemm_parts(a, self.w, self.part_ref, 2, 96, mb, mt, 1)
        ops.rope_kv_append_parts(self.part_ref, 2, q, pos, self.cos, self.sin, kc, vt, T, P, H=self.H, Hkv=self.Hkv, d=self.d, dyn_P=dyn_P)

    def fused(self, a, pos, q, kc, vt, P, dyn_P=None, shape=None):
        from lookaheaddecoding_amd import ops
        mb, mt = shape or _shape(a.shape[0])
        ops.gemm_qkv_rope(a, self.w, self.part, self.tickets, q, pos, self.cos, self.sin, kc, vt, P, H=self.H, Hkv=self.Hkv, d=self.d, bn=96, mb=mb,
                          mt=mt, nt=1, dyn_P=dyn_P)

    def check(self, T, P, q_new, q_old, kc_new, kc_old, vt_new, vt_old, what):
        torch.cuda.synchronize()
        assert torch.equal(_bits(q_new[:T]), _bits(q_old[:T])), (what, "q")
        assert torch.equal(_bits(kc_new), _bits(kc_old)), (what, "K cache")
        assert torch.equal(_bits(vt_new), _bits(vt_old)), (what, "V^T cache")
        assert not bool(torch.any(self.tickets)), (what, "a ticket counter was left non-zero")


_CASES = {}


def _case(H, Hkv, d, dtype, ktile=True):
    key = (H, Hkv, d, dtype, ktile)
    if key not in _CASES:
        _CASES[key] = _Case(H, Hkv, d, dtype, seed=H * 1000 + Hkv * 100 + d + (dtype == torch.float16), ktile=ktile)
    return _CASES[key]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H,Hkv,d", [(4, 4, 128), (4, 2, 128), (4, 4, 64)])
@pytest.mark.parametrize("P", [0, 5, 70])
@pytest.mark.parametrize("T", [1, 31, 33, 60, 64])
def test_same_bits_as_the_two_launches(T, P, H, Hkv, d, dtype):
    c = _case(H, Hkv, d, dtype)
    a, pos = c.inputs(T)
    kc_old, vt_old = c.caches()
    kc_new, vt_new = c.caches()
    q_old = torch.zeros(T, H * d, dtype=dtype, device="cuda")
    q_new = torch.full_like(q_old, 3.0)
    c.two_launches(a, pos, q_old, kc_old, vt_old, P)
    c.fused(a, pos, q_new, kc_new, vt_new, P)
    c.check(T, P, q_new, q_old, kc_new, kc_old, vt_new, vt_old, (T, P, H, Hkv, d, dtype))
    # nothing outside rows P .. P+T-1 (stated on its own: the comparison above would not see a byte both paths wrote)
    sent = _bits(torch.full((1,), -7.75, dtype=dtype, device="cuda"))[0]
    kb, vb = _bits(kc_new), _bits(vt_new)
    assert bool((kb[:, :P] == sent).all()) and bool((kb[:, P + T:] == sent).all())
    assert bool((vb[:, :, :P] == sent).all()) and bool((vb[:, :, P + T:] == sent).all())
    assert not bool((kb[:, P:P + T] == sent).all())          # ... and the rows themselves were written


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("T,ktile,shape", [(92, True, None), (128, True, None), (60, False, None), (60, True, (1, 1)), (128, True, (2, 1))])
def test_the_other_wave_grids_and_a_row_major_weight(T, ktile, shape, dtype):
    """(+ 60 / 128 rows on 32 / 64-row work-groups: two m-blocks of work-groups per n-block, each pair with a ticket of its own)"""
    H, Hkv, d, P = 4, 2, 128, 5
    c = _case(H, Hkv, d, dtype, ktile)
    a, pos = c.inputs(T)
    kc_old, vt_old = c.caches()
    kc_new, vt_new = c.caches()
    q_old, q_new = torch.zeros(T, H * d, dtype=dtype, device="cuda"), torch.ones(T, H * d, dtype=dtype, device="cuda")
    c.two_launches(a, pos, q_old, kc_old, vt_old, P, shape=shape)
    c.fused(a, pos, q_new, kc_new, vt_new, P, shape=shape)
    c.check(T, P, q_new, q_old, kc_new, kc_old, vt_new, vt_old, (T, ktile, shape, dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_back_to_back_launches_reuse_slots_and_tickets(dtype):
    """the hand-off space and the counters of launch i are those of launch i + 1: fresh inputs every time, no synchronisation in between"""
    H, Hkv, d, T = 4, 4, 128, 60
    c = _case(H, Hkv, d, dtype)
    outs = []
    for i in range(8):
        a, pos = c.inputs(T)
        P = 7 * i
        kc_old, vt_old = c.caches()
        kc_new, vt_new = c.caches()
        q_old, q_new = torch.zeros(T, H * d, dtype=dtype, device="cuda"), torch.ones(T, H * d, dtype=dtype, device="cuda")
        c.fused(a, pos, q_new, kc_new, vt_new, P)
        c.two_launches(a, pos, q_old, kc_old, vt_old, P)
        outs.append((P, q_new, q_old, kc_new, kc_old, vt_new, vt_old))
    for i, (P, *t) in enumerate(outs):
        c.check(T, P, *t, ("launch", i, dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_three_replays_of_one_graph_with_P_advancing_on_the_device(dtype):
    H, Hkv, d, T = 4, 2, 128, 60
    c = _case(H, Hkv, d, dtype)
    a, pos = c.inputs(T)
    dyn_P = torch.zeros(1, dtype=torch.int32, device="cuda")
    kc_old, vt_old = c.caches()
    kc_new, vt_new = c.caches()
    q_old, q_new = torch.zeros(T, H * d, dtype=dtype, device="cuda"), torch.ones(T, H * d, dtype=dtype, device="cuda")
    warm_k, warm_v = c.caches()
    c.fused(a, pos, q_new, warm_k, warm_v, 0, dyn_P)          # eager once: first-launch attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.fused(a, pos, q_new, kc_new, vt_new, 0, dyn_P)
    kc_new.fill_(-7.75)
    vt_new.fill_(-7.75)
    for i in range(3):
        a2, pos2 = c.inputs(T)
        a.copy_(a2)
        pos.copy_(pos2)
        dyn_P.fill_(60 * i)
        g.replay()
        c.two_launches(a, pos, q_old, kc_old, vt_old, 0, dyn_P)
        c.check(T, 60 * i, q_new, q_old, kc_new, kc_old, vt_new, vt_old, ("replay", i, dtype))
    # a step that would pass the end of the cache writes nothing (and still leaves its counters at zero)
    dyn_P.fill_(S_MAX - T + 1)
    before_k, before_v = kc_new.clone(), vt_new.clone()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(kc_new), _bits(before_k)) and torch.equal(_bits(vt_new), _bits(before_v)) and not bool(torch.any(c.tickets))


def test_arguments_the_fused_kernel_cannot_serve_are_refused():
    from lookaheaddecoding_amd import cabi, ops
    c = _case(4, 4, 128, torch.bfloat16)
    a, pos = c.inputs(60)
    kc, vt = c.caches()
    q = torch.zeros(60, 4 * 128, dtype=torch.bfloat16, device="cuda")
    kw = dict(H=4, Hkv=4, d=128)
    with pytest.raises(cabi.LadeHipError, match="no fused kernel"):
        ops.gemm_qkv_rope(a, c.w, c.part, c.tickets, q, pos, c.cos, c.sin, kc, vt, 0, bn=128, mb=2, mt=1, nt=1, **kw)
    with pytest.raises(cabi.LadeHipError, match="hand-off space"):
        ops.gemm_qkv_rope(a, c.w, c.part[:1024], c.tickets, q, pos, c.cos, c.sin, kc, vt, 0, bn=96, mb=2, mt=1, nt=1, **kw)
    with pytest.raises(cabi.LadeHipError, match="hand-off space"):
        ops.gemm_qkv_rope(a, c.w, c.part, c.tickets[:4], q, pos, c.cos, c.sin, kc, vt, 0, bn=96, mb=2, mt=1, nt=1, **kw)
    with pytest.raises(cabi.LadeHipError, match="S_max"):
        ops.gemm_qkv_rope(a, c.w, c.part, c.tickets, q, pos, c.cos, c.sin, kc, vt, S_MAX - 59, bn=96, mb=2, mt=1, nt=1, **kw)
    with pytest.raises(cabi.LadeHipError, match="whole 32-row blocks"):
        ops.gemm_qkv_rope(a, c.w, c.part, c.tickets, q, pos, c.cos, c.sin, kc, vt, 0, bn=96, mb=2, mt=1, nt=1, H=3, Hkv=4, d=128)


# ---- engine level ------------------------------------------------------------------------------------------------------------------------

def _engine(name, dtype, monkeypatch, layers=4):
    """a small engine whose kernel decisions are pinned: wqkv on the two-split 96-row shape of each row class the fused kernel is built for, the
    library everywhere else - so that the only thing the LADE_DEBUG switch changes is the launch under test"""
    from lookaheaddecoding_amd.engine import StepEngine
    from lookaheaddecoding_amd.tuning import GemmCfg
    from lookaheaddecoding_amd.weights import make_config, random_weights_numpy
    monkeypatch.setenv("LADE_TUNE_FILE", "off")
    cfg = make_config(name, layers=layers, max_pos=512)
    w = {k: torch.as_tensor(v) for k, v in random_weights_numpy(cfg, seed=3, std=0.05).items()}
    eng = StepEngine(cfg, w, dtype=dtype, device="cuda:0", max_seq=256, max_T=128)
    assert eng.custom_gemm
    for m in eng.ROW_CLASSES:
        for n in eng.GEMM_NAMES:
            eng.gemm_cfg[(n, m)] = None
        if m <= 128:
            mb, mt = _shape(m)
            eng.gemm_cfg[("wqkv", m)] = GemmCfg(mb, 96, 2, mt, 1)
        eng._refined.add(m)
    return eng


def _count_launches(monkeypatch):
    from lookaheaddecoding_amd import ops
    n = {"fused": 0, "rope_parts": 0, "epi": 0}
    f0, r0 = ops.gemm_qkv_rope, ops.rope_kv_append_parts

    def fused(*a, **k):
        n["fused"] += 1
        return f0(*a, **k)

    def rope_parts(*a, **k):
        n["rope_parts"] += 1
        n["epi"] += k.get("epi") is not None
        return r0(*a, **k)
    monkeypatch.setattr(ops, "gemm_qkv_rope", fused)
    monkeypatch.setattr(ops, "rope_kv_append_parts", rope_parts)
    return n


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_engine_streams_and_logits_do_not_depend_on_the_launch(dtype, monkeypatch):
    """tiny-d128 with 4 layers: 24 lookahead steps (eager, then as hipGraph steps) and one 60-row step with gathered positions, once with the
    old pair forced and once with the fused launch forced - same tokens, same step counts, same logits bits"""
    from lookaheaddecoding_amd.decoding import LookaheadDecoder
    from lookaheaddecoding_amd.ops import StepMask
    prompt = [1, 5, 9, 17, 33, 5, 9, 17, 44, 5, 9]
    n = _count_launches(monkeypatch)
    res = {}
    for arm in ("0", "1"):
        monkeypatch.setenv("LADE_DEBUG", f"qkv_rope={arm}")
        eng = _engine("tiny-d128", dtype, monkeypatch)
        before = dict(n)
        out = LookaheadDecoder(eng, 7, 4, 7).greedy(prompt, len(prompt) + 40, rng=random.Random(1))
        assert out.steps >= 24 or out.generated == 40
        gr = LookaheadDecoder(eng, 7, 4, 7, use_graph=True).greedy(prompt, len(prompt) + 40, rng=random.Random(1))
        T, P = 60, 50
        rnd = random.Random(5)
        ids = torch.tensor([rnd.randrange(300) for _ in range(T)], dtype=torch.int32, device="cuda")
        pos = torch.tensor([P + rnd.randrange(40) for _ in range(T)], dtype=torch.int32, device="cuda")
        sel = torch.arange(T, dtype=torch.int32, device="cuda")
        logits = eng.forward(ids, pos, StepMask(T=T, P=P, is_prefill=True), sel, T)
        torch.cuda.synchronize()
        res[arm] = (out.tokens, out.steps, gr.tokens, gr.steps, _bits(logits).clone(), _bits(eng.kv).clone())
        took = {k: n[k] - before[k] for k in n}
        if arm == "0":
            assert took["fused"] == 0 and took["rope_parts"] > 0, took
        else:
            assert took["fused"] > 0 and took["rope_parts"] == 0, took
    assert res["0"][:4] == res["1"][:4]
    assert torch.equal(res["0"][4], res["1"][4]), "logits differ between the two launch forms"
    assert torch.equal(res["0"][5], res["1"][5]), "KV cache differs between the two launch forms"


@pytest.mark.parametrize("name", ["tiny-qwen2", "tiny-qwen3"])
def test_a_layer_with_a_qkv_epilogue_keeps_the_two_launches(name, monkeypatch):
    """Qwen bias / head norm run in lade_rope_kv_append's epilogue: even with the fused launch forced on, the engine must not take it"""
    from lookaheaddecoding_amd.ops import StepMask
    n = _count_launches(monkeypatch)
    monkeypatch.setenv("LADE_DEBUG", "qkv_rope=1")
    eng = _engine(name, torch.bfloat16, monkeypatch, layers=2)
    assert eng.has_epilogue and all(lw["epi_parts"] is not None for lw in eng.layers)
    T = 20
    ids = torch.arange(T, dtype=torch.int32, device="cuda")
    eng.forward(ids, ids, StepMask(T=T, P=0, is_prefill=True), torch.zeros(1, dtype=torch.int32, device="cuda"), 1)
    torch.cuda.synchronize()
    assert n["fused"] == 0 and n["rope_parts"] == len(eng.layers) and n["epi"] == len(eng.layers), n
    assert not eng.use_qkv_rope(32, eng.gemm_cfg[("wqkv", 32)])
