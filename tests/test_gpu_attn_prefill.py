"""lade_attn_prefill, the one-pass causal attention of prefill chunks (csrc/attn_prefill.hip), on the GPU:

* kernel level against the CPU oracle's dense attention under the causal mask (lade/models/modeling_llama.py:124-130, :520-541) on the same
  rounded inputs, at the tolerances of the other attention tests (bf16 2e-2 / 2e-2, f16 4e-3 / 1e-2);
* stale cache rows (NaN beyond P + T) never reach the output; argument validation answers LADE_E_ARG with a message;
* engine level: chunked prefill of a 3000-token prompt through the new kernel (LADE_DEBUG=prefill_attn=1) and through the split-KV
  pair (the default) - both within the reference's own 16-bit envelope (the rule of test_gpu_parity_shapes.py), layer-0 K / V rows bit-identical,
  and the call counter of the ops wrapper shows which kernel ran."""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lade_oracle as O
from lookaheaddecoding_amd.weights import make_config, random_weights_numpy

TOL = {torch.bfloat16: dict(atol=2e-2, rtol=2e-2), torch.float16: dict(atol=4e-3, rtol=1e-2)}
T_SET = (257, 512, 1000, 2048, 2303)
P_SET = (0, 100, 2049, 6144)
HEADS = ((4, 4, 128), (8, 2, 128), (8, 1, 64), (4, 2, 64))
DTYPES = (torch.bfloat16, torch.float16)


def _cases():
    """every (T, P) pair once; the head set and the dtype rotate so that each head set runs in both dtypes, at short and long chunks, at P = 0
    (the diagonal alone), at P not a multiple of 64 (100, 2049: the masked band starts inside a tile) and at a long cache.  What has a code
    path of its own: d = 64 / 128 (tile sizes, DMA pieces), n_rep = 1 / 2 / 4 / 8 (heads stacked in the row space: with T not a multiple of 32 a
    wave's rows straddle two heads), T not a multiple of 256 (dead waves, padded rows), P + T not a multiple of 64 (the zeroed V^T tail),
    odd cases pass q as a strided view into a qkv buffer."""
    out = []
    for it, T in enumerate(T_SET):
        for ip, P in enumerate(P_SET):
            out.append((T, P, HEADS[(it + ip) % 4], DTYPES[it % 2], (it * len(P_SET) + ip) % 2 == 1))
    # ... and the other dtype at every T: f16 at the chunks with a partial last wave (257, 1000, 2303), bf16 at 512 and 2048
    out += [(257, 100, (4, 2, 64), torch.float16, True), (1000, 100, (8, 2, 128), torch.float16, True), (1000, 2049, (8, 1, 64), torch.float16, False),
            (2303, 2049, (8, 1, 64), torch.float16, False), (2303, 0, (4, 4, 128), torch.float16, True),
            (512, 2049, (8, 2, 128), torch.bfloat16, False), (2048, 100, (4, 4, 128), torch.bfloat16, False), (2048, 6144, (8, 1, 64), torch.bfloat16, True)]
    return out


def test_case_table_covers_every_head_set_in_both_dtypes():
    cs = _cases()
    assert {(c[0], c[1]) for c in cs} == {(T, P) for T in T_SET for P in P_SET}
    assert {(c[0], c[3]) for c in cs} == {(T, dt) for T in T_SET for dt in DTYPES}
    assert {(c[2], c[3]) for c in cs} == {(h, dt) for h in HEADS for dt in DTYPES}
    assert {(c[2], c[4]) for c in cs} >= {(h, True) for h in HEADS}
    assert any(c[2] == (8, 1, 64) and c[0] % 32 for c in cs)          # n_rep = 8 at d = 64 with a chunk that is no multiple of 32


def _inputs(T, P, H, Hkv, d, dtype, seed, S_max=None, strided=False, fill=0.0, k_growth=0.0):
    """k_growth: the K rows of 64-key tile i are scaled by 1 + k_growth * i (scores that keep growing along the cache)"""
    g = torch.Generator().manual_seed(seed)
    S = P + T
    S_max = S_max or (S + 63) // 64 * 64
    k = torch.full((Hkv, S_max, d), fill).to(dtype)
    v = torch.full((Hkv, S_max, d), fill).to(dtype)
    k[:, :S] = (torch.randn(Hkv, S, d, generator=g) * (1.0 + k_growth * (torch.arange(S) // 64)).view(1, S, 1)).to(dtype)
    v[:, :S] = torch.randn(Hkv, S, d, generator=g).to(dtype)
    q = torch.randn(T, H * d, generator=g).to(dtype)
    if strided:                                      # q stays inside a qkv buffer: row stride (H + 2 Hkv) d
        qkv = torch.randn(T, (H + 2 * Hkv) * d, generator=g).to(dtype)
        qkv[:, :H * d] = q
        q_dev = qkv.cuda()[:, :H * d]
        assert q_dev.stride(0) == (H + 2 * Hkv) * d
    else:
        q_dev = q.cuda()
    return q, k, v, q_dev, k.cuda().contiguous(), v.transpose(1, 2).contiguous().cuda()


def _causal(T, P):
    vis = np.zeros((T, P + T), dtype=bool)
    vis[:, :P] = True
    vis[:, P:] = np.tril(np.ones((T, T), dtype=bool))
    return vis


@pytest.mark.parametrize("T,P,heads,dtype,strided", _cases(), ids=lambda x: str(x).replace("torch.", "").replace(" ", ""))
def test_prefill_attention_vs_oracle(T, P, heads, dtype, strided):
    from lookaheaddecoding_amd import ops
    H, Hkv, d = heads
    q, k, v, qd, kd, vtd = _inputs(T, P, H, Hkv, d, dtype, seed=(T * 7 + P) % 1000, strided=strided)
    S = P + T
    lay = O.StepLayout(ids=[0] * T, positions=[], n_input=T, level_sizes=[], lguess=0, is_prefill=True, window=1)
    vis = O.dense_mask(lay, P, 1)
    assert np.array_equal(vis, _causal(T, P))
    ref = O.attention_dense(q.float().view(T, H, d).transpose(0, 1), k.float()[:, :S], v.float()[:, :S], vis).transpose(0, 1).reshape(T, H * d)
    out = ops.attn_prefill(qd, kd, vtd, ops.StepMask(T=T, P=P, is_prefill=True), H=H, Hkv=Hkv, d=d).float().cpu()
    err = (out - ref).abs().max().item()
    print(f"T={T} P={P} heads={heads} {dtype} strided={strided}: max abs err {err:.5f}")
    assert torch.isfinite(out).all()
    assert torch.allclose(out, ref, **TOL[dtype]), (T, P, heads, dtype, err)


@pytest.mark.parametrize("T,P,heads,dtype", [(300, 100, (4, 2, 64), torch.bfloat16), (512, 1536, (4, 4, 128), torch.float16),
                                             (1000, 2049, (8, 1, 64), torch.float16), (257, 0, (8, 2, 128), torch.bfloat16)],
                         ids=lambda x: str(x).replace("torch.", "").replace(" ", ""))
def test_prefill_attention_ignores_stale_cache_rows(T, P, heads, dtype):
    """S_max well above P + T, NaN in every cache row from P + T on (the chunk's last tile is partly stale in three of the four cases, and
    ends on a tile boundary in one): the output is finite and bit-identical to the run over a cache whose unused rows are zero."""
    from lookaheaddecoding_amd import ops
    H, Hkv, d = heads
    S_max = (P + T + 63) // 64 * 64 + 1024
    m = ops.StepMask(T=T, P=P, is_prefill=True)
    _, _, _, qd, kd, vtd = _inputs(T, P, H, Hkv, d, dtype, seed=5, S_max=S_max, fill=0.0)
    clean = ops.attn_prefill(qd, kd, vtd, m, H=H, Hkv=Hkv, d=d).cpu()
    _, _, _, qd2, kd2, vtd2 = _inputs(T, P, H, Hkv, d, dtype, seed=5, S_max=S_max, fill=float("nan"))
    assert torch.isnan(kd2[:, P + T:]).all() and torch.isnan(vtd2[:, :, P + T:]).all() and torch.equal(kd2[:, :P + T], kd[:, :P + T])
    stale = ops.attn_prefill(qd2, kd2, vtd2, m, H=H, Hkv=Hkv, d=d).cpu()
    assert torch.isfinite(stale.float()).all()
    assert torch.equal(stale, clean)


BITWISE = [(2065, 0, (32, 32, 128), torch.bfloat16), (2065, 100, (4, 4, 128), torch.float16), (1000, 2049, (8, 1, 64), torch.bfloat16),
           (2303, 6144, (8, 2, 128), torch.bfloat16), (257, 0, (4, 2, 64), torch.float16), (2048, 2048, (8, 8, 128), torch.bfloat16),
           (777, 70, (8, 2, 128), torch.float16), (2303, 31, (4, 1, 64), torch.bfloat16)]


# Small shapes on the same equality: a break in the arithmetic the two kernels share (csrc/attn_core.hpp) shows up in a test of a second.  The
# kernel entry point takes any T > 0 (the "more than 256 rows" rule is tuning.use_prefill_attn's, not the kernel's).
#   T=33 P=31 (2,2,64): one full wave plus a one-row wave, P inside the first 32-key sub-tile, a single tile;
#   T=70 P=90 (4,1,128): n_rep = 4 stacks 280 rows - two row blocks, waves that straddle heads, P + T = 160 leaves the last tile half stale;
#   T=96 P=0 (1,1,128): the diagonal alone, masked / unmasked sub-tile boundaries on multiples of 32;
#   T=40 P=1000 (8,8,64): unmasked cache tiles first, then the band;
#   T=64 P=448 (2,2,128) with K rows growing along the cache: the lazy rescale fires again and again (checked on the CPU before the launch).
RESCALE_GROWTH = 3.0
BITWISE_SMALL = [(33, 31, (2, 2, 64), torch.bfloat16, 0.0), (33, 31, (2, 2, 64), torch.float16, 0.0), (70, 90, (4, 1, 128), torch.bfloat16, 0.0),
                 (70, 90, (4, 1, 128), torch.float16, 0.0), (96, 0, (1, 1, 128), torch.bfloat16, 0.0), (40, 1000, (8, 8, 64), torch.float16, 0.0),
                 (64, 448, (2, 2, 128), torch.bfloat16, RESCALE_GROWTH)]
RESCALE_THR = 8.0               # csrc/attn_core.hpp: the running max (log2 units) is only raised when it grows by more


def _bitwise_id(case):
    return "-".join(str(x).replace("torch.", "").replace(" ", "") for x in (case if case[4] else case[:4]))


def _rescale_rises(q, k, T, P, H, Hkv, d):
    """Per (query row, 32-key half of a tile) state: how often the row's running max rises by more than RESCALE_THR after its first tile, under
    the kernels' rule - the 32 rows of a wave decide together (a rescale when ANY of them sees its sub-tile maximum exceed its running max by
    more than the threshold; then every row takes max(m, sub-tile max)).  Scores from the rounded inputs: q . k * scale * log2(e), causal."""
    n_rep, S = H // Hkv, P + T
    s = torch.einsum("thd,hkd->htk", q.float().view(T, H, d), k.float()[:, :S].repeat_interleave(n_rep, 0)) * (1.4426950408889634 / math.sqrt(d))
    s = s.masked_fill(~torch.as_tensor(_causal(T, P)), float("-inf"))
    n_tiles = (S + 63) // 64
    s = torch.nn.functional.pad(s, (0, n_tiles * 64 - S), value=float("-inf"))
    tmax = s.view(Hkv, n_rep * T, n_tiles, 2, 32).amax(-1)                  # [KV head][row of the (head-in-group, token) space][tile][half]
    rises = torch.zeros(Hkv, n_rep * T, 2, dtype=torch.int64)
    for r0 in range(0, n_rep * T, 32):                                      # a wave's rows (row blocks are multiples of 32 rows in both kernels)
        m = torch.full((Hkv, min(32, n_rep * T - r0), 2), -1.0e30)
        for i in range(n_tiles):
            t = tmax[:, r0:r0 + 32, i]
            own = t > m + RESCALE_THR
            fire = own.any(1, keepdim=True)
            rises[:, r0:r0 + 32] += (own & fire & (m > -1.0e29)).long()
            m = torch.where(fire, torch.maximum(m, t), m)
    return rises


BITWISE_CASES = [c + (0.0,) for c in BITWISE] + BITWISE_SMALL


@pytest.mark.parametrize("T,P,heads,dtype,k_growth", BITWISE_CASES, ids=[_bitwise_id(c) for c in BITWISE_CASES])
def test_prefill_attention_equals_the_single_launch_decode_kernel_bit_for_bit(T, P, heads, dtype, k_growth):
    """lade_attn_prefill keeps one online-softmax state per 32-key half of a tile and merges them as lade_attn_fwd's two waves of a row group
    do: its output is lade_attn_fwd's with n_splits = 1 (what the engine launched for a chunk that fills the chip by itself - bench.py's
    2065-row pass among them), bit for bit, so routing such a chunk to it changes no logit and no token.  Chunks with a partial last wave
    (T not a multiple of 32), heads stacked in the row space, P inside a tile and P = 0 are all in; so are small shapes (BITWISE_SMALL), one of
    them with K rows that grow along the cache so that the lazy rescale of a state fires at least twice more after its first tile."""
    from lookaheaddecoding_amd import ops
    H, Hkv, d = heads
    q, k, _, qd, kd, vtd = _inputs(T, P, H, Hkv, d, dtype, seed=T + P, S_max=(P + T + 63) // 64 * 64 + 128, strided=True, fill=float("nan"), k_growth=k_growth)
    if k_growth:
        rises = _rescale_rises(q, k, T, P, H, Hkv, d)
        frac = (rises >= 2).float().mean().item()
        print(f"T={T} P={P} heads={heads} growth {k_growth}: {frac:.1%} of the (row, half) states rise by more than {RESCALE_THR} at least twice; "
              f"mean {rises.float().mean().item():.2f} rises")
        assert frac > 0.75, (frac, rises.float().mean().item())
    m = ops.StepMask(T=T, P=P, is_prefill=True)
    new = ops.attn_prefill(qd, kd, vtd, m, H=H, Hkv=Hkv, d=d)
    old = ops.attn_fwd(qd, kd, vtd, m, H=H, Hkv=Hkv, d=d, n_splits=1)
    torch.cuda.synchronize()
    assert torch.isfinite(new.float()).all()
    diff = (new.float() - old.float()).abs()
    assert torch.equal(new, old), (T, P, heads, dtype, int((diff > 0).sum()), diff.max().item())


def test_prefill_attention_argument_validation():
    """what the entry point does not take is LADE_E_ARG with a message, not a crash and not another kernel"""
    from lookaheaddecoding_amd import cabi, ops
    lib = cabi.load_library()
    H = Hkv = 2
    T, P, S_max = 300, 20, 320

    def args(d=128, dtype=torch.bfloat16, **kw):
        q = torch.zeros(T, H * d, dtype=dtype, device="cuda")
        k = torch.zeros(Hkv, S_max, d, dtype=dtype, device="cuda")
        vt = torch.zeros(Hkv, d, S_max, dtype=dtype, device="cuda")
        out = torch.zeros(T, H * d, dtype=dtype, device="cuda")
        keep = [q, k, vt, out]
        mask = ops.StepMask(T=T, P=P, is_prefill=kw.pop("is_prefill", True))
        a = cabi.AttnArgs(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), None, None, None, q.stride(0), out.stride(0), H, Hkv, d, S_max,
                          ops.DTYPE_CODE_OF(dtype), 1, 1.0 / math.sqrt(d), mask.c_struct(), 0)
        for name, val in kw.items():
            setattr(a, name, val)
        return a, keep

    a, keep = args()
    assert lib.lade_attn_prefill(C.byref(a), None) == 0            # the valid form of the same arguments is accepted
    torch.cuda.synchronize()
    dynp = torch.zeros(1, dtype=torch.int32, device="cuda")
    for what, (a, keep), word in (("is_prefill = 0", args(is_prefill=False), b"is_prefill"),
                                  ("fp32", args(dtype=torch.float32), b"dtype"),
                                  ("dyn_P", args(dyn_P=dynp.data_ptr()), b"dyn_P"),
                                  ("d = 96", args(d=96), b"head_dim")):
        rc = lib.lade_attn_prefill(C.byref(a), None)
        msg = lib.lade_last_error_string()
        assert rc == -1, (what, rc)
        assert msg and b"lade_attn_prefill" in msg and word in msg, (what, msg)
    torch.cuda.synchronize()
    with pytest.raises(cabi.LadeHipError):                          # ... and through the wrapper it is an exception
        ops.attn_prefill(torch.zeros(T, H * 128, device="cuda"), torch.zeros(Hkv, S_max, 128, device="cuda"), torch.zeros(Hkv, 128, S_max, device="cuda"),
                         ops.StepMask(T=T, P=P, is_prefill=True), H=H, Hkv=Hkv, d=128)


# ---- engine level ---------------------------------------------------------------------------------------------------------------------

def _prompt(n, vocab, seed=11):
    rng = random.Random(seed)
    base = [rng.randrange(3, vocab) for _ in range(23)]
    return [base[i % len(base)] if (i // 7) % 3 else rng.randrange(3, vocab) for i in range(n)]


def _envelope(cfg, w_f32, tokens, n_rows, dtype):
    """the reference's own 16-bit error on the logits of the last n_rows tokens (test_gpu_parity_shapes._reference_bf16_envelope): the oracle in
    fp32 and with every op output rounded to `dtype`, same rounded weights, one causal pass"""
    wq = {k: v.to(dtype).float() for k, v in w_f32.items()}
    T = len(tokens)
    vis = np.tril(np.ones((T, T), dtype=bool))
    out = []
    for dt in (torch.float32, dtype):
        model = O.OracleLlama(cfg, wq, dtype=dt)
        hid = model.forward(tokens, list(range(T)), vis, model.new_cache())
        out.append(model.logits(hid[T - n_rows:]).float())
    z, z16 = out
    e = z16 - z
    return z, e.pow(2).mean().sqrt().item(), e.abs().max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", ["tiny-d128", "tiny-d64"])
def test_engine_prefill_runs_on_the_prefill_kernel(shape, dtype, monkeypatch):
    """3000-token prompt, max_T = 2048 (a 952-row and a 2048-row chunk) and max_T = 512 (five 512- / 440-row chunks and the logits chunk).
    Run with LADE_DEBUG=prefill_attn=1 and default run: (1) the logits of the last 64 rows are within the reference's 16-bit envelope of the fp32
    oracle - engine error at most 1.1 x rms and 1.25 x max of the 16-bit oracle's own error; (2) layer 0's K / V rows (they do not depend
    on attention) are bit-identical between the two runs; (3) the switched-on run reaches lade_attn_prefill once per layer and chunk, the
    default run never."""
    from lookaheaddecoding_amd import ops
    from lookaheaddecoding_amd.engine import StepEngine
    cfg = make_config(shape, max_pos=4096)
    w = {k: torch.as_tensor(v) for k, v in random_weights_numpy(cfg, seed=3, std=0.05).items()}
    n, n_rows = 3000, 64
    tokens = _prompt(n, cfg["vocab"])
    z, rms_ref, max_ref = _envelope(cfg, w, tokens, n_rows, dtype)
    rows = list(range(n - n_rows, n))
    for max_T, n_chunks in ((2048, 2), (512, 6)):
        eng = StepEngine(cfg, w, dtype=dtype, device="cuda", max_seq=3072, max_T=max_T)
        kv = {}
        for arm in ("on", "off"):                    # the kernel is behind LADE_DEBUG=prefill_attn=1; "off" is the default
            if arm == "on":
                monkeypatch.setenv("LADE_DEBUG", "prefill_attn=1")
            else:
                monkeypatch.delenv("LADE_DEBUG", raising=False)
            eng.reset()
            before = ops.PREFILL_ATTN_CALLS
            logits, done = eng.prefill(tokens, rows)
            torch.cuda.synchronize()
            calls = ops.PREFILL_ATTN_CALLS - before
            assert n - done <= max_T and (max_T != 2048 or done == 952)
            assert calls == (n_chunks * eng.L if arm == "on" else 0), (arm, max_T, calls)
            e = logits.float().cpu() - z
            rms, mx = e.pow(2).mean().sqrt().item(), e.abs().max().item()
            print(f"[{shape} {str(dtype)[6:]} max_T={max_T} {arm}] engine rms {rms:.5f} max {mx:.5f} | 16-bit oracle rms {rms_ref:.5f} max {max_ref:.5f} "
                  f"| ratios {rms / rms_ref:.3f} (bar 1.1) {mx / max_ref:.3f} (bar 1.25)")
            assert rms <= 1.1 * rms_ref and mx <= 1.25 * max_ref, (shape, dtype, max_T, arm, rms, rms_ref, mx, max_ref)
            kv[arm] = (eng.k_cache(0)[:, :n].clone(), eng.vt_cache(0)[:, :, :n].clone())
        monkeypatch.delenv("LADE_DEBUG", raising=False)
        assert torch.equal(kv["on"][0], kv["off"][0]) and torch.equal(kv["on"][1], kv["off"][1])
        del eng
