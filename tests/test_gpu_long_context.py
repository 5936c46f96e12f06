"""Contexts of 8k to 32k keys on the GPU - nothing beyond 4096 keys had a test:

* the decode-shape attention pair (lade_attn_fwd with the engine's split rule + lade_attn_combine) against the CPU oracle's dense attention at
  P = 8192 / 16384 / 32768, T = 60 and 120, static launch and cache length read from the device (dyn_P), bf16 and f16, at the tolerances of
  the other attention tests;
* one end-to-end lookahead run in fp32 on a 12000-token prompt (tiny-d16, max_seq 16384): eager and hipGraph streams equal the engine's plain
  greedy stream and the CPU oracle's lookahead / plain greedy streams token for token;
* bf16 at the 7B width (2 layers) on a 9000-token prompt: 32 lookahead tokens, eager and hipGraph, each within 2.5 x max_ref of the fp32 model's best
  token for its prefix, max_ref = the 16-bit HF model's own worst logit error against the fp32 HF model on the same weights (rule (2) of DESIGN.md 5)."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import lade_oracle as O
from lookaheaddecoding_amd.weights import make_config, random_weights_numpy

TOL = {torch.bfloat16: dict(atol=2e-2, rtol=2e-2), torch.float16: dict(atol=4e-3, rtol=1e-2)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 1)])
@pytest.mark.parametrize("T", [60, 120])
@pytest.mark.parametrize("P", [8192, 16384, 32768])
def test_decode_attention_pair_at_long_context(P, T, H, Hkv, dtype):
    """W = 15, N = 5 lookahead step (60 rows; with G = 15 candidates 120) on top of P cached keys, the engine's split count for that shape
    (ops.choose_splits as KernelDecisions.n_splits_for calls it: never the single-launch form), static P and dyn_P."""
    from lookaheaddecoding_amd import ops
    d, gs = 128, 4
    ls, lguess = [14, 15, 15, 15], T - 60
    torch.manual_seed(P // 64 + T + H)
    S = P + T
    S_max = (S + 63) // 64 * 64 + 64
    lay = O.StepLayout(ids=[0] * T, positions=[], n_input=1, level_sizes=ls, lguess=lguess, is_prefill=False, window=ls[-1])
    vis = O.dense_mask(lay, P, gs)
    q = torch.randn(T, H, d).to(dtype)
    k = torch.randn(Hkv, S_max, d).to(dtype)
    v = torch.randn(Hkv, S_max, d).to(dtype)
    ref = O.attention_dense(q.float().transpose(0, 1), k.float()[:, :S], v.float()[:, :S], vis).transpose(0, 1).reshape(T, H * d)
    ns = min(ops.choose_splits(H, H // Hkv, T, max(S, 1024), 256, allow_single=False), 32)
    assert ns > 1
    qd, kd, vtd = q.reshape(T, H * d).cuda(), k.cuda().contiguous(), v.transpose(1, 2).contiguous().cuda()
    out = ops.attn_fwd(qd, kd, vtd, ops.StepMask.from_levels(1, ls, lguess, gs, P), H=H, Hkv=Hkv, d=d, n_splits=ns).float().cpu()
    err = (out - ref).abs().max().item()
    print(f"P={P} T={T} H={H} Hkv={Hkv} {dtype} n_splits={ns}: static max abs err {err:.5f}")
    assert torch.isfinite(out).all() and torch.allclose(out, ref, **TOL[dtype]), ("static", P, T, H, Hkv, dtype, ns, err)
    dyn = torch.tensor([P], dtype=torch.int32, device="cuda")
    out_d = ops.attn_fwd(qd, kd, vtd, ops.StepMask.from_levels(1, ls, lguess, gs, 0), H=H, Hkv=Hkv, d=d, n_splits=ns, dyn_P=dyn).float().cpu()
    err_d = (out_d - ref).abs().max().item()
    print(f"P={P} T={T} H={H} Hkv={Hkv} {dtype} n_splits={ns}: dyn_P  max abs err {err_d:.5f}")
    assert torch.isfinite(out_d).all() and torch.allclose(out_d, ref, **TOL[dtype]), ("dyn_P", P, T, H, Hkv, dtype, ns, err_d)


def _prompt(n, vocab, seed):
    rng = random.Random(seed)
    base = [rng.randrange(3, vocab) for _ in range(23)]
    return [base[i % len(base)] if (i // 7) % 3 else rng.randrange(3, vocab) for i in range(n)]


def test_lookahead_fp32_on_a_12000_token_prompt_equals_the_oracle():
    """fp32 tiny-d16 engine with a 16384-row cache, a seeded 12000-token prompt, 96 new tokens with W = 5, N = 3, G = 5: the eager and the
    hipGraph lookahead streams, the engine's plain greedy stream and the CPU oracle's lookahead and plain greedy streams are one and the
    same token sequence, and the lookahead step counts equal the oracle's.  (The oracle's prefill is one dense forward: about 6.5 GB of
    host memory at this length.)"""
    from lookaheaddecoding_amd.decoding import LookaheadDecoder
    from lookaheaddecoding_amd.engine import StepEngine
    cfg = make_config("tiny-d16", max_pos=16384)
    w = {k: torch.as_tensor(v) for k, v in random_weights_numpy(cfg, seed=2, std=0.05).items()}
    n_prompt, n_new, (W, N, G) = 12000, 96, (5, 3, 5)
    prompt = _prompt(n_prompt, cfg["vocab"], seed=7)
    model = O.OracleLlama(cfg, w)
    ref_plain = O.plain_greedy(model, prompt, n_prompt + n_new)
    ref = O.lookahead_greedy(model, prompt, W, N, G, n_prompt + n_new, random.Random(4))
    assert ref.tokens == ref_plain
    eng = StepEngine(cfg, w, dtype=torch.float32, device="cuda", max_seq=16384, max_T=512)
    assert eng.plain_greedy(prompt, n_prompt + n_new) == ref_plain
    for use_graph in (False, True):
        out = LookaheadDecoder(eng, W, N, G, use_graph=use_graph).greedy(prompt, n_prompt + n_new, rng=random.Random(4))
        assert out.tokens == ref.tokens and out.steps == ref.steps, (use_graph, out.steps, ref.steps,
                                                                     [i for i, (a, b) in enumerate(zip(out.tokens, ref.tokens)) if a != b][:4])
        assert out.generated == n_new and out.steps < n_new


def _hf_llama(dtype):
    from transformers import LlamaConfig, LlamaForCausalLM
    p = make_config("llama2-7b")
    torch.manual_seed(3)
    with torch.device("cuda"):
        m = LlamaForCausalLM(LlamaConfig(vocab_size=p["vocab"], hidden_size=p["hidden"], intermediate_size=p["inter"], num_hidden_layers=2,
                                         num_attention_heads=p["heads"], num_key_value_heads=p["kv_heads"], max_position_embeddings=16384,
                                         rms_norm_eps=p["eps"], rope_theta=p["rope_theta"], tie_word_embeddings=False))
    with torch.no_grad():
        for prm in m.parameters():
            if prm.dim() > 1:
                prm.normal_(0, 0.02)
        for prm in m.parameters():
            prm.copy_(prm.bfloat16().float())              # the fp32 model runs on the bf16 model's weights
    return m.to(dtype).eval()


def _hf_logits(model, tokens, n_prompt):
    """logits of the generated positions only: the hidden states of the whole sequence, lm_head on the rows that predict a generated token"""
    with torch.no_grad():
        hid = model.model(torch.tensor([tokens[:-1]], device="cuda")).last_hidden_state[0, n_prompt - 1:]
        return model.lm_head(hid).float()


def test_bf16_7b_width_lookahead_on_a_9000_token_prompt():
    from lookaheaddecoding_amd import hf
    from lookaheaddecoding_amd.decoding import LookaheadDecoder
    from lookaheaddecoding_amd.engine import StepEngine
    m32 = _hf_llama(torch.float32)
    m16 = _hf_llama(torch.bfloat16)
    cfg = hf.config_from_hf(m16)
    rng = random.Random(11)
    n_prompt, n_new = 9000, 32
    prompt = [rng.randrange(3, 32000) for _ in range(n_prompt)]
    eng = StepEngine(cfg, hf.weights_from_hf(m16), dtype=torch.bfloat16, device="cuda", max_seq=9472, max_T=2048)
    outs = {g: LookaheadDecoder(eng, 15, 5, 15, use_graph=g).greedy(prompt, n_prompt + n_new, rng=random.Random(1)).tokens for g in (False, True)}
    tokens = outs[False]
    assert len(tokens) == n_prompt + n_new
    z32 = _hf_logits(m32, tokens, n_prompt)
    max_ref = (_hf_logits(m16, tokens, n_prompt) - z32).abs().max().item()
    for g, toks in outs.items():
        z = z32 if toks == tokens else _hf_logits(m32, toks, n_prompt)
        worst = 0.0
        for j in range(n_new):
            deficit = (z[j].max() - z[j, toks[n_prompt + j]]).item()
            worst = max(worst, deficit)
            assert deficit <= 2.5 * max_ref, ("graph" if g else "eager", j, deficit, max_ref)
        print(f"[7B width, 9000-token prompt, {'hipGraph' if g else 'eager'}] worst deficit against the fp32 model's best token {worst:.4f} "
              f"(allowed 2.5 x the bf16 model's own worst logit error {max_ref:.4f})")
