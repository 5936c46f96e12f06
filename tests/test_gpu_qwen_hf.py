"""GPU: Qwen2 (q / k / v bias) and Qwen3 (per-head q / k RMSNorm, H * d != hidden) end to end.
(a) fp32: lade.augment_all(); USE_LADE=1 model.generate() on tiny HF models with randomised biases and norm weights (HF initialises them
    to 0 / 1, which would hide both) equals plain HF greedy token for token - two lookahead settings, hipGraph on and off - and sampling runs.
(b) bf16 at the Qwen2.5-7B / Qwen3-8B widths (3 layers): the engine's logits against HF's fp32 model on the same (bf16-rounded) weights
    stay within HF's own bf16 error envelope - through a wide prefill (library GEMM + addmm bias) and through 64-row chunks on the split-K
    GEMM (the epilogue inside the partials kernel) - and every lookahead token, eager and hipGraph, is a near-best token of the fp32 model."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu


def _randomise(model, std):
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("q_norm.weight") or name.endswith("k_norm.weight"):
                p.copy_(1 + 0.2 * torch.randn_like(p))
            elif name.endswith(".bias"):
                p.normal_(0, 0.5)
            elif p.dim() > 1:
                p.normal_(0, std)
    return model


def _tiny(family):
    torch.manual_seed(0)
    common = dict(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512, rms_norm_eps=1e-6,
                  tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=None, rope_theta=1000000.0)
    if family == "qwen2":
        from transformers import Qwen2Config, Qwen2ForCausalLM
        m = Qwen2ForCausalLM(Qwen2Config(**common, num_attention_heads=2, num_key_value_heads=1))
    else:
        from transformers import Qwen3Config, Qwen3ForCausalLM
        m = Qwen3ForCausalLM(Qwen3Config(**common, num_attention_heads=4, num_key_value_heads=2, head_dim=64))      # H * d = 256 != 128
    return _randomise(m, 0.05).float().cuda().eval()


def _drop_engine(m):
    for attr in ("_lade_decoder", "_lade_engine"):
        if attr in m.__dict__:
            del m.__dict__[attr]


@pytest.mark.parametrize("family", ["qwen2", "qwen3"])
def test_fp32_generate_with_use_lade_equals_plain_hf_greedy(family, monkeypatch):
    import lade
    from transformers import GenerationMixin
    m = _tiny(family)
    orig = GenerationMixin._sample
    prompt = torch.tensor([[1, 5, 9, 17, 33, 5, 9, 17, 44, 5, 9, 17, 33, 5]], device="cuda")
    mask = torch.ones_like(prompt)
    n_new = 56
    try:
        monkeypatch.delenv("USE_LADE", raising=False)
        plain = m.generate(prompt, attention_mask=mask, do_sample=False, max_new_tokens=n_new)
        lade.augment_all()
        monkeypatch.setenv("USE_LADE", "1")
        for (W, N, G, extra) in ((5, 4, 5, {}), (7, 3, 7, dict(POOL_FROM_PROMPT=1, USE_FLASH=1))):
            for graph in ("0", "1"):
                monkeypatch.setenv("LADE_GRAPH", graph)
                _drop_engine(m)
                lade.config_lade(LEVEL=N, WINDOW_SIZE=W, GUESS_SET_SIZE=G, DEBUG=1, **extra)
                random.seed(1)
                out = m.generate(prompt, attention_mask=mask, do_sample=False, max_new_tokens=n_new)
                assert out.shape == plain.shape and torch.equal(out, plain), (family, W, N, G, graph, out.tolist(), plain.tolist())
                gen, steps, _ratio = lade.decoding.CONFIG_MAP["log"][-1]
                assert gen == n_new and steps <= n_new
        random.seed(2)
        smp = m.generate(prompt, attention_mask=mask, do_sample=True, temperature=0.7, top_k=0, top_p=1.0, max_new_tokens=24)
        assert smp.shape[1] == prompt.shape[1] + 24 and int(smp.max()) < 256
    finally:
        GenerationMixin._sample = orig
        lade.decoding.FUNC_MAP.pop("_sample", None)
        lade.decoding.CONFIG_MAP.clear()
        _drop_engine(m)


# ---- (b) full width, 3 layers, bf16 ------------------------------------------------------------------------------------------

def _wide(preset):
    from lookaheaddecoding_amd.weights import make_config
    p = make_config(preset)
    common = dict(vocab_size=p["vocab"], hidden_size=p["hidden"], intermediate_size=p["inter"], num_hidden_layers=3, num_attention_heads=p["heads"],
                  num_key_value_heads=p["kv_heads"], max_position_embeddings=4096, rms_norm_eps=p["eps"], rope_theta=p["rope_theta"],
                  tie_word_embeddings=False)
    torch.manual_seed(3)
    with torch.device("cuda"):
        if preset.startswith("qwen2"):
            from transformers import Qwen2Config, Qwen2ForCausalLM
            m = Qwen2ForCausalLM(Qwen2Config(**common))
        else:
            from transformers import Qwen3Config, Qwen3ForCausalLM
            m = Qwen3ForCausalLM(Qwen3Config(**common, head_dim=p["head_dim"]))
    _randomise(m, 0.02)
    with torch.no_grad():
        for prm in m.parameters():
            prm.copy_(prm.bfloat16().float())             # the fp32 model runs on the bf16 model's weights
    return m.eval()


def _logits(model, tokens, n_prompt):
    with torch.no_grad():
        out = model(torch.tensor([tokens[:-1]], device="cuda")).logits[0, n_prompt - 1:]
    return out.float()


@pytest.mark.parametrize("preset", ["qwen2.5-7b", "qwen3-8b"])
def test_bf16_full_width_within_hf_bf16_envelope(preset, monkeypatch):
    from lookaheaddecoding_amd import hf
    from lookaheaddecoding_amd.decoding import LookaheadDecoder
    from lookaheaddecoding_amd.engine import StepEngine
    m32 = _wide(preset)
    m16 = _wide(preset).to(torch.bfloat16)
    cfg = hf.config_from_hf(m16)
    rng = random.Random(11)
    n_prompt, n_new = 300, 32
    prompt = [rng.randrange(3, 150000) for _ in range(n_prompt)]
    # lookahead tokens, eager and hipGraph (the prefill of 300 rows is one wide chunk: library GEMM, addmm bias, norm-only epilogue)
    eng = StepEngine(cfg, hf.weights_from_hf(m16), dtype=torch.bfloat16, device="cuda", max_seq=1024, max_T=512)
    outs = {g: LookaheadDecoder(eng, 15, 5, 15, use_graph=g).greedy(prompt, n_prompt + n_new, rng=random.Random(1)).tokens for g in (False, True)}
    tokens = outs[False]
    # HF's own bf16 error on these tokens = the envelope
    z32 = _logits(m32, tokens, n_prompt)
    e_ref = _logits(m16, tokens, n_prompt) - z32
    rms_ref, max_ref = e_ref.pow(2).mean().sqrt().item(), e_ref.abs().max().item()
    rows = list(range(n_prompt - 1, len(tokens) - 1))

    def within(e_logits, tag):
        e = e_logits.float() - z32
        rms, mx = e.pow(2).mean().sqrt().item(), e.abs().max().item()
        print(f"[{preset} {tag}] engine rms {rms:.4f} max {mx:.4f} | HF bf16 rms {rms_ref:.4f} max {max_ref:.4f} | ratios {rms / rms_ref:.3f} {mx / max_ref:.3f}")
        assert rms <= 1.1 * rms_ref and mx <= 1.25 * max_ref, (preset, tag, rms, rms_ref, mx, max_ref)

    eng.reset()
    logits, done = eng.prefill(tokens[:-1], rows)
    assert done == 0                                       # one wide chunk: the library path
    within(logits, "wide prefill")
    # 64-row chunks on the split-K GEMM (K-tile-major weights only: the library is no candidate at decode widths)
    monkeypatch.setenv("LADE_W_KTILE", "only")
    eng64 = StepEngine(cfg, hf.weights_from_hf(m16), dtype=torch.bfloat16, device="cuda", max_seq=1024, max_T=64)
    logits64, done64 = eng64.prefill(tokens[:-1], rows)
    assert done64 > 0 and eng64.gemm_cfg.get(("wqkv", 64)) is not None         # the last chunk ran the qkv GEMM split-K
    within(logits64, "64-row split-K chunks")
    del eng64
    # every lookahead token is a near-best token of the fp32 model for its prefix
    for g, toks in outs.items():
        z = z32 if toks == tokens else _logits(m32, toks, n_prompt)
        for j in range(n_new):
            deficit = (z[j].max() - z[j, toks[n_prompt + j]]).item()
            assert deficit <= 2.5 * max_ref, (preset, "graph" if g else "eager", j, deficit, max_ref)
