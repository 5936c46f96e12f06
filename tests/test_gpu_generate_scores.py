"""GPU: generate(return_dict_in_generate=True, output_scores=True, output_logits=True) under USE_LADE=1 - HF's GenerateDecoderOnlyOutput
with one fp32 [1, V] row per generated token, from the rows that decided the tokens of each lookahead step (lade_emit_rows).

Tiny random models (2 layers, hidden 64, vocab 256), LEVEL=4, WINDOW_SIZE=5, GUESS_SET_SIZE=5, POOL_FROM_PROMPT=1, a prompt with repeats.
The embeddings are large against the other weights and the lm_head row of token succ(t) is the embedding of t, succ = one random cycle
through the vocabulary: the stream walks that cycle (every token differs from its neighbours, so a row taken from the wrong candidate
position shows), and the window's guesses converge onto it, so steps accept n-grams.  Every greedy case asserts that at least one step
emitted more than one token: otherwise only out rows would be checked.

fp32 greedy parity bound (derived, not chosen): the yardstick is HF alone.  d_ref = the largest difference between the `logits` HF's own
incremental decoding returns and ONE teacher-forced forward over the final sequence - the same numbers computed in two batch shapes.  A
lookahead row is computed in a third batch shape (and by other kernels), so two such independent differences add: 2 * d_ref; the bound is
4 * d_ref, a factor 2 over that sum.  Both numbers are appended to profiles/generate_scores_parity.txt."""
import os
import random

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHAIN = (torch.randperm(254, generator=torch.Generator().manual_seed(5)) + 2).tolist()      # the cycle the models walk (ids 0 / 1: pad / bos)
PROMPT = [1] + CHAIN[:6] + [CHAIN[20]] + CHAIN[:3]          # ends inside a 6-gram it has shown before: the pool holds the continuation
LADE = dict(LEVEL=4, WINDOW_SIZE=5, GUESS_SET_SIZE=5, POOL_FROM_PROMPT=1, DEBUG=1)
PARITY_FILE = os.path.join(ROOT, "profiles", "generate_scores_parity.txt")


def _tiny(family="llama", dtype=torch.float32, head_scale=1.0):
    """head_scale: how sharply the logits single out the successor (1.0: by ~60, greedy never leaves the cycle; 0.07: a few tokens share the
    probability mass at temperature 0.7, so the sampling warpers keep more than one)"""
    torch.manual_seed(0)
    common = dict(vocab_size=256, hidden_size=64, intermediate_size=128, num_hidden_layers=2, max_position_embeddings=512, rms_norm_eps=1e-6,
                  pad_token_id=0, bos_token_id=1, eos_token_id=None, num_attention_heads=2, num_key_value_heads=1, head_dim=64)
    if family == "qwen2":
        from transformers import Qwen2Config, Qwen2ForCausalLM
        m = Qwen2ForCausalLM(Qwen2Config(**common, tie_word_embeddings=False, rope_theta=1000000.0))
    else:
        from transformers import LlamaConfig, LlamaForCausalLM
        m = LlamaForCausalLM(LlamaConfig(**common, tie_word_embeddings=False))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(".bias"):
                p.normal_(0, 0.5)
            elif p.dim() > 1:
                p.normal_(0, 0.05)
        emb = m.model.embed_tokens.weight
        emb.normal_(0, 1.0)
        succ = torch.arange(256)
        succ[torch.tensor(CHAIN)] = torch.tensor(CHAIN[1:] + CHAIN[:1])
        m.lm_head.weight[succ] = emb * head_scale
    return m.to(dtype).cuda().eval()


def _drop_engine(m):
    for attr in ("_lade_decoder", "_lade_engine"):
        if attr in m.__dict__:
            del m.__dict__[attr]


@pytest.fixture
def lade_env(monkeypatch):
    import lade
    from transformers import GenerationMixin
    orig = GenerationMixin._sample
    monkeypatch.delenv("USE_LADE", raising=False)
    lade.augment_all()
    lade.config_lade(**LADE)
    yield lade, monkeypatch
    GenerationMixin._sample = orig
    lade.decoding.FUNC_MAP.pop("_sample", None)
    lade.decoding.CONFIG_MAP.clear()


class _Steps:
    """a streamer that records what each step handed over (generate() itself puts the prompt first, as a 2-D tensor)"""

    def __init__(self):
        self.steps = []

    def put(self, value):
        if value.dim() == 1:
            self.steps.append(value.tolist())

    def end(self):
        pass


def _generate(m, mp, use_lade, graph="1", full=True, **kw):
    prompt = torch.tensor([PROMPT], device="cuda")
    if use_lade:
        mp.setenv("USE_LADE", "1")
    else:
        mp.delenv("USE_LADE", raising=False)
    mp.setenv("LADE_GRAPH", graph)
    random.seed(1)
    if full:
        kw = dict(return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
    try:
        return m.generate(prompt, attention_mask=torch.ones_like(prompt), **kw)
    finally:
        mp.delenv("USE_LADE", raising=False)


def _multi_token_steps(lade):
    gen, steps, _ = lade.decoding.CONFIG_MAP["log"][-1]
    return steps < gen


def _check_shapes(out, n_new, V=256):
    assert type(out).__name__ == "GenerateDecoderOnlyOutput" and out.past_key_values is None
    assert out.sequences.shape == (1, len(PROMPT) + n_new)
    for t in (out.scores, out.logits):
        assert isinstance(t, tuple) and len(t) == n_new
        for row in t:
            assert row.shape == (1, V) and row.dtype == torch.float32 and row.is_cuda


_HF_FP32 = {}


def _hf_fp32_reference(m, mp, n_new):
    """plain HF greedy (USE_LADE=0) on the fp32 model: its output object and d_ref (module docstring); computed once"""
    if "out" not in _HF_FP32:
        plain = _generate(m, mp, False, do_sample=False, max_new_tokens=n_new)
        inc = torch.cat(plain.logits).float()
        with torch.no_grad():
            tf = m(plain.sequences).logits[0, len(PROMPT) - 1:-1].float()
        _HF_FP32["out"], _HF_FP32["inc"], _HF_FP32["d_ref"] = plain, inc, float((inc - tf).abs().max())
    return _HF_FP32["out"], _HF_FP32["inc"], _HF_FP32["d_ref"]


@pytest.fixture(scope="module")
def fp32_model():
    return _tiny("llama", torch.float32)


@pytest.mark.parametrize("graph", ["1", "0"], ids=["hipgraph", "eager"])
def test_fp32_greedy_scores_and_logits_against_plain_hf(graph, fp32_model, lade_env):
    lade, mp = lade_env
    m, n_new = fp32_model, 40
    plain, inc, d_ref = _hf_fp32_reference(m, mp, n_new)
    _drop_engine(m)
    try:
        out = _generate(m, mp, True, graph, do_sample=False, max_new_tokens=n_new)
    finally:
        _drop_engine(m)
    assert _multi_token_steps(lade), "no step emitted more than one token: only out rows would be checked"
    assert torch.equal(out.sequences, plain.sequences)
    _check_shapes(out, n_new)
    new = out.sequences[0, len(PROMPT):].tolist()
    for i, tok in enumerate(new):
        assert int(out.scores[i].argmax()) == tok, (graph, i)
        assert torch.equal(out.scores[i], out.logits[i]), (graph, i)
    d = float((torch.cat(out.logits) - inc).abs().max())
    print(f"fp32 greedy parity ({graph}): lookahead rows vs HF incremental logits {d:.3e}, d_ref {d_ref:.3e}, bound 4 * d_ref {4 * d_ref:.3e}")
    with open(PARITY_FILE, "a") as f:
        f.write(f"LADE_GRAPH={graph} tokens={n_new} max|lookahead - hf_incremental|={d:.6e} d_ref=max|hf_incremental - hf_teacher_forced|={d_ref:.6e} "
                f"bound=4*d_ref={4 * d_ref:.6e}\n")
    assert d <= 4 * d_ref, (graph, d, d_ref)


@pytest.mark.parametrize("graph", ["1", "0"], ids=["hipgraph", "eager"])
def test_bf16_greedy_scores_are_hf_processors_of_our_logits(graph, lade_env):
    """repetition_penalty=1.3, min_new_tokens=6: scores[i] = HF's own processor objects applied on the GPU to logits[i] with the input_ids
    plain decoding would have, bit for bit (the bar tests/test_gpu_gen_controls.py holds lade_gen_rows to); logits are bf16 values"""
    from transformers.generation.logits_process import MinNewTokensLengthLogitsProcessor, RepetitionPenaltyLogitsProcessor
    lade, mp = lade_env
    m, n_new, min_new = _tiny("llama", torch.bfloat16), 40, 6
    # an EOS id far along the cycle: the stream stays on the stretch of the cycle the pool knows (a masked token in its way would send it
    # elsewhere and no candidate would match again); the mask still shows in the score rows.  The penalty hits CHAIN[20], seen in the prompt
    eos = CHAIN[200]
    try:
        out = _generate(m, mp, True, graph, do_sample=False, max_new_tokens=n_new, repetition_penalty=1.3, min_new_tokens=min_new, eos_token_id=eos)
    finally:
        _drop_engine(m)
    assert _multi_token_steps(lade)
    new = out.sequences[0, len(PROMPT):].tolist()
    _check_shapes(out, len(new))
    assert len(new) == n_new and CHAIN[20] in new
    rep = RepetitionPenaltyLogitsProcessor(1.3)
    mnl = MinNewTokensLengthLogitsProcessor(len(PROMPT), min_new, torch.tensor([eos], device="cuda"), device="cuda")
    masked = 0
    for i, tok in enumerate(new):
        ids = out.sequences[:, :len(PROMPT) + i]
        want = mnl(ids, rep(ids, out.logits[i].clone()))
        assert torch.equal(out.scores[i], want), (graph, i, (out.scores[i] != want).nonzero().tolist()[:4])
        assert torch.equal(out.logits[i].to(torch.bfloat16).float(), out.logits[i]), (graph, i)
        assert int(out.scores[i].argmax()) == tok, (graph, i)
        masked += int(torch.isinf(out.scores[i][0, eos]))
    assert masked == min_new, "the min-length mask must show in exactly the first min_new_tokens score rows"


def test_sampling_scores_are_the_warped_rows(fp32_model, lade_env):
    """temperature=0.7, top_k=20, top_p=0.9: scores[i] against HF's three warper objects applied to logits[i] - the same -inf pattern, the
    kept entries bit-equal (the comparison tests/test_gpu_kernels.py::test_warp_rows_equals_the_hf_warpers makes, on CPU tensors like there)"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    lade, mp = lade_env
    m, n_new = _tiny("llama", torch.float32, head_scale=0.07), 32
    warpers = (TemperatureLogitsWarper(0.7), TopKLogitsWarper(20), TopPLogitsWarper(0.9))
    kept, multi = [], False
    try:
        for graph, seed in (("1", 0), ("0", 1), ("1", 2)):
            torch.manual_seed(seed)
            out = _generate(m, mp, True, graph, do_sample=True, temperature=0.7, top_k=20, top_p=0.9, max_new_tokens=n_new)
            _check_shapes(out, n_new)
            multi |= _multi_token_steps(lade)
            new = out.sequences[0, len(PROMPT):].tolist()
            for i, tok in enumerate(new):
                want = out.logits[i].cpu()
                for wp in warpers:
                    want = wp(None, want)
                got = out.scores[i].cpu()
                assert torch.equal(torch.isinf(got), torch.isinf(want)), (graph, seed, i)
                keep = ~torch.isinf(want)
                assert 1 <= int(keep.sum()) <= 20 and torch.equal(got[keep], want[keep]), (graph, seed, i)
                kept.append(int(keep.sum()))
                assert bool(torch.isfinite(got[0, tok])), (graph, seed, i, tok)
            ts = m.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
            assert ts.shape == (1, n_new) and bool(torch.isfinite(ts).all()), (graph, seed, ts)
    finally:
        _drop_engine(m)
    assert max(kept) > 1, "every row kept one token: the -inf patterns would not tell top-k / top-p from a plain argmax"
    assert multi, "no sampling step accepted a draft: only out rows were checked"


def test_eos_inside_a_multi_token_step_drops_its_rows(fp32_model, lade_env):
    lade, mp = lade_env
    m, n_new = fp32_model, 40
    _drop_engine(m)
    try:
        rec = _Steps()
        plain = _generate(m, mp, True, full=False, do_sample=False, max_new_tokens=n_new, streamer=rec)[0, len(PROMPT):].tolist()
        assert [t for s in rec.steps for t in s] == plain
        pick, at = None, 0
        for s in rec.steps:                                # a token in the middle of a multi-token step that the stream has not emitted before
            for j, tok in enumerate(s[:-1]):
                if len(s) > 1 and tok not in plain[:at + j] and pick is None:
                    pick = (tok, at + j, len(s) - 1 - j)
            at += len(s)
        assert pick is not None, ("no multi-token step with a fresh token before its end", rec.steps)
        eos, pos, dropped = pick
        out = _generate(m, mp, True, do_sample=False, max_new_tokens=n_new, eos_token_id=eos)
    finally:
        _drop_engine(m)
    new = out.sequences[0, len(PROMPT):].tolist()
    assert new == plain[:pos + 1] and dropped >= 1 and len(set(plain)) > 20
    _check_shapes(out, pos + 1)
    for i, tok in enumerate(new):
        assert int(out.scores[i].argmax()) == tok


def test_emit_on_off_on_with_one_decoder(fp32_model, lade_env):
    """three calls on one model (one decoder, hipGraph steps): the switch re-captures, a second emit call only rewrites the descriptor"""
    lade, mp = lade_env
    m = fp32_model
    plain, _, _ = _hf_fp32_reference(m, mp, 40)
    want = plain.sequences[0].tolist()
    _drop_engine(m)
    try:
        a = _generate(m, mp, True, do_sample=False, max_new_tokens=20)
        dec = m._lade_decoder
        key_on = dec._graph_key
        b = _generate(m, mp, True, full=False, do_sample=False, max_new_tokens=30)
        key_off = dec._graph_key
        c = _generate(m, mp, True, do_sample=False, max_new_tokens=25)
        d = _generate(m, mp, True, do_sample=False, max_new_tokens=33)
        assert m._lade_decoder is dec and key_on is not None and key_on != key_off and dec._graph_key == key_on
    finally:
        _drop_engine(m)
    assert torch.is_tensor(b) and b[0].tolist() == want[:len(PROMPT) + 30]
    for out, n in ((a, 20), (c, 25), (d, 33)):
        assert out.sequences[0].tolist() == want[:len(PROMPT) + n]
        _check_shapes(out, n)
        for i in range(n):
            assert int(out.scores[i].argmax()) == want[len(PROMPT) + i], (n, i)
            assert torch.equal(out.scores[i], out.logits[i])
    # the rows of an earlier call stay what they were: every call gets buffers of its own
    assert torch.equal(torch.cat(a.logits), torch.cat(d.logits)[:20])


def test_qwen2_bf16_logits_only(lade_env):
    lade, mp = lade_env
    m, n_new = _tiny("qwen2", torch.bfloat16), 24
    prompt = torch.tensor([PROMPT], device="cuda")
    mp.setenv("USE_LADE", "1")
    random.seed(1)
    try:
        out = m.generate(prompt, attention_mask=torch.ones_like(prompt), do_sample=False, max_new_tokens=n_new, return_dict_in_generate=True,
                         output_logits=True)
    finally:
        _drop_engine(m)
    assert out.scores is None and isinstance(out.logits, tuple) and len(out.logits) == n_new
    new = out.sequences[0, len(PROMPT):].tolist()
    for i, tok in enumerate(new):
        row = out.logits[i]
        assert row.shape == (1, 256) and row.dtype == torch.float32
        assert int(row.argmax()) == tok and torch.equal(row.to(torch.bfloat16).float(), row), i


def test_lookahead_parallelism_refuses_return_dict_in_generate(fp32_model, lade_env):
    from lookaheaddecoding_amd import cabi
    lade, mp = lade_env
    m = fp32_model
    prompt = torch.tensor([PROMPT], device="cuda")
    _drop_engine(m)
    mp.setenv("USE_LADE", "1")
    lade.decoding.CONFIG_MAP["FORCE_LP"] = 1
    try:
        with pytest.raises(cabi.LadeHipError, match="return_dict_in_generate"):
            m.generate(prompt, attention_mask=torch.ones_like(prompt), do_sample=False, max_new_tokens=8, return_dict_in_generate=True, output_scores=True)
        with pytest.raises(cabi.LadeHipError, match="output_attentions"):
            lade.decoding.CONFIG_MAP["FORCE_LP"] = 0
            m.generate(prompt, attention_mask=torch.ones_like(prompt), do_sample=False, max_new_tokens=8, return_dict_in_generate=True,
                       output_attentions=True)
    finally:
        _drop_engine(m)
