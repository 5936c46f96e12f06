"""GPU: generate(do_sample=True, ...) under USE_LADE=1 with the warpers HF builds behind top-p - min_p, typical_p, epsilon_cutoff, eta_cutoff -
on the tiny chain-walking models of tests/test_gpu_generate_scores.py (head_scale = 0.07: several tokens share the mass at temperature 0.7).
`scores` are the rows after all seven stages; they are held to the rule of tests/warp_ref.py, stage by stage, against HF's classes in fp64."""
import pytest
import torch

from test_gpu_generate_scores import PROMPT, _check_shapes, _drop_engine, _generate, _multi_token_steps, _tiny, lade_env  # noqa: F401
from warp_ref import STAGES, check_stage, hf64

pytestmark = pytest.mark.gpu

SEVEN = dict(temperature=0.7, top_k=20, top_p=0.9, min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)


@pytest.fixture(scope="module")
def soft_model():
    return _tiny("llama", torch.float32, head_scale=0.07)


def _three_warpers(logits, t, k, p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    want = logits
    for wp in (TemperatureLogitsWarper(t), TopKLogitsWarper(k), TopPLogitsWarper(p)):
        want = wp(None, want)
    return want


def _same_rows(got, want, where):
    assert torch.equal(torch.isinf(got), torch.isinf(want)), where
    keep = ~torch.isinf(want)
    assert torch.equal(got[keep], want[keep]), where


@pytest.mark.parametrize("graph", ["1", "0"], ids=["hipgraph", "eager"])
def test_all_seven_stages_in_generate(graph, soft_model, lade_env):
    from lookaheaddecoding_amd import ops
    lade, mp = lade_env
    m, n_new = soft_model, 32
    multi, new_stage_cut, compared, differing = False, 0, 0, 0
    _drop_engine(m)
    try:
        for seed in (0, 1, 2):
            torch.manual_seed(seed)
            out = _generate(m, mp, True, graph, do_sample=True, max_new_tokens=n_new, **SEVEN)
            _check_shapes(out, n_new)
            multi |= _multi_token_steps(lade)
            logits, scores = torch.cat(out.logits), torch.cat(out.scores).cpu()
            # temperature, top-k and top-p as before them: HF's three classes on the logits rows
            prev = ops.warp_rows(logits, n_new, 0, SEVEN["temperature"], SEVEN["top_k"], SEVEN["top_p"]).cpu()
            _same_rows(prev, _three_warpers(logits.cpu(), SEVEN["temperature"], SEVEN["top_k"], SEVEN["top_p"]), (graph, seed))
            first = prev
            # then every later stage against its own yardstick on the device's rows of the stages before it
            for s, stage in enumerate(STAGES):
                upto = {name: SEVEN[name] for name in STAGES[:s + 1]}
                got = ops.warp_rows(logits, n_new, 0, SEVEN["temperature"], SEVEN["top_k"], SEVEN["top_p"], **upto).cpu()
                differing += check_stage(stage, prev, got, hf64(stage, SEVEN[stage], prev), (graph, seed, stage))
                compared += n_new
                prev = got
            assert torch.equal(scores, prev), (graph, seed, "scores are not the rows after all seven stages")
            new_stage_cut += int((torch.isfinite(first) & ~torch.isfinite(scores)).sum())
            for i, tok in enumerate(out.sequences[0, len(PROMPT):].tolist()):
                assert bool(torch.isfinite(scores[i, tok])), (graph, seed, i, tok)
    finally:
        _drop_engine(m)
    assert differing <= 0.05 * compared, (differing, compared)
    assert multi, "no sampling step accepted a draft: only out rows were checked"
    assert new_stage_cut > 0, "no row lost a token to min_p / typical / epsilon / eta that top-k and top-p had kept: the test shows nothing"


@pytest.mark.parametrize("setting", [dict(min_p=1.0), dict(epsilon_cutoff=0.999)], ids=["min_p=1", "epsilon=0.999"])
def test_single_survivor_settings_sample_the_greedy_sequence(setting, soft_model, lade_env):
    lade, mp = lade_env
    m, n_new = soft_model, 24
    _drop_engine(m)
    try:
        greedy = _generate(m, mp, False, full=False, do_sample=False, max_new_tokens=n_new)
        torch.manual_seed(3)
        out = _generate(m, mp, True, do_sample=True, max_new_tokens=n_new, **setting)
    finally:
        _drop_engine(m)
    assert torch.equal(out.sequences, greedy), (setting, out.sequences.tolist(), greedy.tolist())
    for i in range(n_new):
        assert int(torch.isfinite(out.scores[i]).sum()) == 1, (setting, i)


def _tiny_qwen3():
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from test_gpu_generate_scores import CHAIN
    torch.manual_seed(0)
    m = Qwen3ForCausalLM(Qwen3Config(vocab_size=256, hidden_size=64, intermediate_size=128, num_hidden_layers=2, max_position_embeddings=512,
                                     rms_norm_eps=1e-6, pad_token_id=0, bos_token_id=1, eos_token_id=None, num_attention_heads=2,
                                     num_key_value_heads=1, head_dim=64, tie_word_embeddings=False, rope_theta=1000000.0))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.normal_(0, 0.05)
        emb = m.model.embed_tokens.weight
        emb.normal_(0, 1.0)
        succ = torch.arange(256)
        succ[torch.tensor(CHAIN)] = torch.tensor(CHAIN[1:] + CHAIN[:1])
        m.lm_head.weight[succ] = emb * 0.07
    return m.float().cuda().eval()


def test_the_qwen3_model_card_settings_run(lade_env):
    """temperature=0.6, top_k=20, top_p=0.95, min_p=0: generate() appends MinPLogitsWarper(0.0), which used to be refused"""
    lade, mp = lade_env
    m, n_new = _tiny_qwen3(), 24
    try:
        torch.manual_seed(0)
        out = _generate(m, mp, True, do_sample=True, max_new_tokens=n_new, temperature=0.6, top_k=20, top_p=0.95, min_p=0.0)
    finally:
        _drop_engine(m)
    _check_shapes(out, n_new)
    _same_rows(torch.cat(out.scores).cpu(), _three_warpers(torch.cat(out.logits).cpu(), 0.6, 20, 0.95), "qwen3")


def test_bf16_tokens_lie_in_their_kept_sets(lade_env):
    lade, mp = lade_env
    m, n_new = _tiny("llama", torch.bfloat16, head_scale=0.07), 24
    try:
        torch.manual_seed(0)
        out = _generate(m, mp, True, do_sample=True, max_new_tokens=n_new, **SEVEN)
    finally:
        _drop_engine(m)
    _check_shapes(out, n_new)
    for i, tok in enumerate(out.sequences[0, len(PROMPT):].tolist()):
        row = out.scores[i][0]
        assert bool(torch.isfinite(row[tok])) and 1 <= int(torch.isfinite(row).sum()) <= 20, (i, tok)
