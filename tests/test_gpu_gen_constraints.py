"""GPU: HF's token constraints (bad_words_ids, suppress_tokens, begin_suppress_tokens, sequence_bias) on the lookahead step.
(1) lade_gen_argmax / lade_gen_rows with a constraint block attached against HF's own processor objects, applied on the GPU in HF's order
    (SequenceBias, RepetitionPenalty, NoBadWords, MinLength, SuppressTokens, SuppressTokensAtBegin) to the widened fp32 rows, each row with
    the input_ids it has in plain decoding: the argmax and the fp32 rows bit for bit (compared as int32 words: -0.0 is not +0.0).  Window
    rows are held to what the device step gives them: the bans and the length-1 biases.  Without a block the kernels return the bits of
    the penalty / min-length pipeline alone.  The block's tail follows lade_gen_ctl_update.
(2) fp32 greedy end to end on the tiny Llama of tests/test_gpu_hf.py: USE_LADE=1 generate() equals plain HF token for token under each
    setting and all of them together, two lookahead settings, hipGraph on and off; the constraints are derived from the model's own
    unconstrained output and must change it.  A copy-biased model adds steps that accept candidate rows.
(3) consecutive calls with different constraint sets on one decoder; sampling `scores` against HF's processors + warpers of the `logits`;
    lookahead parallelism refuses."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

NEG_INF = -float("inf")
A_POS, B_NEG, T1, T2, T3, T4, T5, W1, W2, S1, S2, B1, NEVER = 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 99


def _bits(t):
    return t.contiguous().view(torch.int32)


def _constraint_set(full, guess, V):
    """Entries of length 1 to 4 and 16; two entries with different prefixes that end in T1 and fire on the out row, plus T1's length-1 bias
    placed behind them in the dict; finite positive and negative biases; -inf on the out row's winner (W2, a two-token bad word) and on a
    candidate row's winner (T2, its prefix straddles the accepted tail and guess[0][0..1]); entries longer than a 2-token context."""
    g0, g1 = guess[0].tolist(), guess[1].tolist()
    pre15 = ([60] * 15 + full)[-15:]
    pre13 = ([61] * 13 + full)[-13:]
    sequence_bias = {
        (A_POS,): 2.0,
        (full[-1], T1): 3.0,
        (full[-2], full[-1], T1): -0.75,
        (B_NEG,): -1.5,
        (T1,): 0.5,
        (NEVER, T1): 100.0,                                     # a prefix no row has
        (g1[0], T3): 4.0,                                       # candidate 1, position 0: the prefix is the candidate's own token
        tuple(pre15) + (T4,): 1.25,                             # length 16, the out row
        tuple(pre13) + (g0[0], g0[1], T5): -2.5,                # length 16, straddling
        (full[-1], g0[0], g0[1], T2): NEG_INF,                  # length 4, straddling, on the token that would win
        (full[-1], g0[0], T5): 0.125,
    }
    bad_words = [[W1], [full[-1], W2], [V - 2]]
    suppress = [S1, S2, V - 3]
    return sequence_bias, bad_words, suppress


def _hf_rows(logits, seqs, procs_of_row):
    out = []
    for r, ids in enumerate(seqs):
        scores = logits[r:r + 1].float()
        ids_t = torch.tensor([ids], dtype=torch.long, device="cuda")
        for p in procs_of_row(r):
            scores = p(ids_t, scores)
        out.append(scores)
    return torch.cat(out)


@pytest.mark.parametrize("V", [256, 257, 32000, 152064])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_constrained_rows_match_hf_processors(V, dtype):
    from transformers.generation import logits_process as lp
    from lookaheaddecoding_amd import cabi, ops
    from lookaheaddecoding_amd.decoding import GenControls
    from lookaheaddecoding_amd.hf import controls_from_processors
    gen_t = torch.Generator().manual_seed(V + 1)
    gs, n_inp, n_slots, g = 3, 4, 3, 2                       # 2 real candidates, slot 2 is padding
    rows = 1 + n_inp + n_slots * gs
    eos = [V - 1, 3]
    penalty = 1.3
    pad = 5 if V % 8 else 0
    base_logits = (torch.randint(-8, 9, (rows, V + pad), generator=gen_t).float() * 0.5).to(dtype)
    base_logits[:, 100:140:3] = -0.0                        # HF's `scores + bias` turns them into +0.0: part of the bits
    guess = torch.randint(0, 40, (n_slots, gs), generator=gen_t)
    guess_d = guess.flatten().to(torch.int32).cuda()
    ctl = torch.zeros(cabi.CTL_WORDS, dtype=torch.int32, device="cuda")
    gen = torch.zeros(cabi.gen_words(V), dtype=torch.int32, device="cuda")
    cons = torch.zeros(cabi.gen_cons_words(V), dtype=torch.int32, device="cuda")
    drawn = torch.randint(0, 40, (40,), generator=gen_t).tolist()
    # (prompt, accepted chunks): a long context whose tail has rolled, a 2-token prompt (entries longer than the context), and a 2-token
    # prompt followed by two updates that fill the tail and push it over its 15 slots
    scenarios = ((drawn[:17] + [7, 7], [[V - 1, drawn[20], drawn[21]]]), (drawn[:2], []), (drawn[2:4], [drawn[4:7], drawn[7:21]]))
    for prompt, chunks in scenarios:
        full = prompt + [t for ch in chunks for t in ch]
        n_seen = len(full)
        min_len = n_seen + 2
        logits = base_logits.clone()
        c0j1 = 1 + n_inp + 0 * gs + 1
        logits[:, [A_POS, B_NEG, T1, T3, T4, T5]] = 4.0
        logits[:, eos] = 4.5
        logits[0, W2] = 9.0                                 # the out row's winner, banned by the two-token bad word
        logits[0, B1] = 8.0                                 # ... the next one, banned at the begin index
        logits[c0j1, T2] = 9.0                              # the winner of candidate 0, position 1
        logits[c0j1, B1] = 8.0                              # not at the begin index: it wins there
        logits = logits.cuda()[:, :V]
        sequence_bias, bad_words, suppress = _constraint_set(full, guess, V)
        begin_index = n_seen                                # the out row alone is at it
        procs = [lp.SequenceBiasLogitsProcessor(dict(sequence_bias)), lp.RepetitionPenaltyLogitsProcessor(penalty),
                 lp.NoBadWordsLogitsProcessor(bad_words), lp.MinLengthLogitsProcessor(min_len, torch.tensor(eos, device="cuda"), device="cuda"),
                 lp.SuppressTokensLogitsProcessor(suppress, device="cuda"),
                 lp.SuppressTokensAtBeginLogitsProcessor([B1, S1], begin_index, device="cuda")]
        window_procs = [lp.SequenceBiasLogitsProcessor({k: v for k, v in sequence_bias.items() if len(k) == 1}), procs[1],
                        lp.NoBadWordsLogitsProcessor([w for w in bad_words if len(w) == 1]), procs[3], procs[4]]
        plain_procs = [procs[1], procs[3]]
        controls, rest = controls_from_processors(procs)
        assert rest == [] and isinstance(controls, GenControls) and len(controls.sequence_bias) == len(sequence_bias) + 1

        pos = [n_seen - 1] + [n_seen + i for i in range(n_inp)] + [n_seen + (k % gs) for k in range(n_slots * gs)]
        pos_d = torch.tensor(pos, dtype=torch.int32, device="cuda")
        seqs = [full] + [full + [full[0]] * (i + 1) for i in range(n_inp)]
        live = []
        for c in range(n_slots):
            for j in range(gs):
                seqs.append(full + guess[c, :j + 1].tolist())
                live.append(c < g)
        ref = _hf_rows(logits, seqs, lambda r: window_procs if 1 <= r <= n_inp else procs)
        ref_plain = _hf_rows(logits, seqs, lambda r: plain_procs)
        ref_am, plain_am = ref.argmax(dim=-1), ref_plain.argmax(dim=-1)
        assert int(plain_am[0]) == W2 and int(ref_am[0]) not in (W2, B1), "the out row's winners must be the banned tokens"
        assert int(plain_am[c0j1]) == T2 and int(ref_am[c0j1]) == B1, "T2 banned by the straddling entry, B1 free away from the begin index"

        prompt_d = torch.tensor(prompt, dtype=torch.int32, device="cuda")
        ops.gen_ctl_init(gen, V, penalty, min_len, eos, prompt_d)
        ops.gen_constraints_init(gen, cons, V, controls.ban, controls.begin_ban, controls.begin_index, controls.sequence_bias,
                                 controls.add_bias, prompt_d)
        ctl[cabi.CTL_G] = g
        for ch in chunks:                                   # what a post-step leaves, then the update of the captured step
            ctl[cabi.CTL_N_ACCEPT] = len(ch)
            ctl[cabi.CTL_HITS:cabi.CTL_HITS + len(ch)] = torch.tensor(ch, dtype=torch.int32)
            ops.gen_ctl_update(gen, ctl)
        want_tail = full[-15:]
        words = cons[:cabi.CONS_TAIL + 15].tolist()
        assert words[cabi.CONS_TAIL_N] == len(want_tail) and words[cabi.CONS_TAIL + 15 - len(want_tail):] == want_tail, (V, prompt, chunks, words)
        addr = gen[cabi.GEN_CONS:cabi.GEN_CONS + 2].tolist()
        assert (addr[0] & 0xffffffff) | ((addr[1] & 0xffffffff) << 32) == cons.data_ptr()

        def run():
            am = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
            ops.gen_argmax(logits, n_inp, gs, gen, ctl, guess_d, pos_d, None, am)
            rows_out = torch.full((1 + n_slots * gs, V), float("nan"), dtype=torch.float32, device="cuda")
            am2 = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
            ops.gen_argmax(logits, n_inp, gs, gen, ctl, guess_d, pos_d, None, am2, rows_out)
            torch.cuda.synchronize()
            return am.tolist(), am2.tolist(), rows_out

        def check(want, want_am, what):
            am, am2, rows_out = run()
            for r in range(rows):
                if r > n_inp and not live[r - 1 - n_inp]:
                    assert am[r] == 0 and am2[r] == 0, (what, r)
                    continue
                assert am[r] == int(want_am[r]) == am2[r], (what, r, am[r], am2[r], int(want_am[r]))
            assert torch.equal(_bits(rows_out[0]), _bits(want[0])), (what, (rows_out[0] != want[0]).nonzero().flatten().tolist()[:8])
            for k in range(g * gs):
                assert torch.equal(_bits(rows_out[1 + k]), _bits(want[1 + n_inp + k])), (what, k, (rows_out[1 + k] != want[1 + n_inp + k]).nonzero().flatten().tolist()[:8])
            assert bool(torch.isnan(rows_out[1 + g * gs:]).all()), (what, "a padded slot was written")

        what = (V, str(dtype), len(prompt), [len(ch) for ch in chunks])
        check(ref, ref_am, what + ("constrained",))
        # detached (lade_gen_ctl_init zeroes the attach words): the bits of the penalty / min-length kernels, with the seen set as it stands
        ops.gen_ctl_init(gen, V, penalty, min_len, eos, torch.tensor(full, dtype=torch.int32, device="cuda"))
        assert gen[cabi.GEN_CONS:cabi.GEN_CONS + 2].tolist() == [0, 0]
        check(ref_plain, plain_am, what + ("detached",))


# ---- (2) HF end to end ------------------------------------------------------------------------------------------------------

CHAIN = (torch.randperm(254, generator=torch.Generator().manual_seed(5)) + 2).tolist()      # the cycle the "cycle" model walks
PROMPTS = dict(hf=[1, 5, 9, 17, 33, 5, 9, 17, 44, 5, 9, 17, 33, 5], cycle=[1] + CHAIN[:6] + [CHAIN[20]] + CHAIN[:3])
PROMPTS["cycle_soft"] = PROMPTS["cycle"]


def _tiny(kind):
    """"hf": the fp32 Llama of tests/test_gpu_hf.py.  "cycle": the model of tests/test_gpu_generate_scores.py - the lm_head row of succ(t) is
    the embedding of t, succ one random cycle through the vocabulary, so the stream walks the cycle, the window's guesses converge onto
    it and steps accept candidate rows; a banned token throws the stream to another place of the cycle.  "cycle_soft": the same with the
    lm_head scaled by 0.07, so that a few tokens share the probability mass at temperature 0.7 (sampling)."""
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    common = dict(vocab_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=512,
                  rms_norm_eps=1e-6, tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=None)
    if kind == "hf":
        m = LlamaForCausalLM(LlamaConfig(hidden_size=128, intermediate_size=256, **common))
    else:
        m = LlamaForCausalLM(LlamaConfig(hidden_size=64, intermediate_size=128, head_dim=64, **common))
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.normal_(0, 0.05)
        if kind != "hf":
            emb = m.model.embed_tokens.weight
            emb.normal_(0, 1.0)
            succ = torch.arange(256)
            succ[torch.tensor(CHAIN)] = torch.tensor(CHAIN[1:] + CHAIN[:1])
            m.lm_head.weight[succ] = emb * (0.07 if kind == "cycle_soft" else 1.0)
    return m.float().cuda().eval()


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
    yield lade, monkeypatch
    GenerationMixin._sample = orig
    lade.decoding.FUNC_MAP.pop("_sample", None)
    lade.decoding.CONFIG_MAP.clear()


SETTINGS = ((5, 4, 5, {}), (7, 3, 7, dict(POOL_FROM_PROMPT=1)))
N_NEW = 32
_MODELS = {}


def _model(kind="hf"):
    """(model, its unconstrained plain-HF greedy continuation): built once per kind"""
    if kind not in _MODELS:
        m = _tiny(kind)
        m.test_prompt = PROMPTS[kind]
        _MODELS[kind] = (m, _plain(m, {}))
    return _MODELS[kind]


def _plain(m, kwargs, n_new=N_NEW):
    prompt = torch.tensor([m.test_prompt], device="cuda")
    return m.generate(prompt, attention_mask=torch.ones_like(prompt), do_sample=False, max_new_tokens=n_new, **kwargs)[0, prompt.shape[1]:].tolist()


def _lade_generate(lade, mp, m, kwargs, graph, n_new=N_NEW, **extra):
    prompt = torch.tensor([m.test_prompt], device="cuda")
    mp.setenv("USE_LADE", "1")
    mp.setenv("LADE_GRAPH", graph)
    random.seed(1)
    extra.setdefault("do_sample", False)
    try:
        return m.generate(prompt, attention_mask=torch.ones_like(prompt), max_new_tokens=n_new, **kwargs, **extra)
    finally:
        mp.delenv("USE_LADE", raising=False)


def _compare(lade, mp, m, base, kwargs):
    """plain HF under kwargs differs from the unconstrained stream, and USE_LADE=1 equals it in every setting; returns (tokens, stats)"""
    mp.delenv("USE_LADE", raising=False)
    want = _plain(m, kwargs)
    assert want != base, ("the constraints do not bite on plain HF", kwargs)
    lade.augment_all()
    stats = []
    try:
        for (W, N, G, extra) in SETTINGS:
            for graph in ("0", "1"):
                _drop_engine(m)
                lade.config_lade(LEVEL=N, WINDOW_SIZE=W, GUESS_SET_SIZE=G, DEBUG=1, **extra)
                out = _lade_generate(lade, mp, m, kwargs, graph)[0, len(m.test_prompt):].tolist()
                assert out == want, (kwargs, W, N, G, graph, out, want)
                gen, steps, _ = lade.decoding.CONFIG_MAP["log"][-1]
                stats.append((gen, steps))
    finally:
        _drop_engine(m)
    return want, stats


def _settings_from(m, base):
    """constraint settings that bite on a model whose unconstrained continuation is `base`"""
    PROMPT = m.test_prompt
    free = [t for t in range(2, 256) if t not in base and t not in PROMPT]
    return dict(
        bad_words_ids=dict(bad_words_ids=[[base[3], base[4]], [base[9], base[10], base[11]], [base[20]], [PROMPT[-1], base[0]]]),
        suppress_tokens=dict(suppress_tokens=[base[1], base[6], free[0]]),
        begin_suppress_tokens=dict(begin_suppress_tokens=[base[0], free[1]]),
        sequence_bias=dict(sequence_bias={(base[2],): -30.0, (base[5], base[6]): -30.0, (base[7], base[8], free[2]): 30.0, (free[3],): 0.5,
                                          (base[12], base[13], base[14], base[15]): NEG_INF}),
    )


@pytest.mark.parametrize("which", ["bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "sequence_bias", "all"])
def test_constrained_greedy_equals_plain_hf(which, lade_env):
    lade, mp = lade_env
    m, base = _model()
    settings = _settings_from(m, base)
    if which == "all":
        kwargs = dict(repetition_penalty=1.3)
        for kw in settings.values():
            kwargs.update(kw)
    else:
        kwargs = settings[which]
    out, _ = _compare(lade, mp, m, base, kwargs)
    for t in kwargs.get("suppress_tokens", []):
        assert t not in out
    if "begin_suppress_tokens" in kwargs:
        assert out[0] not in kwargs["begin_suppress_tokens"]


def test_constrained_greedy_on_a_cycle_walking_model_accepts_candidates(lade_env):
    """a model whose stream the window's guesses predict: steps accept candidate rows, so rows whose input_ids end in the candidate's own
    prefix decide emitted tokens under the constraints"""
    lade, mp = lade_env
    m, base = _model("cycle")
    assert len(set(base)) == len(base)
    kwargs = dict(repetition_penalty=1.05)
    for kw in _settings_from(m, base).values():
        kwargs.update(kw)
    _, stats = _compare(lade, mp, m, base, kwargs)
    assert any(steps < gen for gen, steps in stats), stats


def test_consecutive_calls_rewrite_the_block_in_place(lade_env):
    """one decoder, hipGraph steps: two constraint sets, the penalty alone (controls on, block detached), then nothing at all"""
    lade, mp = lade_env
    m, base = _model()
    settings = _settings_from(m, base)
    first = dict(repetition_penalty=1.3, **settings["bad_words_ids"], **settings["sequence_bias"])
    second = dict(repetition_penalty=1.3, **settings["suppress_tokens"], **settings["begin_suppress_tokens"])
    calls = (first, second, dict(repetition_penalty=1.3), {})
    mp.delenv("USE_LADE", raising=False)
    wants = [_plain(m, kw) for kw in calls]
    assert wants[3] == base and len({tuple(w) for w in wants}) == 4, "the four calls must differ on plain HF"
    lade.augment_all()
    _drop_engine(m)
    lade.config_lade(LEVEL=4, WINDOW_SIZE=5, GUESS_SET_SIZE=5, DEBUG=1)
    try:
        dec, keys = None, []
        for kw, want in zip(calls, wants):
            out = _lade_generate(lade, mp, m, kw, "1")[0, len(m.test_prompt):].tolist()
            assert out == want, (kw, out, want)
            dec = dec or m._lade_decoder
            assert m._lade_decoder is dec
            keys.append(dec._graph_key)
        assert keys[0] == keys[1] == keys[2] != keys[3], "constraint sets come and go without a re-capture; controls on / off re-captures"
    finally:
        _drop_engine(m)


def test_sampling_scores_carry_the_constraints(lade_env):
    """scores[i] = HF's processors (in generate()'s order) and warpers applied to logits[i] with the row's prefix: the same -inf pattern, the
    kept entries bit-equal (the comparison of tests/test_gpu_generate_scores.py: the warpers are evaluated on CPU tensors there, since
    torch's device kernels divide by the temperature through a reciprocal; the processors on the GPU, as in (1)); no banned id is ever
    emitted"""
    from transformers.generation import logits_process as lp
    lade, mp = lade_env
    m, base = _model("cycle_soft")
    PROMPT = m.test_prompt
    s = _settings_from(m, base)
    kwargs = dict(repetition_penalty=1.3, **s["bad_words_ids"], **s["suppress_tokens"], **s["begin_suppress_tokens"], **s["sequence_bias"])
    procs = [lp.SequenceBiasLogitsProcessor(dict(s["sequence_bias"]["sequence_bias"])), lp.RepetitionPenaltyLogitsProcessor(1.3),
             lp.NoBadWordsLogitsProcessor(s["bad_words_ids"]["bad_words_ids"]),
             lp.SuppressTokensLogitsProcessor(s["suppress_tokens"]["suppress_tokens"], device="cuda"),
             lp.SuppressTokensAtBeginLogitsProcessor(s["begin_suppress_tokens"]["begin_suppress_tokens"], len(PROMPT), device="cuda")]
    warpers = [lp.TemperatureLogitsWarper(0.7), lp.TopKLogitsWarper(20)]
    banned = set(s["suppress_tokens"]["suppress_tokens"]) | {w[0] for w in s["bad_words_ids"]["bad_words_ids"] if len(w) == 1}
    bad_seqs = [w for w in s["bad_words_ids"]["bad_words_ids"] if len(w) > 1]
    lade.augment_all()
    _drop_engine(m)
    lade.config_lade(LEVEL=4, WINDOW_SIZE=5, GUESS_SET_SIZE=5, POOL_FROM_PROMPT=1, DEBUG=1)
    n_new = 24
    try:
        for graph, seed in (("1", 0), ("0", 1)):
            torch.manual_seed(seed)
            out = _lade_generate(lade, mp, m, kwargs, graph, n_new, do_sample=True, temperature=0.7, top_k=20, return_dict_in_generate=True,
                                 output_scores=True, output_logits=True)
            seq = out.sequences[0].tolist()
            new = seq[len(PROMPT):]
            assert len(new) == n_new == len(out.scores) == len(out.logits)
            assert not banned & set(new) and new[0] not in s["begin_suppress_tokens"]["begin_suppress_tokens"], (graph, new)
            for w in bad_seqs:
                assert not any(seq[i:i + len(w)] == w for i in range(len(PROMPT) - len(w) + 1, len(seq))), (graph, w, new)
            for i, tok in enumerate(new):
                ids = out.sequences[:, :len(PROMPT) + i]
                want = out.logits[i].clone()
                for p in procs:                         # on the GPU, where the rows of (1) are held to them bit for bit
                    want = p(ids, want)
                want = want.cpu()
                for wp in warpers:                      # on CPU tensors, as tests/test_gpu_generate_scores.py holds the warp kernel to them
                    want = wp(None, want)
                got = out.scores[i].cpu()
                assert torch.equal(torch.isinf(got), torch.isinf(want)), (graph, i, (torch.isinf(got) != torch.isinf(want)).nonzero().tolist()[:4])
                keep = ~torch.isinf(want)
                assert torch.equal(got[keep], want[keep]), (graph, i)
                assert bool(torch.isfinite(got[0, tok])), (graph, i, tok)
    finally:
        _drop_engine(m)


def test_lookahead_parallel_refuses_constraints(lade_env):
    from lookaheaddecoding_amd import cabi
    lade, mp = lade_env
    m, base = _model()
    lade.augment_all()
    _drop_engine(m)
    lade.config_lade(LEVEL=4, WINDOW_SIZE=5, GUESS_SET_SIZE=5)
    lade.decoding.CONFIG_MAP["FORCE_LP"] = 1
    try:
        for kw in _settings_from(m, base).values():
            with pytest.raises(cabi.LadeHipError, match="suppress_tokens"):
                _lade_generate(lade, mp, m, kw, "1", 8)
    finally:
        _drop_engine(m)
