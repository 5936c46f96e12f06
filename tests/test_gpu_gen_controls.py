"""GPU: repetition penalty, the min-length family and EOS sets on the lookahead step.
(1) lade_gen_argmax / lade_gen_rows against HF's own processor classes applied row by row (on the GPU, as plain decoding applies them) to
    the input_ids each row has in plain decoding: fp32 / bf16 / f16 logits, V = 256 / 32000 / 152064, candidate prefixes with repeats,
    padded candidate slots, min_len on both sides of a row boundary, exact ties; the argmax and the fp32 rows bit-exact.
(2) fp32 greedy end to end: USE_LADE=1 model.generate() equals USE_LADE=0 token for token on tiny Llama and Qwen2 models, hipGraph on and
    off, two lookahead settings, with repetition_penalty, min_new_tokens and a list of EOS ids.
(3) sampling with Qwen2.5-Instruct's generation settings on a bf16 tiny Qwen2 model.
(4) lookahead parallelism refuses the controls and EOS sets it does not implement."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu


def _hf_rows(logits, seqs, penalty, min_len, eos):
    """HF's RepetitionPenaltyLogitsProcessor then MinLengthLogitsProcessor on fp32 scores, one row at a time with that row's input_ids"""
    from transformers.generation.logits_process import MinLengthLogitsProcessor, RepetitionPenaltyLogitsProcessor
    rep = RepetitionPenaltyLogitsProcessor(penalty)
    mlp = MinLengthLogitsProcessor(min_len, torch.tensor(eos, device="cuda"), device="cuda")
    out = []
    for r, ids in enumerate(seqs):
        scores = logits[r:r + 1].float()
        ids_t = torch.tensor([ids], dtype=torch.long, device="cuda")
        out.append(mlp(ids_t, rep(ids_t, scores)))
    return torch.cat(out)


@pytest.mark.parametrize("V", [256, 257, 32000, 32001, 152064])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_processed_argmax_and_rows_match_hf_processors(V, dtype):
    from lookaheaddecoding_amd import cabi, ops
    gen_t = torch.Generator().manual_seed(V)
    gs, n_inp, n_slots, g = 4, 6, 5, 3                      # 5 candidate slots, 3 live: slots 3 and 4 are padding
    rows = 1 + n_inp + n_slots * gs
    eos = [V - 1, 3]
    # quantised scores: many exact ties, before and after the penalty.  A vocabulary that is not a multiple of 8 also gets a row stride
    # ld = V + 5 (a column slice: rows off the 16-byte grid, the scalar loop) and misaligned fp32 output rows (V % 4 != 0)
    pad = 5 if V % 8 else 0
    logits = ((torch.randint(-8, 9, (rows, V + pad), generator=gen_t).float() * 0.5)).to(dtype).cuda()[:, :V]
    seen = torch.randint(0, 40, (30,), generator=gen_t).tolist() + [V - 1, 7, 7]          # repeats, an EOS id among them
    guess = torch.randint(0, 40, (n_slots, gs), generator=gen_t)
    guess[0, 2] = guess[0, 0]                               # a repeat inside a candidate
    guess[1, 1] = seen[3]                                   # a candidate token that is already in the seen set
    for c in range(n_slots):                               # make the penalised tokens and the EOS ids the ones that matter
        logits[1 + n_inp + c * gs:1 + n_inp + (c + 1) * gs, guess[c]] = 4.0
    logits[:, seen[:6]] = 4.0
    logits[:, eos] = 4.5
    guess_d = guess.flatten().to(torch.int32).cuda()
    ctl = torch.zeros(cabi.CTL_WORDS, dtype=torch.int32, device="cuda")
    ctl[cabi.CTL_G] = g
    n_seen = len(seen)
    lst_pos = n_seen - 1
    pos = [lst_pos] + [lst_pos + 1 + i for i in range(n_inp)] + [lst_pos + 1 + (k % gs) for k in range(n_slots * gs)]
    pos_d = torch.tensor(pos, dtype=torch.int32, device="cuda")
    # the same positions reached through a row selection that is not the identity (what a step's `sel` does)
    perm = torch.randperm(rows + 7, generator=gen_t)[:rows]
    pos_full = torch.zeros(rows + 7, dtype=torch.int32)
    pos_full[perm] = torch.tensor(pos, dtype=torch.int32)
    pos_full, sel = pos_full.cuda(), perm.to(torch.int32).cuda()
    gen = torch.zeros(cabi.gen_words(V), dtype=torch.int32, device="cuda")
    for penalty, min_len in ((1.05, 0), (1.3, n_seen + 2), (5.0, n_seen + 1), (0.7, 0)):
        ops.gen_ctl_init(gen, V, penalty, min_len, eos, torch.tensor(seen, dtype=torch.int32, device="cuda"))
        seqs = [seen] + [seen + [seen[0]] * (i + 1) for i in range(n_inp)]      # window rows: the seen set, their own length
        live = []
        for c in range(n_slots):
            for j in range(gs):
                seqs.append(seen + guess[c, :j + 1].tolist())
                live.append(c < g)
        ref = _hf_rows(logits, seqs, penalty, min_len if min_len else 0, eos)
        ref_am = ref.argmax(dim=-1).to(torch.int32)
        am = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
        ops.gen_argmax(logits, n_inp, gs, gen, ctl, guess_d, pos_d, None, am)
        rows_out = torch.full((1 + n_slots * gs, V), float("nan"), dtype=torch.float32, device="cuda")
        am2 = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
        ops.gen_argmax(logits, n_inp, gs, gen, ctl, guess_d, pos_full, sel, am2, rows_out)
        torch.cuda.synchronize()
        what = (V, str(dtype), penalty, min_len)
        for r in range(rows):
            is_pad = r > n_inp and not live[r - 1 - n_inp]
            if is_pad:
                assert int(am[r]) == 0 and int(am2[r]) == 0, what
                continue
            assert int(am[r]) == int(ref_am[r]) == int(am2[r]), (what, r, int(am[r]), int(ref_am[r]))
        assert torch.equal(rows_out[0], ref[0]), what
        for k in range(g * gs):
            assert torch.equal(rows_out[1 + k], ref[1 + n_inp + k]), (what, k)
        if min_len:                                         # the mask decided some rows: an EOS id wins without it
            assert int(ref_am[0]) not in eos
    # the seen set grows on the device from the post-step's accepted tokens
    ctl[cabi.CTL_N_ACCEPT] = 3
    ctl[cabi.CTL_HITS:cabi.CTL_HITS + 3] = torch.tensor([41, 42, V - 2], dtype=torch.int32)
    ops.gen_ctl_init(gen, V, 1.3, 0, eos, torch.tensor(seen, dtype=torch.int32, device="cuda"))
    ops.gen_ctl_update(gen, ctl)
    seen2 = seen + [41, 42, V - 2]
    bits = gen[cabi.GEN_SEEN:].cpu().numpy().view("uint32")
    got = {w * 32 + b for w in range(len(bits)) for b in range(32) if (int(bits[w]) >> b) & 1}
    assert got == set(seen2)


# ---- (2) HF end to end ------------------------------------------------------------------------------------------------------

def _tiny(family, copy_biased=False):
    torch.manual_seed(0)
    common = dict(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512, rms_norm_eps=1e-6,
                  pad_token_id=0, bos_token_id=1, eos_token_id=None, num_attention_heads=2, num_key_value_heads=1)
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
        if copy_biased:                     # large tied embeddings: the model copies its context, the stream repeats n-grams
            m.model.embed_tokens.weight.normal_(0, 1.0)
            m.lm_head.weight.copy_(m.model.embed_tokens.weight)
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


PROMPT = [1, 5, 9, 17, 33, 5, 9, 17, 44, 5, 9, 17, 33, 5]
SETTINGS = ((5, 4, 5, {}), (7, 3, 7, dict(POOL_FROM_PROMPT=1)))


def _compare(lade, mp, m, kwargs, n_new=48):
    """plain HF greedy vs USE_LADE=1 in every setting; returns (plain tokens, [(generated, steps)])"""
    prompt = torch.tensor([PROMPT], device="cuda")
    mask = torch.ones_like(prompt)
    mp.delenv("USE_LADE", raising=False)
    plain = m.generate(prompt, attention_mask=mask, do_sample=False, max_new_tokens=n_new, **kwargs)
    lade.augment_all()
    mp.setenv("USE_LADE", "1")
    stats = []
    try:
        for (W, N, G, extra) in SETTINGS:
            for graph in ("0", "1"):
                mp.setenv("LADE_GRAPH", graph)
                _drop_engine(m)
                lade.config_lade(LEVEL=N, WINDOW_SIZE=W, GUESS_SET_SIZE=G, DEBUG=1, **extra)
                random.seed(1)
                out = m.generate(prompt, attention_mask=mask, do_sample=False, max_new_tokens=n_new, **kwargs)
                assert torch.equal(out, plain), (kwargs, W, N, G, graph, out.tolist(), plain.tolist())
                gen, steps, _ = lade.decoding.CONFIG_MAP["log"][-1]
                stats.append((gen, steps))
    finally:
        mp.delenv("USE_LADE", raising=False)
        _drop_engine(m)
    return plain[0, len(PROMPT):].tolist(), stats


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_repetition_penalty_greedy_equals_plain_hf(family, lade_env):
    lade, mp = lade_env
    m = _tiny(family)
    base, _ = _compare(lade, mp, m, {})
    changed = False
    for p in (1.05, 1.3, 5.0):
        out, _ = _compare(lade, mp, m, dict(repetition_penalty=p))
        changed |= out != base
    assert changed, "the penalty never changed the stream: the test would not see a missing penalty"
    # a copy-biased model repeats n-grams: candidate rows are accepted under the penalty
    mc = _tiny(family, copy_biased=True)
    out, stats = _compare(lade, mp, mc, dict(repetition_penalty=1.05))
    assert any(steps < gen for gen, steps in stats), stats


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_min_new_tokens_and_eos_sets_greedy_equal_plain_hf(family, lade_env):
    lade, mp = lade_env
    m = _tiny(family)
    base, _ = _compare(lade, mp, m, {})
    k = next(i for i in range(2, len(base)) if base[i] not in base[:i])       # a token plain greedy emits early, first at index k
    eos = base[k]
    never = next(t for t in range(2, 256) if t not in base and t not in PROMPT)
    out, _ = _compare(lade, mp, m, dict(eos_token_id=eos))
    assert out == base[:k + 1]
    out, _ = _compare(lade, mp, m, dict(eos_token_id=[never, eos]))
    assert out == base[:k + 1], "the second EOS id of the list must stop the stream"
    out, _ = _compare(lade, mp, m, dict(eos_token_id=[never, eos], min_new_tokens=k + 6))
    assert len(out) >= k + 6 and eos not in out[:k + 5]
    out, _ = _compare(lade, mp, m, dict(eos_token_id=eos, min_length=len(PROMPT) + k + 3, repetition_penalty=1.3))
    assert eos not in out[:k + 2]


# ---- (3) sampling ------------------------------------------------------------------------------------------------------------

def test_sampling_with_qwen25_instruct_settings_bf16(lade_env):
    lade, mp = lade_env
    m = _tiny("qwen2").to(torch.bfloat16)
    prompt = torch.tensor([PROMPT], device="cuda")
    mask = torch.ones_like(prompt)
    lade.augment_all()
    mp.setenv("USE_LADE", "1")
    base = m.generate(prompt, attention_mask=mask, do_sample=False, max_new_tokens=40)[0, len(PROMPT):].tolist()
    eos_ids = [base[2], base[5]]
    min_new = 12
    for graph in ("0", "1"):
        mp.setenv("LADE_GRAPH", graph)
        _drop_engine(m)
        lade.config_lade(LEVEL=4, WINDOW_SIZE=5, GUESS_SET_SIZE=5, DEBUG=1)
        for seed in range(3):
            random.seed(seed)
            torch.manual_seed(seed)
            out = m.generate(prompt, attention_mask=mask, do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.05,
                             eos_token_id=eos_ids, min_new_tokens=min_new, max_new_tokens=64)[0, len(PROMPT):].tolist()
            assert len(out) >= min_new and not any(t in eos_ids for t in out[:min_new]), (graph, seed, out)
            hit = [i for i, t in enumerate(out) if t in eos_ids]
            assert not hit or hit[0] == len(out) - 1, (graph, seed, out)
    _drop_engine(m)


def _copy_biased_engine():
    from lookaheaddecoding_amd.engine import StepEngine
    from lookaheaddecoding_amd.weights import make_config, random_weights_numpy
    cfg = make_config("tiny-d64", max_pos=512)
    w = {k: torch.as_tensor(v) for k, v in random_weights_numpy(cfg, seed=1, std=0.05).items()}
    w["embed"] = w["embed"] * 20.0                          # copy-biased: candidates exist and are verified
    w["lm_head"] = w["embed"]
    return lambda: StepEngine(cfg, w, dtype=torch.float32, device="cuda:0", max_seq=512, max_T=128)


def _check_tables(make_engine, prompt, out, gs, controls, temp):
    """Every verifying step's whole live table against softmax(HF processors (+ nothing without controls) of the step's rows / temp).
    The rows are recomputed on a fresh engine from the step's own inputs (the same tokens prefilled, then the step's ids / positions /
    mask, padded candidate slots included).  table[0][c] = P(drafts[c][0] | out row); table[1 + c'*gs + j][c] = P(drafts[c][j + 1] | the
    row of candidate c' at position j), j < gs - 1 (sampling.resolve_drafts)."""
    from lookaheaddecoding_amd.ops import StepMask
    penalty = controls.penalty if controls is not None else 1.0
    min_len = controls.min_len if controls is not None else 0
    eos = list(controls.min_len_eos) if controls is not None else []
    eng2 = make_engine()
    checked, seq = 0, list(prompt)
    for t in out.trace:
        if t.get("table") and t["g"] > 0:
            g = t["g"]
            eng2.reset()
            eng2.prefill(seq[:-1], [len(seq) - 2])
            ids = torch.tensor(t["ids"], dtype=torch.int32, device="cuda")
            pos = torch.tensor(t["pos"], dtype=torch.int32, device="cuda")
            mask = StepMask.from_levels(1, t["level_sizes"], t["cand_rows"], gs, len(seq) - 1)
            T = mask.T
            rows = [0] + list(range(T - t["cand_rows"], T - t["cand_rows"] + g * gs))
            logits = eng2.forward(ids, pos, mask, torch.tensor(rows, dtype=torch.int32, device="cuda"), len(rows))
            drafts = torch.tensor(t["drafts"]).view(g, gs)
            seqs = [seq] + [seq + drafts[c, :j + 1].tolist() for c in range(g) for j in range(gs)]
            probs = torch.softmax(_hf_rows(logits, seqs, penalty, min_len, eos) / temp, dim=-1).cpu()
            table = torch.tensor(t["table"])
            want = torch.zeros(1 + g * gs, g)
            live = [0] + [1 + cp * gs + j for cp in range(g) for j in range(gs - 1)]
            for r in live:
                k = 0 if r == 0 else (r - 1) % gs + 1                    # the draft position this row judges
                want[r] = probs[r, drafts[:, k]]
            for r in live:
                assert torch.allclose(table[r, :g], want[r], rtol=1e-4, atol=1e-6), (checked, r, table[r, :g], want[r])
            checked += 1
        seq += t["accepted"]
    return checked


def test_sampling_probability_table_uses_processed_rows():
    """The draft-probability table of every verifying step, all of its live rows, equals softmax over HF's processors + temperature
    applied to that step's rows (fp32; within the softmax kernels' rounding: they take exp in their own order)."""
    from lookaheaddecoding_amd.decoding import GenControls, LookaheadDecoder
    from lookaheaddecoding_amd.sampling import Warper
    make = _copy_biased_engine()
    dec = LookaheadDecoder(make(), 5, 3, 3)
    prompt = [1, 5, 9, 17, 33, 5, 9, 17, 44, 5, 9, 17, 33, 5, 9]
    ctl = GenControls(penalty=1.3, min_len=len(prompt) + 4, min_len_eos=(9, 17))
    out = dec.sample(prompt, len(prompt) + 30, warp=Warper(0.7), eos_token_id=None, rng=random.Random(3), keep_trace=True, controls=ctl,
                     torch_gen=torch.Generator().manual_seed(3))
    assert _check_tables(make, prompt, out, dec.gs, ctl, 0.7) > 0


def test_sampling_graph_follows_controls_on_and_off():
    """One decoder, hipGraph steps, sampling with controls off, then on, then off again: the captured forward step must follow (its body
    returns the processed out / candidate rows with controls, every row's logits without), and every verifying step's table must equal
    the restatement of its own mode."""
    from lookaheaddecoding_amd.decoding import GenControls, LookaheadDecoder
    from lookaheaddecoding_amd.sampling import Warper
    make = _copy_biased_engine()
    dec = LookaheadDecoder(make(), 5, 3, 3, use_graph=True)
    prompt = [1, 5, 9, 17, 33, 5, 9, 17, 44, 5, 9, 17, 33, 5, 9]
    ctl = GenControls(penalty=1.3, min_len=len(prompt) + 4, min_len_eos=(9, 17))
    for i, controls in enumerate((None, ctl, None)):
        out = dec.sample(prompt, len(prompt) + 30, warp=Warper(0.7), eos_token_id=None, rng=random.Random(3 + i), keep_trace=True,
                         controls=controls, torch_gen=torch.Generator().manual_seed(3 + i))
        assert any(t["phase"] == 2 for t in out.trace)
        assert _check_tables(make, prompt, out, dec.gs, controls, 0.7) > 0, (i, controls)


# ---- (4) lookahead parallelism ------------------------------------------------------------------------------------------------

def test_lookahead_parallel_refuses_controls_and_eos_sets(lade_env):
    from lookaheaddecoding_amd import cabi
    lade, mp = lade_env
    m = _tiny("llama")
    prompt = torch.tensor([PROMPT], device="cuda")
    mask = torch.ones_like(prompt)
    lade.augment_all()
    mp.setenv("USE_LADE", "1")
    try:
        lade.config_lade(LEVEL=4, WINDOW_SIZE=5, GUESS_SET_SIZE=5)
        lade.decoding.CONFIG_MAP["FORCE_LP"] = 1
        with pytest.raises(cabi.LadeHipError, match="repetition_penalty"):
            m.generate(prompt, attention_mask=mask, do_sample=False, max_new_tokens=8, repetition_penalty=1.3)
        with pytest.raises(cabi.LadeHipError, match="one EOS id"):
            m.generate(prompt, attention_mask=mask, do_sample=False, max_new_tokens=8, eos_token_id=[3, 4])
    finally:
        _drop_engine(m)
