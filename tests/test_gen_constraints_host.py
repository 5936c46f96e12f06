"""CPU: the host side of the token constraints (bad_words_ids, suppress_tokens, begin_suppress_tokens, sequence_bias) under lookahead.
hf.controls_from_processors on processor lists built from HF's own classes, GenControls' defaults and caps, and the argument checks of
lade_gen_constraints_init (they run before any launch: dummy pointers, no GPU)."""
import ctypes as C
import os

import pytest
import torch


def _lp():
    from transformers.generation import logits_process as lp
    return lp


def _split(processors):
    from lookaheaddecoding_amd.hf import controls_from_processors
    return controls_from_processors(processors)


NEG_INF = -float("inf")


def test_gen_controls_defaults_keep_the_three_argument_constructor():
    from lookaheaddecoding_amd.decoding import GenControls
    c = GenControls(1.0, 0, None)
    assert not c.active and not c.constrained
    assert (c.ban, c.begin_ban, c.begin_index, c.sequence_bias, c.add_bias) == ((), (), -1, (), False)
    assert GenControls(1.3, 0, None).active and not GenControls(1.3, 0, None).constrained
    for kw in (dict(ban=(3,)), dict(begin_ban=(3,), begin_index=4), dict(sequence_bias=(((1, 2), -1.0),)), dict(add_bias=True)):
        c = GenControls(**kw)
        assert c.active and c.constrained, kw


def test_each_of_the_four_classes_is_taken():
    lp = _lp()
    ctl, rest = _split([lp.SuppressTokensLogitsProcessor([5, 9])])
    assert rest == [] and ctl.ban == (5, 9) and not ctl.add_bias and ctl.sequence_bias == ()
    ctl, rest = _split([lp.SuppressTokensAtBeginLogitsProcessor([7, 8], 14)])
    assert rest == [] and ctl.begin_ban == (7, 8) and ctl.begin_index == 14 and ctl.ban == ()
    ctl, rest = _split([lp.NoBadWordsLogitsProcessor([[4, 5, 6], [11]])])
    assert rest == [] and ctl.ban == (11,) and ctl.sequence_bias == (((4, 5, 6), NEG_INF),) and ctl.add_bias
    ctl, rest = _split([lp.SequenceBiasLogitsProcessor([[[4, 5], 2.5], [[6], -1.0]])])
    assert rest == [] and ctl.sequence_bias == (((4, 5), 2.5), ((6,), -1.0)) and ctl.ban == () and ctl.add_bias


def test_dict_order_is_kept_and_single_token_bans_merge_with_suppress_tokens():
    lp = _lp()
    bias = {(9, 8, 7): -2.0, (3,): 1.5, (1, 2): 0.25, (4,): NEG_INF, (2, 2): NEG_INF, (6, 2): 4.0}
    procs = [lp.SequenceBiasLogitsProcessor(dict(bias)), lp.RepetitionPenaltyLogitsProcessor(1.2),
             lp.NoBadWordsLogitsProcessor([[30], [31, 32], [33]]), lp.MinLengthLogitsProcessor(20, 2),
             lp.SuppressTokensLogitsProcessor([40, 41]), lp.SuppressTokensAtBeginLogitsProcessor([50], 12)]
    ctl, rest = _split(procs)
    assert rest == []
    assert ctl.sequence_bias == (((9, 8, 7), -2.0), ((3,), 1.5), ((1, 2), 0.25), ((2, 2), NEG_INF), ((6, 2), 4.0), ((31, 32), NEG_INF))
    assert ctl.ban == (4, 30, 33, 40, 41)               # single-token -inf entries of both classes and suppress_tokens, in list order
    assert (ctl.begin_ban, ctl.begin_index) == ((50,), 12)
    assert (ctl.penalty, ctl.min_len, ctl.min_len_eos) == (1.2, 20, (2,))


def test_hf_eos_filtering_of_bad_words_is_honoured():
    lp = _lp()
    ctl, rest = _split([lp.NoBadWordsLogitsProcessor([[2], [7], [2, 7]], eos_token_id=2)])
    assert rest == [] and ctl.ban == (7,) and ctl.sequence_bias == (((2, 7), NEG_INF),)
    ctl, _ = _split([lp.NoBadWordsLogitsProcessor([[2], [7]], eos_token_id=[2, 7])])
    assert ctl.ban == () and ctl.sequence_bias == () and ctl.add_bias and ctl.active        # HF still runs `scores + bias` on every row


def test_order_rules():
    lp = _lp()
    rep = lp.RepetitionPenaltyLogitsProcessor(1.2)
    with pytest.raises(AssertionError, match="before the repetition penalty"):
        _split([rep, lp.SequenceBiasLogitsProcessor({(4, 5): 2.5})])
    # -inf absorbs the penalty: bans may sit behind it (where HF's generate() puts bad_words_ids and suppress_tokens)
    ctl, rest = _split([rep, lp.SequenceBiasLogitsProcessor({(4, 5): NEG_INF}), lp.NoBadWordsLogitsProcessor([[6, 7]])])
    assert rest == [] and ctl.sequence_bias == (((4, 5), NEG_INF), ((6, 7), NEG_INF))
    for taken in (lp.SuppressTokensLogitsProcessor([5]), lp.SuppressTokensAtBeginLogitsProcessor([5], 3), lp.NoBadWordsLogitsProcessor([[5, 6]]),
                  lp.SequenceBiasLogitsProcessor({(5, 6): 1.0})):
        with pytest.raises(AssertionError, match="after a logits warper"):
            _split([lp.TemperatureLogitsWarper(0.7), taken])
    # a second set of finite biases, or a second begin index, is left to the callers to refuse
    second = lp.SequenceBiasLogitsProcessor({(8, 9): 1.0})
    ctl, rest = _split([lp.SequenceBiasLogitsProcessor({(5, 6): 1.0}), second])
    assert rest == [second] and ctl.sequence_bias == (((5, 6), 1.0),)
    other = lp.SuppressTokensAtBeginLogitsProcessor([6], 4)
    ctl, rest = _split([lp.SuppressTokensAtBeginLogitsProcessor([5], 3), other])
    assert rest == [other] and ctl.begin_ban == (5,)


def test_bad_biases_and_caps_are_refused_with_a_message():
    from lookaheaddecoding_amd import cabi
    lp = _lp()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(cabi.LadeHipError, match="finite or -inf"):
            _split([lp.SequenceBiasLogitsProcessor({(4, 5): bad})])
    many = {(i // 200 + 1, i % 200 + 1, 3): -1.0 for i in range(cabi.GEN_MAX_SEQ + 1)}
    assert len(many) == 1025
    with pytest.raises(cabi.LadeHipError, match="LADE_GEN_MAX_SEQ"):
        _split([lp.SequenceBiasLogitsProcessor(many)])
    many.popitem()
    ctl, _ = _split([lp.SequenceBiasLogitsProcessor(many)])
    assert len(ctl.sequence_bias) == 1024
    with pytest.raises(cabi.LadeHipError, match="LADE_GEN_MAX_SEQ_LEN"):
        _split([lp.NoBadWordsLogitsProcessor([list(range(1, 18))])])
    ctl, _ = _split([lp.NoBadWordsLogitsProcessor([list(range(1, 17))])])
    assert len(ctl.sequence_bias[0][0]) == 16
    # single banned tokens are served by the bitmap: no cap
    ctl, _ = _split([lp.NoBadWordsLogitsProcessor([[t] for t in range(5000)]), lp.SuppressTokensLogitsProcessor(list(range(5000, 9000)))])
    assert len(ctl.ban) == 9000 and ctl.sequence_bias == ()


def test_no_repeat_ngram_and_unknown_processors_stay_in_remaining():
    lp = _lp()
    ngram = lp.NoRepeatNGramLogitsProcessor(3)
    ctl, rest = _split([lp.SuppressTokensLogitsProcessor([5]), ngram])
    assert rest == [ngram] and ctl.ban == (5,)
    ctl, rest = _split([ngram])
    assert ctl is None and rest == [ngram]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from lookaheaddecoding_amd import cabi
    if not os.path.exists(cabi.LIB_PATH):
        g.build()
    return cabi.load_library()


def test_constraints_init_validates_its_arguments_before_any_launch(lib):
    from lookaheaddecoding_amd import cabi
    assert cabi.gen_cons_words(32000) == cabi.CONS_BAN + 2 * 1000 and cabi.gen_words(32000) == 16 + 1000
    p = 1 << 20                                         # a dummy non-null pointer: never dereferenced by a refused call
    I32, F32 = C.c_int32, C.c_float

    def init(gen=p, cons=p, V=256, ban=None, begin=None, begin_index=-1, off=None, tok=None, bias=None, n_seq=0, prompt=None, n_prompt=0,
             n_ban=None, n_begin=None):
        ban_a = (I32 * max(len(ban or ()), 1))(*(ban or ()))
        begin_a = (I32 * max(len(begin or ()), 1))(*(begin or ()))
        off_a = (I32 * max(len(off or ()), 1))(*(off or ()))
        tok_a = (I32 * max(len(tok or ()), 1))(*(tok or ()))
        bias_a = (F32 * max(len(bias or ()), 1))(*(bias or ()))
        rc = lib.lade_gen_constraints_init(gen, cons, V, C.addressof(ban_a) if ban else None, len(ban or ()) if n_ban is None else n_ban,
                                           C.addressof(begin_a) if begin else None, len(begin or ()) if n_begin is None else n_begin,
                                           begin_index, C.addressof(off_a) if off else None, C.addressof(tok_a) if tok else None,
                                           C.addressof(bias_a) if bias else None, n_seq, 1, prompt, n_prompt, None)
        return rc, lib.lade_last_error_string()

    def refused(needle=b"", **kw):
        rc, msg = init(**kw)
        assert rc == -1 and b"lade_gen_constraints_init" in msg and needle in msg, (kw.keys(), rc, msg)

    refused(b"null", gen=None)
    refused(b"null", cons=None)
    refused(n_ban=3)                                    # a count without its array
    refused(n_begin=2)
    refused(begin=[4], begin_index=-1)
    refused(n_seq=1)
    refused(n_prompt=4)
    refused(b"LADE_GEN_CONS_MAX_VOCAB", V=cabi.GEN_CONS_MAX_VOCAB + 1)
    n = cabi.GEN_MAX_SEQ + 1
    refused(b"LADE_GEN_MAX_SEQ = 1024", off=list(range(n + 1)), tok=[1] * n, bias=[-1.0] * n, n_seq=n)
    refused(b"LADE_GEN_MAX_SEQ_LEN = 16", off=[0, 17], tok=list(range(17)), bias=[-1.0], n_seq=1)
    refused(b"outside the vocabulary", off=[0, 2], tok=[3, 256], bias=[-1.0], n_seq=1)
    refused(b"finite or -inf", off=[0, 2], tok=[3, 4], bias=[float("nan")], n_seq=1)
    refused(b"finite or -inf", off=[0, 2], tok=[3, 4], bias=[float("inf")], n_seq=1)
    refused(b"negative", ban=[3, -1])
