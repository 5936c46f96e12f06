"""CPU: the host side of the generation controls - HF's processor list split into what the device step applies and the rest, EOS
id sets, and argument validation of the new entry points (LADE_E_ARG before any launch)."""
import ctypes as C

import pytest
import torch


def _lp():
    from transformers.generation import logits_process as lp
    return lp


def test_penalty_and_min_length_processors_become_controls():
    from lookaheaddecoding_amd.decoding import GenControls
    from lookaheaddecoding_amd.hf import controls_from_processors
    lp = _lp()
    ctl, rest = controls_from_processors([lp.RepetitionPenaltyLogitsProcessor(1.05)])
    assert ctl == GenControls(1.05, 0, None) and rest == []
    ctl, rest = controls_from_processors([lp.MinLengthLogitsProcessor(20, 2)])                      # EOS as an int
    assert ctl == GenControls(1.0, 20, (2,)) and rest == []
    ctl, rest = controls_from_processors([lp.MinNewTokensLengthLogitsProcessor(7, 5, [2, 9])])       # EOS as a list
    assert ctl == GenControls(1.0, 12, (2, 9))
    ctl, rest = controls_from_processors([lp.MinLengthLogitsProcessor(3, torch.tensor([9, 2])),     # EOS as a tensor; the larger min wins
                                          lp.MinNewTokensLengthLogitsProcessor(7, 5, torch.tensor([9, 2]))])
    assert ctl == GenControls(1.0, 12, (9, 2))
    assert controls_from_processors([]) == (None, []) and controls_from_processors(None) == (None, [])
    ctl, rest = controls_from_processors([lp.RepetitionPenaltyLogitsProcessor(1.0)])                 # penalty 1: nothing to do
    assert ctl is None and rest == []


def test_processors_mixed_with_warpers_keep_the_warpers_in_order():
    from lookaheaddecoding_amd.hf import controls_from_processors
    lp = _lp()
    ws = [lp.TemperatureLogitsWarper(0.7), lp.TopKLogitsWarper(20), lp.TopPLogitsWarper(0.8)]
    ctl, rest = controls_from_processors([lp.RepetitionPenaltyLogitsProcessor(1.05), lp.MinNewTokensLengthLogitsProcessor(10, 4, [3, 4])] + ws)
    assert ctl.penalty == 1.05 and ctl.min_len == 14 and ctl.min_len_eos == (3, 4)
    assert rest == ws


def test_processor_after_a_warper_is_refused():
    from lookaheaddecoding_amd.hf import controls_from_processors
    lp = _lp()
    with pytest.raises(AssertionError, match="after a logits warper"):
        controls_from_processors([lp.TemperatureLogitsWarper(0.7), lp.RepetitionPenaltyLogitsProcessor(1.3)])


def test_unsupported_processors_stay_and_the_old_assertions_fire():
    from lookaheaddecoding_amd import hf
    lp = _lp()
    bad = lp.NoRepeatNGramLogitsProcessor(3)
    ctl, rest = hf.controls_from_processors([lp.RepetitionPenaltyLogitsProcessor(1.3), bad])
    assert ctl.penalty == 1.3 and rest == [bad]
    if "prompt_ignore_length" in lp.RepetitionPenaltyLogitsProcessor.__init__.__code__.co_varnames:
        opt = lp.RepetitionPenaltyLogitsProcessor(1.3, prompt_ignore_length=4)           # an option the device step does not implement
        assert hf.controls_from_processors([opt]) == (None, [opt])
    # greedy: the assertion of the plain path, before anything touches a model
    with pytest.raises(AssertionError, match="logits processors are not supported in greedy lookahead"):
        hf.jacobi_greedy_search_multilevel(object(), torch.tensor([[1, 2]]), logits_processor=[bad])
    # sampling (transformers >= 4.4x: processors and warpers arrive in one list)
    import os
    old = os.environ.get("USE_LADE")
    os.environ["USE_LADE"] = "1"
    try:
        class Cfg:
            return_dict_in_generate, do_sample = False, True
        with pytest.raises(AssertionError, match="please set top_k"):
            hf._sample_proxy(object(), torch.tensor([[1, 2]]), logits_processor=[lp.TemperatureLogitsWarper(0.7), bad], generation_config=Cfg())
    finally:
        if old is None:
            del os.environ["USE_LADE"]
        else:
            os.environ["USE_LADE"] = old


def test_eos_sets():
    from lookaheaddecoding_amd import cabi
    from lookaheaddecoding_amd.decoding import eos_set
    from lookaheaddecoding_amd.hf import _criteria_limits
    assert eos_set(None) == () and eos_set(5) == (5,) and eos_set(-1) == ()
    assert eos_set([128001, 128008, 128009, 128001]) == (128001, 128008, 128009)
    assert eos_set(torch.tensor([7, 3])) == (7, 3)
    with pytest.raises(cabi.LadeHipError):
        eos_set(list(range(9)))
    from transformers.generation.stopping_criteria import EosTokenCriteria, MaxLengthCriteria
    ml, eos = _criteria_limits([MaxLengthCriteria(40), EosTokenCriteria(torch.tensor([128001, 128008, 128009]))])
    assert ml == 40 and eos == (128001, 128008, 128009)
    assert _criteria_limits([MaxLengthCriteria(40)]) == (40, None)


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from lookaheaddecoding_amd import cabi
    if not os.path.exists(cabi.LIB_PATH):
        g.build()
    return cabi.load_library()


def test_new_entry_points_validate_arguments(lib):
    from lookaheaddecoding_amd import cabi
    fake = 1 << 20                # never dereferenced: every call below fails its checks on the host
    eos = (C.c_int32 * 9)(*range(9))
    # null pointers / bad sizes: LADE_E_ARG, no launch
    assert lib.lade_gen_ctl_init(None, 256, 1.3, 0, None, 0, None, 0, None) == -1
    assert b"lade_gen_ctl_init" in lib.lade_last_error_string()
    assert lib.lade_gen_ctl_init(fake, 256, 0.0, 0, None, 0, None, 0, None) == -1                    # penalty must be > 0
    assert lib.lade_gen_ctl_init(fake, 256, 1.3, -1, None, 0, None, 0, None) == -1                   # min_len >= 0
    assert lib.lade_gen_ctl_init(fake, 256, 1.3, 5, eos, 9, None, 0, None) == -1                     # at most 8 EOS ids
    assert lib.lade_gen_ctl_init(fake, 256, 1.3, 5, None, 2, None, 0, None) == -1                    # ids promised, none given
    neg = (C.c_int32 * 2)(3, -4)
    assert lib.lade_gen_ctl_init(fake, 256, 1.3, 5, neg, 2, None, 0, None) == -1
    assert b"negative" in lib.lade_last_error_string()
    assert lib.lade_gen_ctl_init(fake, cabi.GEN_MAX_VOCAB + 1, 1.3, 0, None, 0, None, 0, None) == -1
    assert lib.lade_gen_ctl_init(fake, 256, 1.3, 0, None, 0, None, 4, None) == -1                    # prompt length without tokens
    assert lib.lade_gen_ctl_update(None, fake, None) == -1 and b"lade_gen_ctl_update" in lib.lade_last_error_string()
    assert lib.lade_gen_ctl_update(fake, None, None) == -1
    for name in ("lade_gen_argmax", "lade_gen_rows"):
        fn = getattr(lib, name)
        tail = (fake, None) if name == "lade_gen_rows" else (None,)
        assert fn(None, 256, 1, 256, cabi.LADE_F32, 0, 3, fake, fake, None, fake, None, fake, *tail) == -1
        assert name.encode() in lib.lade_last_error_string()
        # 1 + 2 window rows + 5 candidate rows: not whole candidates of gs = 3
        assert fn(fake, 256, 8, 256, cabi.LADE_F32, 2, 3, fake, fake, fake, fake, None, fake, *tail) == -1
        # candidate rows without a guess buffer
        assert fn(fake, 256, 9, 256, cabi.LADE_F32, 2, 3, fake, fake, None, fake, None, fake, *tail) == -1
        assert fn(fake, 100, 1, 256, cabi.LADE_F32, 0, 3, fake, fake, None, fake, None, fake, *tail) == -1     # ld < V
        assert fn(fake, 256, 1, 256, 7, 0, 3, fake, fake, None, fake, None, fake, *tail) == -2                 # unknown dtype
    assert lib.lade_gen_rows(fake, 256, 1, 256, cabi.LADE_F32, 0, 3, fake, fake, None, fake, None, fake, None, None) == -1   # no rows_out
    # the multi-EOS post-step: the plain post-step's checks, plus the EOS set
    args = dict(ctl=fake, window=fake, wcap=8, pool_tok=fake, pool_cnt=fake, V=256, W=5, N=4, G=5, am=fake, n_inp=5, guess=fake, T=30,
                cand_rows=0, phase=2, pfp=0, tail=None)
    head = tuple(args.values())
    rest = (None, None, fake, None, None)
    assert lib.lade_greedy_post_step(*head, eos, 9, *rest) == -1
    assert b"lade_greedy_post_step:" in lib.lade_last_error_string() and b"n_eos" in lib.lade_last_error_string()
    assert lib.lade_greedy_post_step(*head, None, 2, *rest) == -1
    assert lib.lade_greedy_post_step(*head, neg, 2, *rest) == -1
    bad_head = head[:6] + (0,) + head[7:]                                                                    # W = 0
    assert lib.lade_greedy_post_step(*bad_head, eos, 2, *rest) == -1
    assert lib.lade_greedy_post_step(*bad_head, None, 0, *rest) == -1 and b"lade_greedy_post_step:" in lib.lade_last_error_string()
