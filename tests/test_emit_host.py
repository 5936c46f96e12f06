"""CPU: the host side of per-token scores / logits under lookahead (generate(return_dict_in_generate=True)).
(1) lade_emit_init / lade_emit_rows refuse bad arguments with LADE_E_ARG before any launch (dummy non-null pointers, no GPU).
(2) hf.output_request reads the flags from keywords and from generation_config; hf.generate_output turns a decode loop's result into HF's
    output object: tuple lengths, [1, V] shapes, None for the field that was not requested (plain CPU tensors stand in).
(3) lookahead parallelism refuses the request, naming return_dict_in_generate."""
import ctypes as C
import os
import types

import pytest
import torch

E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from lookaheaddecoding_amd import cabi
    if not os.path.exists(cabi.LIB_PATH):
        g.build()
    return cabi.load_library()


def test_emit_entry_points_refuse_bad_arguments_before_any_launch(lib):
    buf = (C.c_char * 256)()
    p = C.addressof(buf)                  # a non-null "device pointer": validation fails before anything could read it
    V, gs = 64, 4
    # lade_emit_init(desc, scores, logits, cap_rows, V, stream)
    assert lib.lade_emit_init(None, p, p, 8, V, None) == E_ARG and b"descriptor" in lib.lade_last_error_string()
    assert lib.lade_emit_init(p, p, p, 8, 0, None) == E_ARG
    assert lib.lade_emit_init(p, p, p, 8, -3, None) == E_ARG
    assert lib.lade_emit_init(p, None, None, 8, V, None) == E_ARG and b"both destinations" in lib.lade_last_error_string()
    assert lib.lade_emit_init(p, p, None, -1, V, None) == E_ARG
    # lade_emit_rows(desc, raw, raw_ld, raw_dtype, n_inp, gs, proc, proc_ld, ctl, idx, n_idx, V, stream)
    idx = (C.c_int32 * 8)(0, 1, 1, 1, 1, 1, 1, 1)
    ia = C.addressof(idx)
    assert lib.lade_emit_rows(None, p, V, 0, 5, gs, None, 0, p, None, 0, V, None) == E_ARG and b"descriptor" in lib.lade_last_error_string()
    assert lib.lade_emit_rows(p, None, V, 0, 5, gs, None, 0, p, None, 0, V, None) == E_ARG
    assert lib.lade_emit_rows(p, p, V, 0, 5, gs, None, 0, p, None, 0, 0, None) == E_ARG
    assert lib.lade_emit_rows(p, p, V, 0, 5, gs, None, 0, p, None, 0, -1, None) == E_ARG
    assert lib.lade_emit_rows(p, p, V, 0, 5, gs, None, 0, p, ia, gs + 2, V, None) == E_ARG and b"n_idx" in lib.lade_last_error_string()
    assert lib.lade_emit_rows(p, p, V, 0, 5, gs, None, 0, p, ia, 0, V, None) == E_ARG
    assert lib.lade_emit_rows(p, p, V - 1, 0, 5, gs, None, 0, p, None, 0, V, None) == E_ARG            # row stride below V
    assert lib.lade_emit_rows(p, p, V, 0, 5, gs, p, V - 1, p, None, 0, V, None) == E_ARG               # processed-row stride below V
    assert lib.lade_emit_rows(p, p, V, 0, 5, 0, None, 0, p, None, 0, V, None) == E_ARG                 # gs
    assert lib.lade_emit_rows(p, p, V, 0, -1, gs, None, 0, p, None, 0, V, None) == E_ARG               # n_inp
    assert lib.lade_emit_rows(p, p, V, 0, 5, gs, None, 0, None, None, 0, V, None) == E_ARG             # neither idx nor ctl
    bad = (C.c_int32 * 2)(0, 64)
    assert lib.lade_emit_rows(p, p, V, 0, 5, gs, None, 0, p, C.addressof(bad), 2, V, None) == E_ARG    # candidate beyond LADE_MAX_GUESS_SET
    assert lib.lade_emit_rows(p, p, V, 7, 5, gs, None, 0, p, None, 0, V, None) == -2                   # LADE_E_DTYPE


def test_emit_request_and_capacity():
    from lookaheaddecoding_amd import cabi
    from lookaheaddecoding_amd.decoding import emit_capacity, emit_request
    assert emit_request(None) is None and emit_request(()) is None
    assert emit_request("logits") == ("logits",)
    assert emit_request(["logits", "scores"]) == ("scores", "logits")
    with pytest.raises(cabi.LadeHipError, match="attentions"):
        emit_request(("scores", "attentions"))
    assert emit_capacity(30, 10, 4) == 24 and emit_capacity(5, 10, 4) == 4


def _cfg(**kw):
    base = dict(return_dict_in_generate=False, output_scores=False, output_logits=False, output_attentions=False, output_hidden_states=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_output_request_reads_keywords_and_generation_config():
    from lookaheaddecoding_amd import cabi
    from lookaheaddecoding_amd.hf import output_request
    assert output_request(_cfg()) is None
    assert output_request(_cfg(output_scores=True)) is None, "without return_dict_in_generate a plain tensor is returned, as before"
    assert output_request(_cfg(return_dict_in_generate=True)) == ()
    assert output_request(_cfg(return_dict_in_generate=True, output_scores=True)) == ("scores",)
    assert output_request(_cfg(return_dict_in_generate=True, output_logits=True, output_scores=True)) == ("scores", "logits")
    # the 4.36 call path: keywords, no generation_config; a keyword wins over the config
    assert output_request(None, return_dict_in_generate=True, output_scores=True) == ("scores",)
    assert output_request(None, return_dict_in_generate=True, output_logits=True) == ("logits",)
    assert output_request(None) is None and output_request(None, output_scores=True) is None
    assert output_request(_cfg(return_dict_in_generate=True, output_scores=True), return_dict_in_generate=False) is None
    for name in ("output_attentions", "output_hidden_states"):
        with pytest.raises(cabi.LadeHipError, match=name):
            output_request(_cfg(return_dict_in_generate=True, **{name: True}))
        with pytest.raises(cabi.LadeHipError, match=name):
            output_request(None, return_dict_in_generate=True, **{name: True})
        assert output_request(_cfg(**{name: True})) is None          # without return_dict_in_generate nothing would be returned: as before


def test_generate_output_builds_hf_tuples_from_a_result():
    from lookaheaddecoding_amd import cabi
    from lookaheaddecoding_amd.decoding import GenOut
    from lookaheaddecoding_amd.hf import generate_output
    n, V = 7, 33
    scores, logits = torch.randn(n, V), torch.randn(n, V)
    seq = torch.arange(3 + n).view(1, -1)
    res = GenOut(tokens=seq[0].tolist(), steps=4, generated=n, scores=scores, logits=logits)
    out = generate_output(seq, res, ("scores", "logits"))
    assert type(out).__name__ == "GenerateDecoderOnlyOutput" and out.sequences is seq and out.past_key_values is None
    assert isinstance(out.scores, tuple) and isinstance(out.logits, tuple) and len(out.scores) == len(out.logits) == n
    for i in range(n):
        assert out.scores[i].shape == (1, V) and out.scores[i].dtype == torch.float32 and torch.equal(out.scores[i][0], scores[i])
        assert out.logits[i].shape == (1, V) and torch.equal(out.logits[i][0], logits[i])
        assert out.scores[i].data_ptr() == scores[i].data_ptr(), "views of the result's buffer, not copies"
    only = generate_output(seq, GenOut(tokens=[], steps=4, generated=n, logits=logits), ("logits",))
    assert only.scores is None and len(only.logits) == n
    only = generate_output(seq, GenOut(tokens=[], steps=4, generated=n, scores=scores, logits=logits), ("scores",))
    assert only.logits is None and len(only.scores) == n
    none = generate_output(seq, GenOut(tokens=[], steps=4, generated=n), ())
    assert none.scores is None and none.logits is None and none.sequences is seq
    with pytest.raises(cabi.LadeHipError, match="scores"):            # rows and tokens must agree
        generate_output(seq, GenOut(tokens=[], steps=4, generated=n + 1, scores=scores), ("scores",))


def test_lookahead_parallelism_refuses_the_request():
    from lookaheaddecoding_amd import cabi, hf
    from lookaheaddecoding_amd.decoding import CONFIG_MAP, LP_EMIT_REFUSAL, LookaheadDecoder
    assert "return_dict_in_generate" in LP_EMIT_REFUSAL and "lade_lp_reduce_apply" in LP_EMIT_REFUSAL
    ids = torch.tensor([[1, 2, 3]])
    saved = dict(CONFIG_MAP)
    try:
        for conf in (dict(FORCE_LP=1), dict(DIST_WORKERS=2)):
            CONFIG_MAP.clear()
            CONFIG_MAP.update(conf)
            with pytest.raises(cabi.LadeHipError, match="return_dict_in_generate"):      # before the model or an engine is touched
                hf._run(None, ids, False, None, None, None, None, None, False, None, request=("scores",))
    finally:
        CONFIG_MAP.clear()
        CONFIG_MAP.update(saved)
    # and the decode loops themselves, for callers below the HF surface
    stub = types.SimpleNamespace(lp=types.SimpleNamespace(R=2, force=False))
    for method in (LookaheadDecoder.greedy, LookaheadDecoder.sample):
        raw = method.__wrapped__.__wrapped__
        with pytest.raises(cabi.LadeHipError, match="return_dict_in_generate"):
            raw(stub, [1, 2, 3], 8, emit=("logits",))
