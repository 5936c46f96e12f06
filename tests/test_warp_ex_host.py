"""CPU: the host side of the four warper stages behind top-p (min_p, typical_p, epsilon_cutoff, eta_cutoff) - admission of HF's classes,
their mapping to the seven device parameters, the torch statement of the semantics, argument validation of lade_warp_rows_ex."""
import ctypes as C
import os

import pytest
import torch


def _lp():
    from transformers.generation import logits_process as lp
    return lp


def _hf_chain(t=0.7, k=20, p=0.9, min_p=0.05, typical_p=0.9, eps=3e-4, eta=2e-3):
    lp = _lp()
    return [lp.TemperatureLogitsWarper(t), lp.TopKLogitsWarper(k), lp.TopPLogitsWarper(p), lp.MinPLogitsWarper(min_p), lp.TypicalLogitsWarper(typical_p),
            lp.EpsilonLogitsWarper(eps), lp.EtaLogitsWarper(eta)]


def test_the_four_kinds_are_admitted_and_mapped():
    from lookaheaddecoding_amd import hf
    lp = _lp()
    ws = _hf_chain()
    hf._check_admitted(ws)
    f32 = lambda v: float(torch.tensor(v))                 # EtaLogitsWarper keeps its epsilon as an fp32 tensor
    assert hf._canonical_warper(ws) == (0.7, 20, 0.9, 0.05, 0.9, 3e-4, f32(2e-3))
    assert hf._canonical_warper([lp.TemperatureLogitsWarper(0.6), lp.MinPLogitsWarper(0.1), lp.EtaLogitsWarper(3e-4)]) == (0.6, 0, 1.0, 0.1, 1.0, 0.0, f32(3e-4))
    assert hf._canonical_warper([lp.TemperatureLogitsWarper(0.7), lp.TopKLogitsWarper(20)]) == (0.7, 20, 1.0, 0.0, 1.0, 0.0, 0.0)
    # the device step's processors are still split off in front of them, and a processor behind any of the seven kinds is refused
    ctl, rest = hf.controls_from_processors([lp.RepetitionPenaltyLogitsProcessor(1.05)] + ws)
    assert ctl.penalty == 1.05 and rest == ws
    with pytest.raises(AssertionError, match="after a logits warper"):
        hf.controls_from_processors([lp.MinPLogitsWarper(0.1), lp.RepetitionPenaltyLogitsProcessor(1.3)])


def test_min_p_zero_of_the_qwen3_model_card_is_a_no_op():
    from lookaheaddecoding_amd import hf
    from lookaheaddecoding_amd.sampling import Warper
    lp = _lp()
    par = hf._canonical_warper([lp.TemperatureLogitsWarper(0.6), lp.TopKLogitsWarper(20), lp.TopPLogitsWarper(0.95), lp.MinPLogitsWarper(0.0)])
    assert par == (0.6, 20, 0.95, 0.0, 1.0, 0.0, 0.0)
    w = Warper(*par[:3], min_p=par[3], typical_p=par[4], epsilon_cutoff=par[5], eta_cutoff=par[6])
    assert not w.later_stages
    x = torch.randn(3, 500, generator=torch.Generator().manual_seed(0)) * 3
    assert torch.equal(w(x), Warper(0.6, 20, 0.95)(x))


def test_other_orders_and_options_fall_back_to_the_hf_objects():
    from lookaheaddecoding_amd import hf
    lp = _lp()
    assert hf._canonical_warper([lp.MinPLogitsWarper(0.1), lp.TopPLogitsWarper(0.9)]) is None                      # not HF's order
    assert hf._canonical_warper([lp.MinPLogitsWarper(0.1), lp.MinPLogitsWarper(0.2)]) is None                      # a kind twice
    assert hf._canonical_warper([lp.MinPLogitsWarper(0.1, min_tokens_to_keep=2)]) is None
    assert hf._canonical_warper([lp.TypicalLogitsWarper(0.9, min_tokens_to_keep=3)]) is None
    assert hf._canonical_warper([lp.EpsilonLogitsWarper(3e-4, filter_value=-1e9)]) is None
    assert hf._canonical_warper([lp.EtaLogitsWarper(3e-4, min_tokens_to_keep=2)]) is None
    hf._check_admitted([lp.MinPLogitsWarper(0.1, min_tokens_to_keep=2)])                                           # admitted all the same


def test_top_h_and_other_processors_are_still_refused(monkeypatch):
    from lookaheaddecoding_amd import hf
    lp = _lp()

    class Cfg:
        return_dict_in_generate, do_sample = False, True

    monkeypatch.setenv("USE_LADE", "1")
    for bad in (lp.TopHLogitsWarper(0.4), lp.NoRepeatNGramLogitsProcessor(3)):
        with pytest.raises(AssertionError, match="please set top_k"):
            hf._sample_proxy(object(), torch.tensor([[1, 2]]), logits_processor=[lp.TemperatureLogitsWarper(0.7), lp.MinPLogitsWarper(0.1), bad],
                             generation_config=Cfg())
        with pytest.raises(AssertionError, match="please set top_k"):
            hf.jacobi_sample_multilevel(object(), torch.tensor([[1, 2]]), logits_warper=[bad])
    with pytest.raises(AssertionError, match="logits processors are not supported in greedy lookahead"):
        hf.jacobi_greedy_search_multilevel(object(), torch.tensor([[1, 2]]), logits_processor=[lp.NoRepeatNGramLogitsProcessor(3)])


@pytest.mark.parametrize("scale", [3.0, 0.3])
def test_warper_call_is_hf_s_chain_on_cpu_rows(scale):
    from lookaheaddecoding_amd.sampling import Warper, make_warper
    x = torch.randn(4, 2000, generator=torch.Generator().manual_seed(1)) * scale
    x[1, ::3] = -float("inf")
    cases = [dict(min_p=0.05), dict(typical_p=0.9), dict(typical_p=0.2), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=2e-3), dict(eta_cutoff=0.5),
             dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)]
    lp = _lp()
    make = dict(min_p=lp.MinPLogitsWarper, typical_p=lp.TypicalLogitsWarper, epsilon_cutoff=lp.EpsilonLogitsWarper, eta_cutoff=lp.EtaLogitsWarper)
    for t, k, p in ((1.0, 0, 1.0), (0.7, 20, 0.9)):
        for case in cases:
            want = x
            for wp in [lp.TemperatureLogitsWarper(t), lp.TopKLogitsWarper(k or 2000), lp.TopPLogitsWarper(p)] + [make[s](v) for s, v in case.items()]:
                want = wp(None, want)
            got = make_warper(t, k, p, **case)(x)
            assert torch.equal(got, want), (t, k, p, case)
            assert torch.equal(Warper(t, k, p, **case)(x), want)


def test_fused_temperature_only_without_any_filter():
    from lookaheaddecoding_amd.sampling import Warper
    assert Warper(0.7).fused_temperature == 0.7 and Warper(0.7, 0, 1.0).fused_temperature == 0.7
    assert Warper(0.7, min_p=0.0).fused_temperature == 0.7                     # config 3's fused path with min_p=0 in the generation config
    assert Warper(0.7, 20).fused_temperature is None and Warper(0.7, 0, 0.9).fused_temperature is None
    for later in (dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=3e-4)):
        assert Warper(0.7, **later).fused_temperature is None, later
    w = Warper(0.7, 20, 0.9)
    assert (w.temperature, w.top_k, w.top_p, w.min_p, w.typical_p, w.epsilon_cutoff, w.eta_cutoff) == (0.7, 20, 0.9, 0.0, 1.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from lookaheaddecoding_amd import cabi
    if not os.path.exists(cabi.LIB_PATH):
        g.build()
    return cabi.load_library()


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """dummy non-null pointers, no GPU: every call must come back with LADE_E_ARG from the host-side check"""
    from lookaheaddecoding_amd.cabi import WarpParams
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    ok = dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    nan = float("nan")
    bad = [dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=nan), dict(typical_p=0.0), dict(typical_p=1.2), dict(typical_p=nan),
           dict(epsilon_cutoff=-1e-3), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=nan), dict(eta_cutoff=-1e-3), dict(eta_cutoff=1.0),
           dict(eta_cutoff=nan), dict(temperature=0.0), dict(top_k=-1), dict(top_p=0.0)]
    for b in bad:
        par = WarpParams(**dict(ok, **b))
        rc = lib.lade_warp_rows_ex(p, 8, 1, 8, 2, C.byref(par), 0, p, None)
        assert rc == -1 and b"lade_warp_rows_ex" in lib.lade_last_error_string(), (b, rc)
    rc = lib.lade_warp_rows_ex(p, 8, 1, 8, 2, None, 0, p, None)
    assert rc == -1 and b"null params" in lib.lade_last_error_string()
    par = WarpParams(**ok)
    assert lib.lade_warp_rows_ex(None, 8, 1, 8, 2, C.byref(par), 0, p, None) == -1
    assert lib.lade_warp_rows_ex(p, 8, 0, 8, 2, C.byref(par), 0, p, None) == 0          # no rows: nothing to launch
    assert C.sizeof(WarpParams) == 28
