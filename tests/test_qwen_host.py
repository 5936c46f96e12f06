"""CPU: the Qwen2 / Qwen3 surface - config_from_hf / weights_from_hf on tiny HF models built from a config, the refusals, the presets and
their random streams, and the argument checks of the two qkv-epilogue entry points (no launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

SMALL = dict(vocab_size=64, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
             max_position_embeddings=256)


def _qwen2(**kw):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    return Qwen2ForCausalLM(Qwen2Config(**{**SMALL, **kw}))


def _qwen3(**kw):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    args = {**SMALL, "head_dim": 32, **kw}           # H * d = 64 != hidden = 32
    return Qwen3ForCausalLM(Qwen3Config(**args))


def test_config_and_weights_from_qwen2():
    from lookaheaddecoding_amd import hf
    m = _qwen2(rope_theta=1000000.0, tie_word_embeddings=True)
    c = hf.config_from_hf(m)
    assert c["qkv_bias"] is True and "qk_norm" not in c and c["tied"] is True
    assert (c["hidden"], c["heads"], c["kv_heads"], c["head_dim"]) == (32, 2, 1, 16)
    assert c["rope_theta"] == 1000000.0 and c["rope_scaling"] is None
    w = hf.weights_from_hf(m)
    for i, layer in enumerate(m.model.layers):
        a = layer.self_attn
        for key, proj in (("bq", a.q_proj), ("bk", a.k_proj), ("bv", a.v_proj)):
            t = w[f"layers.{i}.{key}"]
            assert t.data_ptr() == proj.bias.data_ptr() and t.shape == proj.bias.shape         # a reference, not a copy
        assert f"layers.{i}.qn" not in w
    assert w["lm_head"].data_ptr() == w["embed"].data_ptr()


def test_config_and_weights_from_qwen3():
    from lookaheaddecoding_amd import hf
    m = _qwen3(tie_word_embeddings=False)
    c = hf.config_from_hf(m)
    assert c["qk_norm"] is True and "qkv_bias" not in c and c["tied"] is False
    assert c["head_dim"] == 32 and c["heads"] * c["head_dim"] != c["hidden"]
    w = hf.weights_from_hf(m)
    for i, layer in enumerate(m.model.layers):
        a = layer.self_attn
        assert w[f"layers.{i}.qn"].data_ptr() == a.q_norm.weight.data_ptr() and w[f"layers.{i}.qn"].shape == (32,)
        assert w[f"layers.{i}.kn"].data_ptr() == a.k_norm.weight.data_ptr()
        assert w[f"layers.{i}.wq"].shape == (64, 32) and w[f"layers.{i}.wo"].shape == (32, 64)
        assert f"layers.{i}.bq" not in w


def test_llama_config_is_unchanged():
    from transformers import LlamaConfig, LlamaForCausalLM
    from lookaheaddecoding_amd import hf
    c = hf.config_from_hf(LlamaForCausalLM(LlamaConfig(**SMALL)))
    assert "qkv_bias" not in c and "qk_norm" not in c and "tied" not in c


@pytest.mark.parametrize("make,kw,why", [
    (_qwen2, dict(use_sliding_window=True, sliding_window=64, max_window_layers=1), "sliding"),
    (_qwen3, dict(layer_types=["full_attention", "sliding_attention"], sliding_window=64), "sliding"),
    (_qwen3, dict(attention_bias=True), "o_proj"),
    (_qwen2, dict(rope_parameters={"rope_type": "yarn", "rope_theta": 10000.0, "factor": 2.0, "original_max_position_embeddings": 128}), "yarn"),
    (_qwen3, dict(rope_parameters={"rope_type": "yarn", "rope_theta": 10000.0, "factor": 2.0, "original_max_position_embeddings": 128}), "yarn"),
])
def test_qwen_refusals_name_the_reason(make, kw, why):
    from lookaheaddecoding_amd import cabi, hf
    m = make(**kw)
    with pytest.raises(cabi.LadeHipError, match=why):
        hf.config_from_hf(m)


def test_qwen_mlp_bias_refused():
    from lookaheaddecoding_amd import cabi, hf
    m = _qwen3()
    m.config.mlp_bias = True            # (no Qwen config takes it, but a checkpoint's config may carry it)
    with pytest.raises(cabi.LadeHipError, match="mlp_bias"):
        hf.config_from_hf(m)


def test_qwen_o_proj_bias_refused_by_weights():
    from lookaheaddecoding_amd import cabi, hf
    m = _qwen2()
    m.model.layers[0].self_attn.o_proj.bias = torch.nn.Parameter(torch.zeros(32))
    with pytest.raises(cabi.LadeHipError, match="bias"):
        hf.weights_from_hf(m)


def test_qwen_presets():
    from lookaheaddecoding_amd.weights import make_config, random_weights_numpy, weight_shapes
    q7 = make_config("qwen2.5-7b")
    assert (q7["hidden"], q7["inter"], q7["layers"], q7["heads"], q7["kv_heads"], q7["head_dim"], q7["vocab"]) == (3584, 18944, 28, 28, 4, 128, 152064)
    assert q7["qkv_bias"] and not q7.get("qk_norm")
    q8 = make_config("qwen3-8b")
    assert (q8["hidden"], q8["inter"], q8["layers"], q8["heads"], q8["kv_heads"], q8["head_dim"], q8["vocab"]) == (4096, 12288, 36, 32, 8, 128, 151936)
    assert q8["qk_norm"] and not q8.get("qkv_bias")
    q05 = make_config("qwen2.5-0.5b")
    assert (q05["hidden"], q05["heads"] // q05["kv_heads"], q05["head_dim"], q05["tied"], q05["qkv_bias"]) == (896, 7, 64, True, True)
    t3 = make_config("tiny-qwen3")
    assert t3["heads"] * t3["head_dim"] != t3["hidden"]
    s3 = weight_shapes(t3)
    assert s3["layers.0.qn"] == (64,) and s3["layers.0.wo"] == (128, 256) and "layers.0.bq" not in s3
    s2 = weight_shapes(make_config("tiny-qwen2"))
    assert s2["layers.1.bq"] == (6 * 64,) and s2["layers.1.bk"] == (64,) and s2["layers.1.bv"] == (64,)
    w2 = random_weights_numpy(make_config("tiny-qwen2"), seed=3)
    assert abs(float(w2["layers.0.bq"].std()) - 0.5) < 0.1
    w3 = random_weights_numpy(t3, seed=3)
    assert abs(float(w3["layers.0.qn"].mean()) - 1.0) < 0.1 and float(w3["layers.0.qn"].std()) > 0.1
    wt = random_weights_numpy(make_config("qwen2.5-0.5b", layers=1), seed=0)
    assert np.array_equal(wt["lm_head"], wt["embed"])


def test_existing_preset_random_stream_unchanged():
    """a Llama preset draws exactly the keys and values it drew before the Qwen keys existed (an inline restatement of the generator)"""
    from lookaheaddecoding_amd.weights import make_config, random_weights_numpy
    cfg = make_config("tiny-d64")
    w = random_weights_numpy(cfg, seed=1, std=0.05)
    rs = np.random.RandomState(1)
    hid, inter, H, Hkv, d, V = 128, 256, 2, 1, 64, 256
    keys = [("embed", (V, hid)), ("norm", (hid,)), ("lm_head", (V, hid))]
    for i in range(2):
        p = f"layers.{i}."
        keys += [(p + "ln1", (hid,)), (p + "ln2", (hid,)), (p + "wq", (H * d, hid)), (p + "wk", (Hkv * d, hid)), (p + "wv", (Hkv * d, hid)),
                 (p + "wo", (hid, H * d)), (p + "wg", (inter, hid)), (p + "wu", (inter, hid)), (p + "wd", (hid, inter))]
    assert list(w) == [k for k, _ in keys]
    for k, shp in keys:
        ref = np.ones(shp, dtype=np.float32) if len(shp) == 1 else (rs.standard_normal(shp) * 0.05).astype(np.float32)
        assert np.array_equal(w[k], ref), k


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from lookaheaddecoding_amd import cabi
    if not os.path.exists(cabi.LIB_PATH):
        g.build()
    return cabi.load_library()


def test_ex_entry_points_validate_arguments(lib):
    from lookaheaddecoding_amd import cabi
    epi = cabi.QkvEpilogue(None, None, None, 1e-6)
    # null pointers: LADE_E_ARG, no launch
    rc = lib.lade_rope_kv_append(None, None, 0, 0, None, None, None, None, None, None, 4, 0, None, 2, 1, 64, 64, 64, cabi.LADE_BF16, C.byref(epi), None)
    assert rc == -1 and b"lade_rope_kv_append" in lib.lade_last_error_string()
    rc = lib.lade_rope_kv_append(None, None, 2, 0, None, None, None, None, None, None, 4, 0, None, 2, 1, 64, 64, 64, cabi.LADE_BF16, None, None)
    assert rc == -1 and b"lade_rope_kv_append" in lib.lade_last_error_string()
    fake = 1 << 20            # never dereferenced: every call below fails its checks on the host
    for qkv, parts in ((fake, None), (None, fake)):                   # a source, but none of the other pointers / no q_out for the partials
        rc = lib.lade_rope_kv_append(qkv, parts, 2, 0, None, None, None, None, None, None, 4, 0, None, 2, 1, 64, 64, 64, cabi.LADE_BF16, None, None)
        assert rc == -1 and b"lade_rope_kv_append: null pointer" in lib.lade_last_error_string()
    rc = lib.lade_rope_kv_append(None, fake, 0, 4096, fake, fake, fake, fake, fake, fake, 4, 0, None, 2, 1, 64, 64, 64, cabi.LADE_BF16, None, None)
    assert rc == -1 and b"n_parts" in lib.lade_last_error_string()     # the partials need n_parts >= 1
    # bad shapes / a misaligned epilogue pointer / a head norm the partials path cannot reduce: LADE_E_ARG before any launch
    rc = lib.lade_rope_kv_append(fake, None, 0, 0, None, fake, fake, fake, fake, fake, 4, 62, None, 2, 1, 64, 64, 64, cabi.LADE_BF16, C.byref(epi), None)
    assert rc == -1                                                   # P + T > S_max
    bad = cabi.QkvEpilogue(fake + 2, None, None, 1e-6)
    rc = lib.lade_rope_kv_append(fake, None, 0, 0, None, fake, fake, fake, fake, fake, 4, 0, None, 2, 1, 64, 64, 64, cabi.LADE_BF16, C.byref(bad), None)
    assert rc == -1 and b"aligned" in lib.lade_last_error_string()
    neg = cabi.QkvEpilogue(None, fake, None, -1.0)
    rc = lib.lade_rope_kv_append(fake, None, 0, 0, None, fake, fake, fake, fake, fake, 4, 0, None, 2, 1, 64, 64, 64, cabi.LADE_BF16, C.byref(neg), None)
    assert rc == -1 and b"eps" in lib.lade_last_error_string()
    nrm = cabi.QkvEpilogue(None, fake, fake, 1e-6)
    rc = lib.lade_rope_kv_append(None, fake, 2, 4096, fake, fake, fake, fake, fake, fake, 4, 0, None, 2, 1, 96, 64, 64, cabi.LADE_BF16,
                                 C.byref(nrm), None)
    assert rc == -1 and b"power of two" in lib.lade_last_error_string()
    rc = lib.lade_rope_kv_append(None, fake, 2, 4096, fake, fake, fake, fake, fake, fake, 4, 0, None, 2, 1, 64, 64, 64, cabi.LADE_F32,
                                 C.byref(nrm), None)
    assert rc == -2                                                   # the partials path is 16-bit only
    # ... and so are the per-path shape rules: d = 12 (d/2 no multiple of 8) passes the checks of the materialised path only
    rc = lib.lade_rope_kv_append(None, fake, 2, 4096, fake, fake, fake, fake, fake, fake, 4, 0, None, 2, 1, 12, 64, 64, cabi.LADE_BF16, None, None)
    assert rc == -1 and b"d=12" in lib.lade_last_error_string()
    rc = lib.lade_rope_kv_append(fake, None, 0, 0, None, fake, fake, fake, fake, fake, 4, 0, None, 2, 1, 7, 64, 64, cabi.LADE_BF16, None, None)
    assert rc == -1 and b"d=7" in lib.lade_last_error_string()         # the materialised path needs an even d
    rc = lib.lade_rope_kv_append(fake, None, 0, 0, None, fake, fake, fake, fake, fake, 4, 0, None, 2, 1, 64, 64, 64, 7, None, None)
    assert rc == -2                                                   # unknown dtype
