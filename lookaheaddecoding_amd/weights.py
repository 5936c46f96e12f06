"""Synthetic Llama-shaped weights (no hub, no tokenizer) and the shape presets of BASELINE.json.

The reference loads real checkpoints through HF (`lade/utils.py:89-101`); there is no network
here, so every test / bench builds random-weight models of the named architecture.  Weights are
plain tensors in nn.Linear layout ([out_features, in_features]) keyed

    embed [V,hid]  norm [hid]  lm_head [V,hid]
    layers.{i}.ln1 / ln2 [hid]   layers.{i}.wq [H*d,hid]  wk, wv [Hkv*d,hid]  wo [hid,H*d]
    layers.{i}.wg, wu [inter,hid]   layers.{i}.wd [hid,inter]

plus, only where the config sets the flag,

    qkv_bias (Qwen2):  layers.{i}.bq [H*d]  bk, bv [Hkv*d]
    qk_norm (Qwen3):   layers.{i}.qn, kn [d]        (per-head RMSNorm weights of q and k)

which is what both `StepEngine` (HIP) and the CPU oracle consume.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

# shapes: SURVEY.md section 8 (C1..C5) + tiny shapes for parity tests
PRESETS: Dict[str, dict] = {
    # TinyLlama-1.1B shape (BASELINE config 1)
    "tinyllama-1.1b": dict(hidden=2048, inter=5632, layers=22, heads=32, kv_heads=4, head_dim=64, vocab=32000),
    # Llama-2-7B shape (BASELINE configs 2/3)
    "llama2-7b": dict(hidden=4096, inter=11008, layers=32, heads=32, kv_heads=32, head_dim=128, vocab=32000),
    # CodeLlama-13B shape (BASELINE config 4)
    "codellama-13b": dict(hidden=5120, inter=13824, layers=40, heads=40, kv_heads=40, head_dim=128, vocab=32016),
    # Llama-2-70B shape (BASELINE config 5)
    "llama2-70b": dict(hidden=8192, inter=28672, layers=80, heads=64, kv_heads=8, head_dim=128, vocab=32000),
    # parity-test shapes
    "tiny-d64": dict(hidden=128, inter=256, layers=2, heads=2, kv_heads=1, head_dim=64, vocab=256),
    "tiny-d128": dict(hidden=256, inter=384, layers=2, heads=2, kv_heads=2, head_dim=128, vocab=320),
    "tiny-d16": dict(hidden=64, inter=176, layers=2, heads=4, kv_heads=2, head_dim=16, vocab=128),
    # Qwen2.5-7B / Qwen3-8B / Qwen2.5-0.5B shapes (qkv bias; per-head q / k norm; d = 64 with 7 q heads per KV head, tied embeddings)
    "qwen2.5-7b": dict(hidden=3584, inter=18944, layers=28, heads=28, kv_heads=4, head_dim=128, vocab=152064, qkv_bias=True,
                       rope_theta=1000000.0, eps=1e-6),
    "qwen3-8b": dict(hidden=4096, inter=12288, layers=36, heads=32, kv_heads=8, head_dim=128, vocab=151936, qk_norm=True,
                     rope_theta=1000000.0, eps=1e-6),
    "qwen2.5-0.5b": dict(hidden=896, inter=4864, layers=24, heads=14, kv_heads=2, head_dim=64, vocab=151936, qkv_bias=True, tied=True,
                         rope_theta=1000000.0, eps=1e-6),
    # Qwen-style parity shapes: q / k / v bias at d = 64; head norm with H * d (256) != hidden (128)
    "tiny-qwen2": dict(hidden=128, inter=256, layers=2, heads=6, kv_heads=1, head_dim=64, vocab=256, qkv_bias=True),
    "tiny-qwen3": dict(hidden=128, inter=256, layers=2, heads=4, kv_heads=2, head_dim=64, vocab=256, qk_norm=True),
}


def make_config(name_or_cfg, **overrides) -> dict:
    cfg = dict(PRESETS[name_or_cfg]) if isinstance(name_or_cfg, str) else dict(name_or_cfg)
    cfg.setdefault("eps", 1e-5 if cfg.get("hidden", 0) >= 2048 else 1e-6)
    cfg.setdefault("rope_theta", 10000.0)
    cfg.setdefault("max_pos", 4096)
    cfg.update(overrides)
    assert cfg["heads"] % cfg["kv_heads"] == 0
    return cfg


def weight_shapes(cfg: dict) -> Dict[str, tuple]:
    hid, inter, H, Hkv, d, V = cfg["hidden"], cfg["inter"], cfg["heads"], cfg["kv_heads"], cfg["head_dim"], cfg["vocab"]
    shapes = {"embed": (V, hid), "norm": (hid,), "lm_head": (V, hid)}
    for i in range(cfg["layers"]):
        p = f"layers.{i}."
        shapes.update({p + "ln1": (hid,), p + "ln2": (hid,), p + "wq": (H * d, hid), p + "wk": (Hkv * d, hid),
                       p + "wv": (Hkv * d, hid), p + "wo": (hid, H * d), p + "wg": (inter, hid),
                       p + "wu": (inter, hid), p + "wd": (hid, inter)})
        if cfg.get("qkv_bias"):
            shapes.update({p + "bq": (H * d,), p + "bk": (Hkv * d,), p + "bv": (Hkv * d,)})
        if cfg.get("qk_norm"):
            shapes.update({p + "qn": (d,), p + "kn": (d,)})
    return shapes


# the random values of the Qwen keys: biases N(0, 0.5), norm weights 1 + N(0, 0.2) (HF initialises them to 0 / 1, which would hide both)
_BIAS_KEYS, _QKNORM_KEYS = ("bq", "bk", "bv"), ("qn", "kn")


def _kind(key: str) -> str:
    last = key.rsplit(".", 1)[-1]
    return "bias" if last in _BIAS_KEYS else ("qknorm" if last in _QKNORM_KEYS else ("norm" if last in ("ln1", "ln2", "norm") else "linear"))


def random_weights_numpy(cfg: dict, seed: int = 0, std: float = 0.02, tie_lm_head: bool = False) -> Dict[str, np.ndarray]:
    """Deterministic across machines (numpy RandomState stream, fixed key order).  HF init:
    normal(0, std) for linears/embeddings, ones for RMSNorm weights
    (lade/models/modeling_llama.py:934-943).  Meant for small (test) shapes."""
    rs = np.random.RandomState(seed)
    out: Dict[str, np.ndarray] = {}
    for k, shp in weight_shapes(cfg).items():
        kind = _kind(k)
        if kind == "bias":
            out[k] = (rs.standard_normal(shp) * 0.5).astype(np.float32)
        elif kind == "qknorm":
            out[k] = (1.0 + rs.standard_normal(shp) * 0.2).astype(np.float32)
        elif len(shp) == 1:
            out[k] = np.ones(shp, dtype=np.float32)
        else:
            out[k] = (rs.standard_normal(shp) * std).astype(np.float32)
    if tie_lm_head or cfg.get("tied"):
        out["lm_head"] = out["embed"].copy()
    return out


def random_weights_torch(cfg: dict, seed: int = 0, std: float = 0.02, dtype=torch.bfloat16, device="cuda",
                         tie_lm_head: bool = False) -> Dict[str, torch.Tensor]:
    """Large shapes: generate directly on the target device in `dtype` (7B in bf16 = 13.5 GB)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out: Dict[str, torch.Tensor] = {}
    for k, shp in weight_shapes(cfg).items():
        kind = _kind(k)
        if kind in ("bias", "qknorm"):
            w = torch.empty(shp, dtype=torch.float32, device=device)
            w.normal_(0.0, 0.5 if kind == "bias" else 0.2, generator=g)
            out[k] = (w if kind == "bias" else w + 1.0).to(dtype)
        elif len(shp) == 1:
            out[k] = torch.ones(shp, dtype=dtype, device=device)
        else:
            w = torch.empty(shp, dtype=dtype, device=device)
            w.normal_(0.0, std, generator=g)
            out[k] = w
    if tie_lm_head or cfg.get("tied"):
        out["lm_head"] = out["embed"]
    return out


def to_torch(weights: Dict[str, np.ndarray], dtype=torch.float32, device="cpu") -> Dict[str, torch.Tensor]:
    return {k: torch.as_tensor(v).to(device=device, dtype=dtype) for k, v in weights.items()}
