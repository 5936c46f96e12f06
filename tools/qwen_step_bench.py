"""Qwen2 / Qwen3 on the step engine: what the qkv epilogue costs.

    python tools/qwen_step_bench.py kernel            # the epilogue kernel against the call without an epilogue (run it under
                                                      #   rocprofv3 --kernel-trace --stats -- python tools/qwen_step_bench.py kernel)
    python tools/qwen_step_bench.py step [--steps K]  # lookahead step time (W15 N5 G15, hipGraph) and plain decoding per token

`kernel`: at the step shape of qwen2.5-7b (bias) and qwen3-8b (head norm, and bias + norm), T = 60 rows of split-K partials (--parts of
them, 2 by default), lade_rope_kv_append without and with the epilogue launched alternately on the same
inputs, one launch per layer's K/V cache (the caches of all layers together are larger than the Infinity Cache, as in the step).
The two kernels carry distinct names (rope_kv_append_kernel<T, false> / <T, true>), so the trace's per-kernel statistics are the A/B.
`step`: both presets at full depth in bf16 (random weights; prompt of 128 tokens), the host clock around K hipGraph steps after a
warm-up, and plain greedy decoding on the same engine (per token, its 128-token prefill included once).
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lookaheaddecoding_amd import ops  # noqa: E402
from lookaheaddecoding_amd.engine import rope_tables  # noqa: E402
from lookaheaddecoding_amd.weights import make_config, random_weights_torch  # noqa: E402

PRESETS = ("qwen2.5-7b", "qwen3-8b")


def kernel(reps: int, n_parts: int) -> None:
    dev, dt, T, P = "cuda", torch.bfloat16, 60, 1000
    for preset in PRESETS:
        cfg = make_config(preset)
        H, Hkv, d, L = cfg["heads"], cfg["kv_heads"], cfg["head_dim"], cfg["layers"]
        row_w = (H + 2 * Hkv) * d
        g = torch.Generator(device=dev).manual_seed(0)
        parts = torch.randn(n_parts, T, row_w, device=dev, generator=g)
        q = torch.empty(T, H * d, dtype=dt, device=dev)
        S_max = 2048
        kcs = [torch.zeros(Hkv, S_max, d, dtype=dt, device=dev) for _ in range(L)]
        vts = [torch.zeros(Hkv, d, S_max, dtype=dt, device=dev) for _ in range(L)]
        cos, sin = rope_tables(d, 4096, cfg["rope_theta"], dt, dev)
        pos = torch.arange(P, P + T, dtype=torch.int32, device=dev)
        bias = (0.5 * torch.randn(row_w, device=dev, generator=g)).to(dt)
        qn = (1 + 0.2 * torch.randn(d, device=dev, generator=g)).to(dt)
        kn = (1 + 0.2 * torch.randn(d, device=dev, generator=g)).to(dt)
        forms = {"bias": ops.qkv_epilogue(bias, None, None, cfg["eps"])} if cfg.get("qkv_bias") else \
                {"norm": ops.qkv_epilogue(None, qn, kn, cfg["eps"]), "bias+norm": ops.qkv_epilogue(bias, qn, kn, cfg["eps"])}
        for name, epi in forms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            for _ in range(20):                            # warm-up
                for li in range(L):
                    ops.rope_kv_append_parts(parts, n_parts, q, pos, cos, sin, kcs[li], vts[li], T, P, H=H, Hkv=Hkv, d=d)
                    ops.rope_kv_append_parts(parts, n_parts, q, pos, cos, sin, kcs[li], vts[li], T, P, H=H, Hkv=Hkv, d=d, epi=epi)
            t_plain = t_epi = 0.0
            for r in range(reps):                          # alternated: plain layer sweep, epilogue layer sweep
                ev[0].record()
                for li in range(L):
                    ops.rope_kv_append_parts(parts, n_parts, q, pos, cos, sin, kcs[li], vts[li], T, P, H=H, Hkv=Hkv, d=d)
                ev[1].record()
                for li in range(L):
                    ops.rope_kv_append_parts(parts, n_parts, q, pos, cos, sin, kcs[li], vts[li], T, P, H=H, Hkv=Hkv, d=d, epi=epi)
                ev[2].record()
                torch.cuda.synchronize()
                t_plain += ev[0].elapsed_time(ev[1])
                t_epi += ev[1].elapsed_time(ev[2])
            us_plain, us_epi = t_plain / reps / L * 1e3, t_epi / reps / L * 1e3
            print(json.dumps({"measure": "kernel", "preset": preset, "epilogue": name, "T": T, "n_parts": n_parts, "layers": L, "reps": reps,
                              "plain_us_per_layer_events": round(us_plain, 3), "epilogue_us_per_layer_events": round(us_epi, 3),
                              "ratio_events": round(us_epi / us_plain, 3)}), flush=True)


def step(steps: int, warmup: int, plain_tokens: int) -> None:
    from lookaheaddecoding_amd.decoding import LookaheadDecoder
    from lookaheaddecoding_amd.engine import StepEngine
    for preset in PRESETS:
        cfg = make_config(preset)
        w = random_weights_torch(cfg, seed=0, dtype=torch.bfloat16, device="cuda")
        eng = StepEngine(cfg, w, dtype=torch.bfloat16, device="cuda", max_seq=4096, max_T=512, consume_weights=True)
        del w
        prompt = torch.randint(3, cfg["vocab"], (128,), generator=torch.Generator().manual_seed(123)).tolist()
        dec = LookaheadDecoder(eng, 15, 5, 15, use_graph=True)
        dec.start(prompt, rng=random.Random(1))
        for _ in range(warmup):
            dec.step()
        torch.cuda.synchronize()
        tok0 = len(dec.tokens)
        t0 = time.perf_counter()
        for _ in range(steps):
            dec.step()
        torch.cuda.synchronize()
        la_ms = (time.perf_counter() - t0) / steps * 1e3
        la_tok = (len(dec.tokens) - tok0) / steps
        eng.plain_greedy(prompt, len(prompt) + 8)          # warm-up (T = 1 row class decisions)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.plain_greedy(prompt, len(prompt) + plain_tokens)
        torch.cuda.synchronize()
        plain_ms = (time.perf_counter() - t0) / plain_tokens * 1e3        # (includes the 128-token prefill, once)
        print(json.dumps({"measure": "step", "preset": preset, "layers": cfg["layers"], "W": 15, "N": 5, "G": 15, "graph": True,
                          "steps": steps, "lookahead_ms_per_step": round(la_ms, 3), "tokens_per_step": round(la_tok, 3),
                          "plain_tokens": plain_tokens, "plain_ms_per_token": round(plain_ms, 3),
                          "qkv_gemm": list(eng.gemm_cfg.get(("wqkv", 128)) or []) or None}), flush=True)
        del dec, eng
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "step"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--plain-tokens", type=int, default=64)
    a = ap.parse_args()
    if a.what == "kernel":
        kernel(a.reps, a.parts)
    else:
        step(a.steps, a.warmup, a.plain_tokens)


if __name__ == "__main__":
    main()
