"""What per-token scores / logits (generate(return_dict_in_generate=True)) cost in the steady lookahead step.

    python tools/emit_bench.py [--steps K] [--warmup W] [--rounds R] [--presets llama2-7b,qwen2.5-7b]

At the c2 shape (llama2-7b, W15 N5 G15) and qwen2.5-7b, bf16, random weights, 128-token prompt, hipGraph steps: the host clock around K steady steps
with the emit request off (the plain step: lm_head argmax epilogue), with "scores" and with "scores" + "logits" (the lm_head materialises
its logits, lade_argmax_rows reads them, lade_emit_rows copies the rows of the accepted tokens behind the post-step), alternated R times.
Prints one JSON line per preset with the medians and the ratios to off."""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lookaheaddecoding_amd.decoding import LookaheadDecoder  # noqa: E402
from lookaheaddecoding_amd.engine import StepEngine  # noqa: E402
from lookaheaddecoding_amd.weights import make_config, random_weights_torch  # noqa: E402

MODES = (("off", None), ("scores", ("scores",)), ("scores_logits", ("scores", "logits")))


def _timed(dec, prompt, emit, steps, warmup):
    dec.start(prompt, rng=random.Random(1), emit=emit, emit_cap=(steps + warmup) * (dec.gs + 1))
    for _ in range(warmup):
        dec.step()
    torch.cuda.synchronize()
    tok0 = len(dec.tokens)
    t0 = time.perf_counter()
    for _ in range(steps):
        dec.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    if emit is not None:                   # the rows are there: as many as tokens were emitted
        got = dec.emitted(len(dec.tokens) - len(dec.prompt))
        assert set(got) == set(emit)
    return ms, (len(dec.tokens) - tok0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--presets", default="llama2-7b,qwen2.5-7b")
    a = ap.parse_args()
    for preset in a.presets.split(","):
        cfg = make_config(preset)
        w = random_weights_torch(cfg, seed=0, dtype=torch.bfloat16, device="cuda")
        eng = StepEngine(cfg, w, dtype=torch.bfloat16, device="cuda", max_seq=4096, max_T=512, consume_weights=True)
        del w
        prompt = torch.randint(3, cfg["vocab"], (128,), generator=torch.Generator().manual_seed(123)).tolist()
        dec = LookaheadDecoder(eng, 15, 5, 15, use_graph=True)
        ms = {name: [] for name, _ in MODES}
        tok = {name: [] for name, _ in MODES}
        for _ in range(a.rounds):
            for name, emit in MODES:
                t, tps = _timed(dec, prompt, emit, a.steps, a.warmup)
                ms[name].append(t)
                tok[name].append(tps)
        med = {name: statistics.median(v) for name, v in ms.items()}
        print(json.dumps({"measure": "step", "preset": preset, "V": cfg["vocab"], "W": 15, "N": 5, "G": 15, "graph": True, "steps": a.steps,
                          "rounds": a.rounds, **{f"{n}_ms_per_step": round(v, 3) for n, v in med.items()},
                          "scores_over_off": round(med["scores"] / med["off"], 4), "scores_logits_over_off": round(med["scores_logits"] / med["off"], 4),
                          **{f"{n}_tokens_per_step": round(statistics.median(v), 3) for n, v in tok.items()},
                          **{f"{n}_all": [round(x, 3) for x in v] for n, v in ms.items()}}), flush=True)
        del dec, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
