"""What the generation controls (repetition penalty / min length on the device) cost in the steady lookahead step.

    python tools/gen_controls_bench.py [--steps K] [--warmup W] [--rounds R]
    python tools/gen_controls_bench.py --loop off|on      # one steady greedy loop only (for rocprofv3 --kernel-trace --stats)
    python tools/gen_controls_bench.py --kernel           # lade_gen_argmax alone against lade_argmax_rows, 16 and 76 rows
    python tools/gen_controls_bench.py --constraints      # the step with token constraints on top of the penalty, against the penalty alone

At the c2 shape (llama2-7b, W15 N5 G15) and qwen2.5-7b, bf16, random weights, 128-token prompt, hipGraph steps: the host clock around
K steps with the controls off (the plain step: lm_head argmax epilogue) and on (repetition_penalty 1.05: the lm_head materialises the
logits, lade_gen_argmax reads them once, lade_gen_ctl_update after the post-step), alternated R times.  Prints one JSON line per preset
with the medians, on / off and the logits rows of the steps that were timed (1 + W + the candidate bucket's rows).
`--kernel`: hipEvent time of lade_gen_argmax (penalty 1.05, a 2048-token seen set) and of lade_argmax_rows on bf16 rows of V = 32000 and
152064, at 16 rows (no candidates) and 76 rows (W15 N5 G15 with all 15 candidates); and of lade_gen_rows (the sampling path: it also
stores the processed fp32 rows) with the penalty alone and with the constraint block attached.
`--constraints`: the same alternating rounds with both arms under repetition_penalty 1.05, one of them with 64 suppressed ids and 32
sequence entries of 2 to 4 tokens (half of them -inf, a quarter built from the prompt's own n-grams so that they can fire): one graph
serves both arms, the block is rewritten in place."""
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

from lookaheaddecoding_amd.decoding import GenControls, LookaheadDecoder  # noqa: E402
from lookaheaddecoding_amd.engine import StepEngine  # noqa: E402
from lookaheaddecoding_amd.weights import make_config, random_weights_torch  # noqa: E402

PRESETS = ("llama2-7b", "qwen2.5-7b")
ON = GenControls(penalty=1.05)


def constrained(V: int, prompt, penalty: float = 1.05) -> GenControls:
    """the constraints arm: 64 suppressed ids, 32 sequence entries of length 2 to 4 (every other one -inf, every fourth from the prompt)"""
    g = torch.Generator().manual_seed(7)
    ban = tuple(torch.randint(3, V, (64,), generator=g).tolist())
    entries = []
    for e in range(32):
        n = 2 + e % 3
        if e % 4 == 0:
            at = int(torch.randint(0, len(prompt) - n, (1,), generator=g))
            seq = tuple(int(t) for t in prompt[at:at + n])
        else:
            seq = tuple(torch.randint(3, V, (n,), generator=g).tolist())
        entries.append((seq, -float("inf") if e % 2 else (-4.0 if e % 4 else 2.5)))
    return GenControls(penalty=penalty, ban=ban, sequence_bias=tuple(entries), add_bias=True)


def _timed(dec, prompt, controls, steps, warmup, rows=None):
    dec.start(prompt, rng=random.Random(1), controls=controls)
    for _ in range(warmup):
        dec.step()
    torch.cuda.synchronize()
    tok0 = len(dec.tokens)
    infos = []
    t0 = time.perf_counter()
    for _ in range(steps):
        infos.append(dec.step())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    if rows is not None:                    # logits rows of each timed step: out + window + the replayed bucket's candidate rows
        rows += [1 + dec.W + info["T"] - (dec.N - 1) * dec.W for info in infos]
    return ms, (len(dec.tokens) - tok0) / steps


def kernel(reps: int) -> None:
    from lookaheaddecoding_amd import cabi, ops
    W, gs = 15, 4
    for V in (32000, 152064):
        gen = torch.zeros(cabi.gen_words(V), dtype=torch.int32, device="cuda")
        seen = torch.randint(0, V, (2048,), dtype=torch.int32, device="cuda")
        ops.gen_ctl_init(gen, V, 1.05, 0, [2], seen)
        for rows in (16, 76):
            g = (rows - 1 - W) // gs
            logits = torch.randn(rows, V, device="cuda").to(torch.bfloat16)
            ctl = torch.zeros(cabi.CTL_WORDS, dtype=torch.int32, device="cuda")
            ctl[cabi.CTL_G] = g
            guess = torch.randint(0, V, (max(g, 1) * gs,), dtype=torch.int32, device="cuda")
            pos = torch.arange(2000, 2000 + rows, dtype=torch.int32, device="cuda")
            am = torch.zeros(rows, dtype=torch.int32, device="cuda")
            rows_out = torch.empty(rows - W, V, dtype=torch.float32, device="cuda")
            cons = torch.zeros(cabi.gen_cons_words(V), dtype=torch.int32, device="cuda")
            c = constrained(V, seen.tolist())

            def attach(on):
                ops.gen_ctl_init(gen, V, 1.05, 0, [2], seen)
                if on:
                    ops.gen_constraints_init(gen, cons, V, c.ban, c.begin_ban, c.begin_index, c.sequence_bias, c.add_bias, seen)

            runs = {"gen_argmax": (False, lambda: ops.gen_argmax(logits, W, gs, gen, ctl, guess, pos, None, am)),
                    "argmax_rows": (False, lambda: ops.argmax_rows(logits, out=am)),
                    "gen_rows": (False, lambda: ops.gen_argmax(logits, W, gs, gen, ctl, guess, pos, None, am, rows_out)),
                    "gen_argmax_constrained": (True, lambda: ops.gen_argmax(logits, W, gs, gen, ctl, guess, pos, None, am)),
                    "gen_rows_constrained": (True, lambda: ops.gen_argmax(logits, W, gs, gen, ctl, guess, pos, None, am, rows_out))}
            res = {}
            for name, (on, fn) in runs.items():
                attach(on)
                for _ in range(10):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[name] = round(e0.elapsed_time(e1) / reps * 1e3, 2)
            print(json.dumps({"measure": "kernel", "V": V, "rows": rows, "candidates": g, "dtype": "bf16", "reps": reps,
                              "gen_argmax_us": res["gen_argmax"], "argmax_rows_us": res["argmax_rows"], "gen_rows_us": res["gen_rows"],
                              "gen_argmax_constrained_us": res["gen_argmax_constrained"],
                              "gen_rows_constrained_us": res["gen_rows_constrained"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop", choices=("off", "on"), default=None)
    ap.add_argument("--presets", default=",".join(PRESETS))
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--constraints", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if a.kernel:
        kernel(a.reps)
        return
    for preset in a.presets.split(","):
        cfg = make_config(preset)
        w = random_weights_torch(cfg, seed=0, dtype=torch.bfloat16, device="cuda")
        eng = StepEngine(cfg, w, dtype=torch.bfloat16, device="cuda", max_seq=4096, max_T=512, consume_weights=True)
        del w
        prompt = torch.randint(3, cfg["vocab"], (128,), generator=torch.Generator().manual_seed(123)).tolist()
        dec = LookaheadDecoder(eng, 15, 5, 15, use_graph=True)
        if a.loop is not None:
            ms, tps = _timed(dec, prompt, ON if a.loop == "on" else None, a.steps, a.warmup)
            print(json.dumps({"measure": "loop", "preset": preset, "controls": a.loop, "ms_per_step": round(ms, 3)}), flush=True)
        elif a.constraints:
            cons_arm = constrained(cfg["vocab"], prompt)
            on, con, tok_on, tok_con, rows = [], [], [], [], []
            _timed(dec, prompt, ON, a.steps, a.warmup)          # (capture and first-use costs stay out of both arms)
            for _ in range(a.rounds):
                ms, tps = _timed(dec, prompt, ON, a.steps, a.warmup)
                on.append(ms)
                tok_on.append(tps)
                ms, tps = _timed(dec, prompt, cons_arm, a.steps, a.warmup, rows)
                con.append(ms)
                tok_con.append(tps)
            m_on, m_con = statistics.median(on), statistics.median(con)
            print(json.dumps({"measure": "constraints_step", "preset": preset, "W": 15, "N": 5, "G": 15, "graph": True, "steps": a.steps,
                              "rounds": a.rounds, "suppressed_ids": len(cons_arm.ban), "sequence_entries": len(cons_arm.sequence_bias),
                              "penalty_only_ms_per_step": round(m_on, 3), "constrained_ms_per_step": round(m_con, 3),
                              "constrained_over_penalty_only": round(m_con / m_on, 4),
                              "penalty_only_tokens_per_step": round(statistics.median(tok_on), 3),
                              "constrained_tokens_per_step": round(statistics.median(tok_con), 3),
                              "penalty_only_all": [round(x, 3) for x in on], "constrained_all": [round(x, 3) for x in con],
                              "constrained_logits_rows": {str(r): rows.count(r) for r in sorted(set(rows))}}), flush=True)
        else:
            off, on, tok_off, tok_on, rows = [], [], [], [], []
            for _ in range(a.rounds):
                ms, tps = _timed(dec, prompt, None, a.steps, a.warmup)
                off.append(ms)
                tok_off.append(tps)
                ms, tps = _timed(dec, prompt, ON, a.steps, a.warmup, rows)
                on.append(ms)
                tok_on.append(tps)
            m_off, m_on = statistics.median(off), statistics.median(on)
            print(json.dumps({"measure": "step", "preset": preset, "W": 15, "N": 5, "G": 15, "graph": True, "steps": a.steps, "rounds": a.rounds,
                              "off_ms_per_step": round(m_off, 3), "on_ms_per_step": round(m_on, 3), "on_over_off": round(m_on / m_off, 4),
                              "off_tokens_per_step": round(statistics.median(tok_off), 3), "on_tokens_per_step": round(statistics.median(tok_on), 3),
                              "off_all": [round(x, 3) for x in off], "on_all": [round(x, 3) for x in on],
                              "on_logits_rows": {str(r): rows.count(r) for r in sorted(set(rows))}}), flush=True)
        del dec, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
