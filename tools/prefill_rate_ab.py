"""End-to-end A/B of the prefill rate (run on the GPU box):

    python tools/prefill_rate_ab.py [--preset llama2-7b] [--prompts 2048 8192 16384 32768] [--rounds 3] > profiles/prefill_rate_ab.txt

StepEngine.prefill of the full model in bf16 (random weights: the timing does not depend on the values), causal chunks of --chunk rows
(2048: what the generate() surface uses), tokens/s with the one-pass prefill attention kernel (LADE_DEBUG=prefill_attn=1) and without it
(lade_attn_fwd + lade_attn_combine, what the engine launched before).  One engine, the arms alternate per prompt length, --rounds rounds
after one untimed prefill per arm; host wall time around a synchronised prefill."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from lookaheaddecoding_amd import ops
    from lookaheaddecoding_amd.engine import StepEngine
    from lookaheaddecoding_amd.weights import make_config, random_weights_torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="llama2-7b")
    ap.add_argument("--layers", type=int, default=0, help="0 = the preset's")
    ap.add_argument("--prompts", type=int, nargs="+", default=[2048, 8192, 16384, 32768])
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    over = {"layers": a.layers} if a.layers else {}
    cfg = make_config(a.preset, max_pos=max(a.prompts) + 64, **over)
    w = random_weights_torch(cfg, seed=0, dtype=torch.bfloat16, device="cuda")
    eng = StepEngine(cfg, w, dtype=torch.bfloat16, device="cuda", max_seq=max(a.prompts) + 64, max_T=a.chunk, consume_weights=True)
    del w
    g = torch.Generator().manual_seed(5)
    print(f"# prefill rate A/B on {torch.cuda.get_device_name(0)}: {a.preset} ({cfg['layers']} layers) bf16, chunks of {a.chunk} rows; "
          f"new = LADE_DEBUG=prefill_attn=1 (lade_attn_prefill), old = the default (lade_attn_fwd + lade_attn_combine); {a.rounds} alternating rounds, tokens/s")
    keep = os.environ.get("LADE_DEBUG")

    def run(n, arm, ids):
        os.environ["LADE_DEBUG"] = ",".join(x for x in (keep, "prefill_attn=1" if arm == "new" else "prefill_attn=0") if x)
        eng.reset()
        before = ops.PREFILL_ATTN_CALLS
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.prefill(ids, [n - 1])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        used = ops.PREFILL_ATTN_CALLS - before
        assert (used > 0) == (arm == "new"), (arm, used)
        return n / dt

    for n in a.prompts:
        ids = torch.randint(3, cfg["vocab"], (n,), generator=g).tolist()
        rates = {"new": [], "old": []}
        for arm in ("new", "old"):
            run(n, arm, ids)                       # untimed: one-off GEMM autotune, allocator, code load
        for _ in range(a.rounds):
            for arm in ("new", "old"):
                rates[arm].append(run(n, arm, ids))
        mn, mo = statistics.median(rates["new"]), statistics.median(rates["old"])
        sp = {k: (max(v) - min(v)) / statistics.median(v) for k, v in rates.items()}
        print(f"  prompt {n:6d}: new {mn:10.1f} tok/s (rounds {' '.join(f'{r:.0f}' for r in rates['new'])}; spread {sp['new']:.1%}) | "
              f"old {mo:10.1f} tok/s (rounds {' '.join(f'{r:.0f}' for r in rates['old'])}; spread {sp['old']:.1%}) | new / old {mn / mo:.3f}", flush=True)


if __name__ == "__main__":
    main()
