"""A/B microbenchmark of the attention launch of a prefill chunk (run on the GPU box):

    python tools/prefill_attn_bench.py [--heads 7b 70b] [--points 2048:6144 512:0] [--block-ms 40] > profiles/prefill_attn_bench.txt

Arm A: what the engine launched for a causal chunk before lade_attn_prefill existed and launches unless LADE_DEBUG=prefill_attn=1 is set -
lade_attn_fwd with is_prefill and the engine's split rule (KernelDecisions.n_splits_for: never the single-launch form) + lade_attn_combine.
Arm B: lade_attn_prefill.  Both arms alternate inside this process, five block pairs per point; a block is `--block-ms` of back-to-back
launches between two device events (at least 200 ms of timed launches per arm and point at the default), after a warm-up of both arms.  The K / V
caches rotate over enough distinct allocations (> the 256 MB Infinity Cache in total) that a launch reads HBM, as the consecutive layers of a
real prefill do.  Per point: median and spread ((max - min) / median over the five blocks) of each arm, TFLOP/s on the causal flop count,
the fraction of the 2.5 PFLOP/s dense bf16 / f16 peak, A / B, and the arm the engine routes the chunk to under LADE_DEBUG=prefill_attn=1 (tuning.use_prefill_attn; without the switch every chunk runs arm A)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FLOPS = 2.5e15             # dense bf16 / f16 MFMA peak of an MI355X
HEAD_SETS = {"7b": (32, 32, 128), "13b": (40, 40, 128), "70b": (64, 8, 128), "tinyllama": (32, 4, 64)}
POINTS = [(2048, 0), (2048, 2048), (2048, 6144), (2048, 14336), (2048, 30720), (512, 0), (512, 6144), (1024, 0), (1024, 6144)]


def causal_flops(T: int, P: int, H: int, d: int) -> int:
    """flops of causal attention of T rows on top of P cached keys: row t sees P + t + 1 keys, 2 d flops per key for QK^T and 2 d for PV:
    4 d H (T P + T (T + 1) / 2)"""
    return 4 * d * H * (T * P + T * (T + 1) // 2)


def io_bytes(T: int, P: int, H: int, Hkv: int, d: int, elem: int = 2) -> int:
    """algorithmic bytes of one launch: K and V^T rows 0 .. P + T once per KV head, q in and out once"""
    return elem * (2 * Hkv * (P + T) * d + 2 * H * T * d)


def engine_splits(H: int, Hkv: int, T: int, S_tot: int, n_cu: int = 256, max_splits: int = 32) -> int:
    """KernelDecisions.n_splits_for for a chunk above the last row class: the 128-row work-group, the sqrt rule, never a single launch"""
    from lookaheaddecoding_amd import ops
    return min(ops.choose_splits(H, H // Hkv, T, max(S_tot, 1024), n_cu, allow_single=False, block_rows=0, mode=0), max_splits)


def main():
    import torch
    from lookaheaddecoding_amd import ops
    from lookaheaddecoding_amd.tuning import use_prefill_attn
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", nargs="+", default=["7b", "13b", "70b", "tinyllama", "7b:f16"], help="head sets (7b 13b 70b tinyllama), ':f16' for float16")
    ap.add_argument("--points", nargs="+", default=[f"{T}:{P}" for T, P in POINTS], help="T:P pairs")
    ap.add_argument("--block-ms", type=float, default=40.0, help="timed launches per block and arm")
    ap.add_argument("--pairs", type=int, default=5)
    a = ap.parse_args()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# prefill attention A/B on {torch.cuda.get_device_name(0)} ({n_cu} CUs): A = lade_attn_fwd(is_prefill, engine splits) + lade_attn_combine, "
          f"B = lade_attn_prefill; {a.pairs} alternating block pairs of >= {a.block_ms:.0f} ms per arm; spread = (max - min) / median of the blocks")
    print(f"# {'heads':14s} {'T':>5s} {'P':>6s} {'ns':>3s} | {'A us':>9s} {'spread':>7s} {'TF/s':>7s} {'of peak':>7s} | {'B us':>9s} {'spread':>7s} {'TF/s':>7s} {'of peak':>7s} | {'A/B':>6s} {'B/A':>6s} engine")
    for hs in a.heads:
        name, _, dts = hs.partition(":")
        H, Hkv, d = HEAD_SETS[name] if name in HEAD_SETS else tuple(int(x) for x in name.split(","))        # or "H,Hkv,d"
        dtype = torch.float16 if dts == "f16" else torch.bfloat16
        for pt in a.points:
            T, P = (int(x) for x in pt.split(":"))
            S_max = (P + T + 63) // 64 * 64 + 64
            per = 2 * Hkv * S_max * d * 2
            n_rot = max(2, min(64, -(-600_000_000 // per)))
            k = [torch.randn(Hkv, S_max, d, device="cuda").to(dtype) for _ in range(n_rot)]
            vt = [torch.randn(Hkv, d, S_max, device="cuda").to(dtype) for _ in range(n_rot)]
            qkv = torch.randn(T, (H + 2 * Hkv) * d, device="cuda").to(dtype)          # q stays inside the qkv buffer, as in the engine
            q = qkv[:, :H * d]
            out = torch.empty(T, H * d, dtype=dtype, device="cuda")
            mask = ops.StepMask(T=T, P=P, is_prefill=True)
            ns = engine_splits(H, Hkv, T, P + T, n_cu)
            part_o = torch.empty(ns, T, H, d, dtype=dtype, device="cuda")
            part_ml = torch.empty(ns, H, T, 2, dtype=torch.float32, device="cuda")

            def arm_a(i):
                ops.attn_fwd(q, k[i % n_rot], vt[i % n_rot], mask, H=H, Hkv=Hkv, d=d, out=out, n_splits=ns, part_o=part_o, part_ml=part_ml)

            def arm_b(i):
                ops.attn_prefill(q, k[i % n_rot], vt[i % n_rot], mask, H=H, Hkv=Hkv, d=d, out=out)

            def block(fn, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(reps):
                    fn(i)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / reps           # us per launch

            reps, times = {}, {"A": [], "B": []}
            for nm, fn in (("A", arm_a), ("B", arm_b)):
                block(fn, 3)                                       # warm-up (first launch: LDS opt-in, code load)
                reps[nm] = max(3, int(a.block_ms * 1e3 / max(block(fn, 5), 1.0)) + 1)
            for _ in range(a.pairs):
                times["A"].append(block(arm_a, reps["A"]))
                times["B"].append(block(arm_b, reps["B"]))
            fl = causal_flops(T, P, H, d)
            cols = []
            for nm in ("A", "B"):
                med = statistics.median(times[nm])
                cols.append((med, (max(times[nm]) - min(times[nm])) / med, fl / med * 1e-6, fl / (med * 1e-6) / PEAK_FLOPS))
            (ma, sa, ta, pa), (mb, sb, tb, pb) = cols
            routed = 'B' if use_prefill_attn(T, True, dtype, switch='1', H=H, Hkv=Hkv, n_cu=n_cu) else 'A'
            print(f"  {hs:14s} {T:5d} {P:6d} {ns:3d} | {ma:9.1f} {sa:6.1%} {ta:7.1f} {pa:6.1%} | {mb:9.1f} {sb:6.1%} {tb:7.1f} {pb:6.1%} | {ma / mb:6.2f} {mb / ma:6.2f} {routed}", flush=True)
            del k, vt, qkv, q, out, part_o, part_ml
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
