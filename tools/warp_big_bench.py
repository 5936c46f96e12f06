"""lade_warp_rows on a Llama-3-class vocabulary (V = 128256: the row's keys live in the output row, csrc/sampling.hip) against the torch
ops it replaces (`sampling.Warper.__call__`: division, topk, sort, softmax, cumsum, scatter, masked_fill), 31 rows (1 + 15 + 15 of a
config-3 step), microseconds per call; and the register form at V = 32000 for scale.   python tools/warp_big_bench.py

`--ex`: the arm of lade_warp_rows_ex (min_p, typical_p, epsilon_cutoff, eta_cutoff behind the three).  The arms are timed in alternating
blocks (one block of every arm, then the next round) and reported as the median block with the smallest and largest one:
  three      lade_warp_rows at (0.8, 40, 0.95) - the kernel the later stages must leave as it was (`--ex --three-only` times nothing else)
  seven      all seven stages in one launch
  fallback   what that launch displaces: lade_warp_rows, then HF's four warper objects as torch ops on the device
  + stage    lade_warp_rows_ex with one later stage switched on (its increment over `three`)

`--ab OTHER.so`: lade_warp_rows at (0.8, 40, 0.95) of another build of the library (the parent commit's, say) against this tree's, both
loaded into this one process through ctypes, 9 rounds of alternating blocks of 200 calls; the two outputs must be bit-equal."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lookaheaddecoding_amd import ops
from lookaheaddecoding_amd.sampling import Warper


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def ex_arms(three_only=False, rounds=7):
    from transformers.generation import logits_process as lp
    T, K, P = 0.8, 40, 0.95
    later = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)
    for V in (32000, 128256):
        lg = (torch.randn(31, V, device="cuda") * 3.0).bfloat16()
        out = torch.empty(31, V, dtype=torch.float32, device="cuda")
        hf = [lp.MinPLogitsWarper(later["min_p"]), lp.TypicalLogitsWarper(later["typical_p"]), lp.EpsilonLogitsWarper(later["epsilon_cutoff"]),
              lp.EtaLogitsWarper(later["eta_cutoff"], device="cuda")]

        def fallback():
            x = ops.warp_rows(lg, 31, 0, T, K, P, out=out)
            for wp in hf:
                x = wp(None, x)
            return x

        arms = {"three": lambda: ops.warp_rows(lg, 31, 0, T, K, P, out=out)}
        if not three_only:
            arms["seven"] = lambda: ops.warp_rows(lg, 31, 0, T, K, P, out=out, **later)
            arms["fallback"] = fallback
            for name, value in later.items():
                arms["+ " + name] = (lambda n, v: lambda: ops.warp_rows(lg, 31, 0, T, K, P, out=out, **{n: v}))(name, value)
        times = {name: [] for name in arms}
        for _ in range(rounds):
            for name, fn in arms.items():
                times[name].append(timed(fn, reps=100))
        for name, ts in times.items():
            ts = sorted(ts)
            print(f"V={V:6d} T={T} top_k={K} top_p={P} {name:18s} median {ts[len(ts) // 2]:8.1f} us   (blocks {ts[0]:.1f} .. {ts[-1]:.1f})", flush=True)


def ab_three(other_path, rounds=9):
    import ctypes as C
    from lookaheaddecoding_amd import cabi
    libs = {"other": C.CDLL(os.path.abspath(other_path)), "this": C.CDLL(cabi.LIB_PATH)}
    for lib in libs.values():
        lib.lade_warp_rows.argtypes, lib.lade_warp_rows.restype = cabi.SIGNATURES["lade_warp_rows"], C.c_int
    for V in (32000, 128256):
        lg = (torch.randn(31, V, device="cuda") * 3.0).bfloat16()
        outs = {name: torch.empty(31, V, dtype=torch.float32, device="cuda") for name in libs}
        st = cabi.stream_ptr()

        def run(name):
            rc = libs[name].lade_warp_rows(lg.data_ptr(), lg.stride(0), 31, V, cabi.LADE_BF16, 0.8, 40, 0.95, 0, outs[name].data_ptr(), st)
            assert rc == 0, (name, rc)

        times = {name: [] for name in libs}
        for _ in range(rounds):
            for name in libs:
                times[name].append(timed(lambda: run(name), reps=200))
        assert torch.equal(outs["other"], outs["this"]), f"V={V}: the two builds' outputs differ"
        for name, ts in times.items():
            ts = sorted(ts)
            print(f"V={V:6d} lade_warp_rows(0.8, 40, 0.95) {name:6s} median {ts[len(ts) // 2]:8.1f} us   (blocks {ts[0]:.1f} .. {ts[-1]:.1f})   outputs bit-equal",
                  flush=True)


if "--ab" in sys.argv:
    ab_three(sys.argv[sys.argv.index("--ab") + 1])
    sys.exit(0)
if "--ex" in sys.argv:
    ex_arms(three_only="--three-only" in sys.argv)
    sys.exit(0)

for V in (32000, 128256):
    lg = (torch.randn(31, V, device="cuda") * 3.0).bfloat16()
    for (temp, k, p) in ((0.8, 50, 0.9), (1.0, 0, 0.9), (0.7, 40, 1.0)):
        w = Warper(temp, k, p)
        out = torch.empty(31, V, dtype=torch.float32, device="cuda")
        t_hip = timed(lambda: ops.warp_rows(lg, 31, 0, temp, k, p, out=out))
        t_torch = timed(lambda: w(lg.float()))
        print(f"V={V:6d} T={temp} top_k={k:3d} top_p={p}: lade_warp_rows {t_hip:8.1f} us   torch warpers {t_torch:8.1f} us", flush=True)
