"""GPU: the two application-level scripts kept from the reference run end to end on the drop-in surface:
examples/minimal.py (reference: minimal.py:29-52) and examples/eval_synthetic.py (reference: applications/eval_mtbench.py:267-386)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT


def _run(args, env_extra, timeout=600):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_minimal_example_lookahead_equals_plain_hf_fp32():
    out = _run(["examples/minimal.py", "--shape", "tiny-d64", "--dtype", "float32", "--max-new-tokens", "48", "--level", "4", "--window", "5", "--guess", "5"],
               {"LOAD_LADE": "1", "USE_LADE": "1"})
    assert "Greedy Generated Tokens: 48" in out and "Sample Generated Tokens: 48" in out
    assert "LADE LOG - OVERALL GEN:" in out
    assert "lookahead greedy ids identical: True" in out, out[-800:]


def test_eval_harness_writes_answers_stats_and_log(tmp_path):
    ans = str(tmp_path / "answers" / "synthetic.jsonl")
    out = _run(["examples/eval_synthetic.py", "--answer-file", ans, "--shape", "tiny-d64", "--dtype", "float32", "--questions", "3", "--max-new-token", "24",
                "--level", "4", "--window", "5", "--guess", "5"], {"USE_LADE": "1"})
    recs = [json.loads(l) for l in open(ans)]
    assert [r["question_id"] for r in recs] == [81, 82, 83]
    for r in recs:
        assert set(r) == {"question_id", "answer_id", "model_id", "choices", "tstamp"}
        ch = r["choices"][0]
        assert ch["index"] == 0 and len(ch["turns"]) == 2 and len(ch["prompts"]) == 2
        assert all(len(t) == 24 for t in ch["turns"])
        assert ch["prompts"][1][:len(ch["prompts"][0])] == ch["prompts"][0]           # the second prompt continues the conversation
        assert ch["prompts"][1][len(ch["prompts"][0]):len(ch["prompts"][0]) + 24] == ch["turns"][0]
    stats = torch.load(ans + ".pt")
    assert set(stats) == {0, 1} and all(len(v) == 2 and v[1] == 24 for v in stats.values())
    log = torch.load(ans + "-lade-log.pt")
    assert len(log) == 6 and all(e[0] == 24 and e[1] <= 24 for e in log)          # [generated, steps, ratio] per generate call
    assert "AVERAGE THROUGHPUT1" in out and "LADE LOG - OVERALL GEN:  144" in out


def test_bench_spawns_its_own_ranks_and_prints_one_json_line_last():
    """`python bench.py --gpus N` without a launcher starts its ranks itself (torch.multiprocessing.spawn, one per GPU, RCCL between
    them).  One GPU here: the spawn path is exercised with one rank on the lookahead-parallel code path (real RCCL group), a reduced
    layer count, and the contract is checked on what it prints: the JSON line is the last line of stdout."""
    out = _run(["bench.py", "--gpus", "1", "--force-lp", "--layers", "2", "--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline", "--prompt-len", "256"],
               {"LADE_BENCH_FORCE_SPAWN": "1"})
    lines = [l for l in out.splitlines() if l.strip()]
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1 and d["config"]["parallelism"] == "lp1" and d["value"] > 0
    assert d["scaling"] == "weak" and d["roofline"]["bound"] == "hbm" and "prefill" in d
    # asking for more GPUs than the box has fails loudly instead of silently running one rank
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "3", "--steps", "1"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "GPU" in (r.stderr + r.stdout)


def test_bench_two_ranks_end_to_end_on_one_gpu():
    """The N > 1 path of bench.py from the first line to the JSON line: two spawned ranks, lookahead parallelism between them (window and
    candidates sharded, one all-gather per step, GEMM choices of rank 0 adopted by rank 1, max-over-ranks timing).  Both ranks sit on the
    one GPU of this box, which RCCL refuses, so the process group is gloo here (LADE_BENCH_SHARE_GPU / LADE_BENCH_BACKEND, test-only
    switches); the token-level parity of the sharded step is pinned in test_gpu_lp.py / test_lp_gloo.py."""
    out = _run(["bench.py", "--gpus", "2", "--layers", "2", "--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline", "--prompt-len", "256"],
               {"LADE_BENCH_SHARE_GPU": "1", "LADE_BENCH_BACKEND": "gloo"})
    lines = [l for l in out.splitlines() if l.strip()]
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["config"]["parallelism"] == "lp2" and d["config"]["shared_gpu"] is True
    assert d["scaling"] == "strong" and d["value"] > 0 and d["step_compression"] >= 1.0
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["T"] < 60          # rank 0's shard of the 60-token step
    _check_multi_rank_line(d, 2)


def _check_multi_rank_line(d, R):
    """what a scaling run needs to be interpretable (round-4 review): the collective's real span, the BASELINE configuration's expected (flat)
    curve, and the reference-default configuration - the one that shards - measured by the same ranks in the same line"""
    assert d["config"]["collective_ranks"] == R and "expected" in d and set(d["expected"]["speedup_vs_one_rank"]) == {"2", "4", "8"}
    assert "unmeasured" in d["expected"]["status"]
    lpd = d["lp_default"]
    assert "error" not in lpd, lpd
    assert (lpd["W"], lpd["N"], lpd["G"]) == (60, 8, 60) and lpd["value"] > 0 and lpd["ms_per_step"] > 0 and lpd["step_compression"] >= 1.0
    assert len(lpd["rows_per_rank_cold"]) == R and max(lpd["rows_per_rank_cold"]) < lpd["rows_one_rank_cold"] == 420
    assert lpd["expected_speedup_vs_one_rank"] == {"2": 1.44, "4": 1.74, "8": 2.11}


def test_bench_eight_ranks_end_to_end_on_one_gpu():
    """the same with EIGHT ranks - the world size the driver's scaling run ends at: window columns 15 / 8 -> 2 per rank (the last rank gets 1),
    candidates sharded eight ways, rank 0's kernel decisions adopted by seven others; the line carries both configurations."""
    out = _run(["bench.py", "--gpus", "8", "--layers", "2", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--prompt-len", "256"],
               {"LADE_BENCH_SHARE_GPU": "1", "LADE_BENCH_BACKEND": "gloo"})
    lines = [l for l in out.splitlines() if l.strip()]
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 8 and d["steps"] == 3 and d["config"]["parallelism"] == "lp8" and d["config"]["shared_gpu"] is True
    assert d["scaling"] == "strong" and d["value"] > 0 and d["roofline"]["bound"] == "hbm" and d["roofline"]["T"] <= 16
    _check_multi_rank_line(d, 8)


def test_bench_plain_run_is_lean_and_its_outputs_repeat(tmp_path):
    """A plain `bench.py` run times exactly --steps steps and prints the contract without the --full measurements; --dump-outputs writes
    what the timed steps emitted, and a second run with the same arguments writes the same arrays (seeded weights, prompt and window)."""
    outs = []
    for i in range(2):
        d_out = tmp_path / f"run{i}"
        out = _run(["bench.py", "--gpus", "1", "--layers", "2", "--steps", "5", "--warmup", "2", "--prompt-len", "256", "--dump-outputs", str(d_out)], {})
        d = json.loads([l for l in out.splitlines() if l.strip()][-1])
        assert d["steps"] == 5 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "bf16"
        assert d["unit"] == "tokens/s" and d["higher_is_better"] is True and "metric" in d
        assert not {"roofline", "cpu_baseline", "spread", "plain_decode", "mid_regime", "hot_regime", "via_generate", "projections"} & set(d)
        arrays = {n: np.load(d_out / f"{n}.npy") for n in ("timed_tokens", "last_step_accepted", "last_step_record")}
        assert all(a.dtype == np.float64 for a in arrays.values())
        assert len(arrays["timed_tokens"]) == round(d["step_compression"] * 5) and len(arrays["last_step_accepted"]) >= 1
        assert list(arrays["timed_tokens"][-len(arrays["last_step_accepted"]):]) == list(arrays["last_step_accepted"])
        outs.append(arrays)
    for n in outs[0]:
        assert np.array_equal(outs[0][n], outs[1][n]), n
