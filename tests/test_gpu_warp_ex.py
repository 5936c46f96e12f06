"""GPU: lade_warp_rows_ex - HF's min-p, typical, epsilon and eta warpers behind temperature / top-k / top-p in one launch - against HF's
own classes on the fp64 copy of the rows (tests/warp_ref.py states the yardstick and the rule a row is held to)."""
import pytest
import torch

from warp_ref import NO_OP, STAGES, check_stage, hf64, ties_whole

pytestmark = pytest.mark.gpu

CELLS = [(s, v) for s, vals in (("min_p", (0.05, 0.3, 1.0)), ("typical_p", (0.2, 0.9, 0.95)), ("epsilon_cutoff", (3e-4, 0.5)),
                                ("eta_cutoff", (3e-4, 4e-3, 0.5))) for v in vals]
ALL_FOUR = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=4e-3)
MAX_DIFFERING = 0.05            # share of compared rows whose -inf pattern may differ from the yardstick (by the one admissible token each)


def _ex(logits, rows, skip, t=1.0, k=0, p=1.0, **stages):
    from lookaheaddecoding_amd import ops
    return ops.warp_rows(logits.cuda(), rows, skip, t, k, p, **dict(NO_OP, **stages)).cpu()


def _upto(stage):
    """the later-stage settings of ALL_FOUR up to and including `stage`"""
    return {s: ALL_FOUR[s] for s in STAGES[:STAGES.index(stage) + 1]}


@pytest.fixture(scope="module")
def inputs():
    """V -> (physical logits [12 + 3, V], logical rows [12, V]): 6 rows of randn * 3 and 6 flat ones (randn * 0.3: thousands of survivors),
    the out row, three window rows to skip, the rest"""
    g = torch.Generator().manual_seed(0)
    out = {}
    for V in (5, 257, 32000, 32769, 128256):
        pick = torch.cat([torch.randn(6, V, generator=g) * 3.0, torch.randn(6, V, generator=g) * 0.3])
        out[V] = (torch.cat([pick[:1], torch.full((3, V), 1e4), pick[1:]]), pick)
    return out


def test_each_stage_equals_hf_in_fp64(inputs):
    compared = differing = 0
    for V, (phys, pick) in inputs.items():
        for stage, value in CELLS:
            got = _ex(phys, 12, 3, **{stage: value})
            differing += check_stage(stage, pick, got, hf64(stage, value, pick), (V, stage, value))
            compared += 12
        # all four behind temperature, top-k and top-p: every stage against its own yardstick on the device's rows of the stages before it
        prev = _ex(phys, 12, 3, 0.7, 50, 0.95)
        for stage in STAGES:
            got = _ex(phys, 12, 3, 0.7, 50, 0.95, **_upto(stage))
            differing += check_stage(stage, prev, got, hf64(stage, ALL_FOUR[stage], prev), (V, "all four", stage))
            compared += 12
            prev = got
    print(f"rows compared {compared}, differing from HF in fp64 by their one boundary token {differing}")
    assert differing <= MAX_DIFFERING * compared, (differing, compared)


def test_no_op_values_run_the_kernels_of_the_three_warpers():
    from lookaheaddecoding_amd import ops
    g = torch.Generator().manual_seed(0)
    for V in (32000, 32016, 257, 5, 128256, 50257, 32769):
        logits = (torch.randn(9, V, generator=g) * 3.0).cuda()
        for (temp, k, p) in ((1.0, 0, 0.9), (0.7, 50, 1.0), (0.8, 40, 0.95), (1.3, 0, 0.5), (1.0, 1, 1.0), (1.0, V + 5, 0.999), (0.6, 7, 0.3), (1.0, 0, 1e-6)):
            old = ops.warp_rows(logits, 6, 3, temp, k, p)
            new = ops._warp_rows_ex(logits, 6, 3, temp, k, p, **NO_OP)
            assert torch.equal(old, new), (V, temp, k, p)


def test_ties_stay_or_go_whole():
    """bf16-granular values (thousands of equal values per row) as bf16 / f16 / fp32 inputs"""
    g = torch.Generator().manual_seed(1)
    compared = differing = 0
    for V in (32000, 128256):
        base = torch.randn(6, V, generator=g) * 2.5
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            lg = base.to(torch.bfloat16).to(dt)
            prev = lg.float()
            for stage, value in CELLS:
                got = _ex(lg, 6, 0, **{stage: value})
                assert ties_whole(prev, got), (V, dt, stage, value)
                differing += check_stage(stage, prev, got, hf64(stage, value, prev), (V, dt, stage, value))
                compared += 6
    assert differing <= MAX_DIFFERING * compared, (differing, compared)


def test_degenerate_rows():
    g = torch.Generator().manual_seed(2)
    every = [(s, v) for s, v in CELLS] + [("min_p", 1.0)]
    for flat in (torch.zeros(2, 1000), torch.zeros(1, 40000), torch.full((1, 1), 0.3)):      # all equal (and V = 1): every stage keeps everything
        for stage, value in every:
            assert torch.equal(_ex(flat, flat.shape[0], 0, **{stage: value}), flat), (flat.shape, stage, value)
        assert torch.equal(_ex(flat, flat.shape[0], 0, **ALL_FOUR), flat)
    for V in (1000, 40000):                                       # one dominant token, min_p = 1: it alone survives
        row = torch.randn(1, V, generator=g)
        row[0, 7] = 50.0
        got = _ex(row, 1, 0, min_p=1.0)
        assert torch.isfinite(got).nonzero().tolist() == [[0, 7]] and got[0, 7] == 50.0
    compared = differing = 0
    for V in (32000, 40000):                                      # every third entry already -inf
        holes = torch.randn(2, V, generator=g) * 2.0
        holes[:, ::3] = -float("inf")
        for stage, value in CELLS:
            got = _ex(holes, 2, 0, **{stage: value})
            differing += check_stage(stage, holes, got, hf64(stage, value, holes), (V, "holes", stage, value))
            compared += 2
    assert differing <= MAX_DIFFERING * compared, (differing, compared)


def test_a_row_means_the_same_at_every_vocabulary_size():
    """40000 tokens of which those from 32768 on are -inf, against the first 32768 alone: the same kept sets for all four stages.  Both rows
    run the output-row form of the kernel (with a later stage active it runs at every V), so this is no comparison of two kernel forms: it
    pins that the cuts do not depend on V, on the 16-byte grouping (both sizes are multiples of 4) or on -inf padding behind the row."""
    g = torch.Generator().manual_seed(3)
    short = torch.cat([torch.randn(2, 32768, generator=g) * 3.0, torch.randn(2, 32768, generator=g) * 0.3])
    long = torch.cat([short, torch.full((4, 40000 - 32768), -float("inf"))], dim=1)
    for stages in [{s: v} for s, v in CELLS] + [ALL_FOUR]:
        a, b = _ex(short, 4, 0, **stages), _ex(long, 4, 0, **stages)
        assert torch.equal(a, b[:, :32768]) and not torch.isfinite(b[:, 32768:]).any(), stages
        a, b = _ex(short, 4, 0, 0.7, 50, 0.95, **stages), _ex(long, 4, 0, 0.7, 50, 0.95, **stages)
        assert torch.equal(a, b[:, :32768]), stages


def test_the_same_launch_twice_gives_the_same_bits(inputs):
    for V in (32000, 128256):
        phys = inputs[V][0].cuda()
        a = _ex(phys, 12, 3, 0.7, 50, 0.95, **ALL_FOUR)
        assert torch.equal(a, _ex(phys, 12, 3, 0.7, 50, 0.95, **ALL_FOUR))
        a = _ex(phys, 12, 3, typical_p=0.9, eta_cutoff=4e-3)
        assert torch.equal(a, _ex(phys, 12, 3, typical_p=0.9, eta_cutoff=4e-3))
