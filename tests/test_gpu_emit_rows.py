"""GPU: lade_emit_init / lade_emit_rows alone - the rows that decided a step's tokens, appended to the scores / logits buffers.
Every comparison is bit-exact against raw[row].float() and proc[row] taken with torch indexing: token 0 of a step from the out row, token
k >= 1 from position k-1 of the accepted candidate c (raw row 1 + n_inp + c*gs + k-1, processed row 1 + c*gs + k-1)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_INP, G = 5, 3            # window rows between the out row and the candidate rows; candidates in the step


def _step(V, ld, dtype, gs, seed=0):
    """raw [1 + N_INP + G*gs][V] as a column slice of a [.., ld] buffer in `dtype`, proc [1 + G*gs][V] fp32"""
    g = torch.Generator().manual_seed(seed + V + gs)
    raw = (torch.randn(1 + N_INP + G * gs, ld, generator=g) * 4.0).to(dtype).cuda()[:, :V]
    proc = torch.randn(1 + G * gs, V, generator=g).cuda()
    return raw, proc


def _desc(scores, logits, V):
    from lookaheaddecoding_amd import cabi, ops
    desc = torch.full((cabi.EMIT_WORDS,), -1, dtype=torch.int64, device="cuda")
    ops.emit_init(desc, scores, logits, V)
    return desc


def _ctl(n, c):
    from lookaheaddecoding_amd import cabi
    ctl = torch.zeros(cabi.CTL_WORDS, dtype=torch.int32, device="cuda")
    ctl[cabi.CTL_N_ACCEPT] = n
    ctl[cabi.CTL_MAX_HIT_IDX] = c
    ctl[cabi.CTL_MAX_HIT] = n - 1
    return ctl


def _count(desc):
    from lookaheaddecoding_amd import cabi
    return int(desc[cabi.EMIT_COUNT].item())


def _src_rows(n, c, gs):
    """(raw row, processed row) of each of the n tokens"""
    return [(0, 0)] + [(1 + N_INP + c * gs + k - 1, 1 + c * gs + k - 1) for k in range(1, n)]


CANARY = -12345.5


def _run_all(V, ld, dtype, gs):
    from lookaheaddecoding_amd import ops
    raw, proc = _step(V, ld, dtype, gs)
    launches = [(mode, n, c) for mode in ("ctl", "idx") for n in (1, 2, gs + 1) for c in (0, G - 1)]
    total = sum(n for _, n, _ in launches)
    scores = torch.full((total + 2, V), CANARY, dtype=torch.float32, device="cuda")
    logits = torch.full((total + 2, V), CANARY, dtype=torch.float32, device="cuda")
    desc = _desc(scores, logits, V)
    assert _count(desc) == 0
    want = []
    for mode, n, c in launches:
        if mode == "ctl":
            ops.emit_rows(desc, raw, N_INP, gs, proc=proc, ctl=_ctl(n, c))
        else:
            ops.emit_rows(desc, raw, N_INP, gs, proc=proc, idx=[0] + [c] * (n - 1))
        want += _src_rows(n, c, gs)
    assert _count(desc) == total == len(want)
    rr = torch.tensor([r for r, _ in want], device="cuda")
    pr = torch.tensor([p for _, p in want], device="cuda")
    what = (V, ld, str(dtype), gs)
    assert torch.equal(logits[:total], raw[rr].float()), what
    assert torch.equal(scores[:total], proc[pr]), what
    assert bool((scores[total:] == CANARY).all()) and bool((logits[total:] == CANARY).all()), what


@pytest.mark.parametrize("gs", [2, 4])
@pytest.mark.parametrize("V,ld", [(257, 264), (32000, 32000)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_emitted_rows_equal_torch_indexing(dtype, V, ld, gs):
    """accepted counts 1, 2 and gs + 1, through the control block and through idx, candidate 0 and the last one; V = 257 in rows of 264
    takes the odd tail, a row stride that is not V and destination rows off the 16-byte grid (the scalar form)"""
    _run_all(V, ld, dtype, gs)


def test_emitted_rows_at_the_qwen_vocabulary():
    _run_all(152064, 152064, torch.bfloat16, 4)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_without_processed_rows_scores_equal_logits(dtype):
    from lookaheaddecoding_amd import ops
    V, gs = 1000, 4
    raw, _ = _step(V, V + 8, dtype, gs)
    scores = torch.full((gs + 1, V), CANARY, dtype=torch.float32, device="cuda")
    logits = torch.full((gs + 1, V), CANARY, dtype=torch.float32, device="cuda")
    desc = _desc(scores, logits, V)
    ops.emit_rows(desc, raw, N_INP, gs, proc=None, ctl=_ctl(gs + 1, 1))
    assert _count(desc) == gs + 1
    rr = torch.tensor([r for r, _ in _src_rows(gs + 1, 1, gs)], device="cuda")
    assert torch.equal(logits, raw[rr].float()) and torch.equal(scores, logits)


def test_counter_advances_across_launches_and_a_new_run_rewinds_it():
    from lookaheaddecoding_amd import ops
    V, gs = 257, 4
    raw, proc = _step(V, 264, torch.bfloat16, gs)
    scores = torch.full((16, V), CANARY, dtype=torch.float32, device="cuda")
    logits = torch.full((16, V), CANARY, dtype=torch.float32, device="cuda")
    desc = _desc(scores, logits, V)
    plan = [(3, 2), (1, 0), (5, 1)]
    for n, c in plan:                              # no synchronisation between the launches: ordered on the stream alone
        ops.emit_rows(desc, raw, N_INP, gs, proc=proc, ctl=_ctl(n, c))
    assert _count(desc) == 9
    want = [rp for n, c in plan for rp in _src_rows(n, c, gs)]
    rr = torch.tensor([r for r, _ in want], device="cuda")
    pr = torch.tensor([p for _, p in want], device="cuda")
    assert torch.equal(logits[:9], raw[rr].float()) and torch.equal(scores[:9], proc[pr])
    assert bool((logits[9:] == CANARY).all())
    # a new generate() call rewrites the SAME descriptor in place: other buffers, counter 0
    scores2 = torch.full((4, V), CANARY, dtype=torch.float32, device="cuda")
    ops.emit_init(desc, scores2, None, V)
    assert _count(desc) == 0
    ops.emit_rows(desc, raw, N_INP, gs, proc=proc, idx=[0, 2])
    assert _count(desc) == 2
    assert torch.equal(scores2[0], proc[0]) and torch.equal(scores2[1], proc[1 + 2 * gs]) and bool((scores2[2:] == CANARY).all())
    assert bool((logits[9:] == CANARY).all()) and torch.equal(logits[:9], raw[rr].float()), "the buffers of the earlier run are no longer written"


@pytest.mark.parametrize("mode", ["ctl", "idx"])
def test_rows_beyond_the_capacity_are_not_written_and_the_counter_shows_it(mode):
    from lookaheaddecoding_amd import ops
    V, gs, cap = 257, 4, 4
    raw, proc = _step(V, 264, torch.float16, gs)
    # the descriptor's buffers are the first `cap` rows of larger allocations: whatever lands behind them is an out-of-capacity write
    big_s = torch.full((cap + 8, V), CANARY, dtype=torch.float32, device="cuda")
    big_l = torch.full((cap + 8, V), CANARY, dtype=torch.float32, device="cuda")
    desc = _desc(big_s[:cap], big_l[:cap], V)

    def launch(n, c):
        if mode == "ctl":
            ops.emit_rows(desc, raw, N_INP, gs, proc=proc, ctl=_ctl(n, c))
        else:
            ops.emit_rows(desc, raw, N_INP, gs, proc=proc, idx=[0] + [c] * (n - 1))

    launch(3, 1)
    launch(gs + 1, 2)                              # rows 3 .. 7: only row 3 fits
    launch(2, 0)                                   # entirely beyond
    assert _count(desc) == 3 + gs + 1 + 2 > cap
    want = _src_rows(3, 1, gs) + _src_rows(gs + 1, 2, gs)[:1]
    rr = torch.tensor([r for r, _ in want], device="cuda")
    pr = torch.tensor([p for _, p in want], device="cuda")
    assert torch.equal(big_l[:cap], raw[rr].float()) and torch.equal(big_s[:cap], proc[pr])
    assert bool((big_l[cap:] == CANARY).all()) and bool((big_s[cap:] == CANARY).all())


@pytest.mark.parametrize("which", ["scores", "logits"])
def test_a_null_destination_is_not_touched(which):
    from lookaheaddecoding_amd import ops
    V, gs = 32000, 2
    raw, proc = _step(V, V, torch.bfloat16, gs)
    # one allocation: the requested field's buffer in front, canary rows behind it where a second buffer might be assumed
    both = torch.full((2 * (gs + 1), V), CANARY, dtype=torch.float32, device="cuda")
    dst = both[:gs + 1]
    desc = _desc(dst if which == "scores" else None, dst if which == "logits" else None, V)
    ops.emit_rows(desc, raw, N_INP, gs, proc=proc, ctl=_ctl(gs + 1, G - 1))
    assert _count(desc) == gs + 1
    want = _src_rows(gs + 1, G - 1, gs)
    if which == "scores":
        assert torch.equal(dst, proc[torch.tensor([p for _, p in want], device="cuda")])
    else:
        assert torch.equal(dst, raw[torch.tensor([r for r, _ in want], device="cuda")].float())
    assert bool((both[gs + 1:] == CANARY).all())


def test_an_accepted_count_of_zero_appends_nothing():
    from lookaheaddecoding_amd import ops
    V, gs = 257, 2
    raw, proc = _step(V, 264, torch.float32, gs)
    scores = torch.full((4, V), CANARY, dtype=torch.float32, device="cuda")
    desc = _desc(scores, None, V)
    ops.emit_rows(desc, raw, N_INP, gs, proc=proc, ctl=_ctl(0, 0))
    assert _count(desc) == 0 and bool((scores == CANARY).all())
