"""Lookahead decode loops on the MI355X step engine.

Mirrors the reference's `lade/decoding.py`: `greedy_search_proxy` / `sample_proxy` (:15-34),
`jacobi_greedy_search_multilevel` (:697-1259) and `jacobi_sample_multilevel` (:137-692), with the
same module globals `CONFIG_MAP` / `FUNC_MAP` (:11-12).  What differs is where the work happens:
the window, the n-gram pool, verification, the window roll and the KV commit live on the GPU
(`liblade_hip.so`); the host loop only launches a step, reads back one small record
(`max_hit`, accepted tokens, next candidate count) and applies the stopping criteria.
"""
from __future__ import annotations

import os
import random
import sys
import time
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Sequence

import torch

from . import cabi, ops
from .cabi import (CTL_FILL_LEVEL, CTL_G, CTL_HITS, CTL_LST_POS, CTL_LST_TOKEN, CTL_N_INPUT, CTL_P, CTL_WLEN, CTL_WORDS,
                   REC_WORDS, call, ptr, record_seal)
from .engine import StepEngine, _on_device
from .ops import StepMask

FUNC_MAP: dict = {}
CONFIG_MAP: dict = {}
COLOR_PRINT = int(os.environ.get("COLOR_PRINT", 0))


@dataclass(frozen=True)
class GenControls:
    """HF's RepetitionPenaltyLogitsProcessor and min-length family as the device step applies them (include/lade_hip.h, "generation
    controls").  penalty: HF's `repetition_penalty` (1.0 = off).  min_len: absolute minimum sequence length, `min_length` or prompt length
    + `min_new_tokens` (0 = off).  min_len_eos: the ids masked while a row is shorter than min_len (None: the stopping EOS set).
    Token constraints (include/lade_hip.h, "token constraints"; HF's suppress_tokens / begin_suppress_tokens / sequence_bias /
    bad_words_ids).  ban: ids that are -inf on every row.  begin_ban / begin_index: ids that are -inf on a row whose input length equals
    begin_index.  sequence_bias: ((t_0, .., t_{n-1}), bias) entries in the order of HF's dict, bias finite or -inf (a banned word of
    more than one token is a -inf entry; a single banned token belongs in `ban`).  add_bias: a SequenceBias / NoBadWords processor is
    present, so every score passes through HF's `scores + bias` (implied by a non-empty sequence_bias)."""
    penalty: float = 1.0
    min_len: int = 0
    min_len_eos: Optional[tuple] = None
    ban: tuple = ()
    begin_ban: tuple = ()
    begin_index: int = -1
    sequence_bias: tuple = ()
    add_bias: bool = False

    def __post_init__(self):
        if len(self.sequence_bias) > cabi.GEN_MAX_SEQ:
            raise cabi.LadeHipError(f"{len(self.sequence_bias)} sequence_bias / bad_words_ids entries: the device step takes at most "
                                    f"{cabi.GEN_MAX_SEQ} (LADE_GEN_MAX_SEQ; single banned tokens do not count)")
        for seq, bias in self.sequence_bias:
            if not 1 <= len(seq) <= cabi.GEN_MAX_SEQ_LEN:
                raise cabi.LadeHipError(f"a sequence_bias / bad_words_ids entry of {len(seq)} tokens: the device step takes 1 to "
                                        f"{cabi.GEN_MAX_SEQ_LEN} (LADE_GEN_MAX_SEQ_LEN)")
            if bias != bias or bias == float("inf"):
                raise cabi.LadeHipError(f"sequence_bias {tuple(seq)} -> {bias}: a bias is finite or -inf")
        if self.begin_ban and self.begin_index < 0:
            raise cabi.LadeHipError(f"begin_suppress_tokens with begin_index={self.begin_index}")

    @property
    def constrained(self) -> bool:
        return bool(self.ban or self.begin_ban or self.sequence_bias or self.add_bias)

    @property
    def active(self) -> bool:
        return self.penalty != 1.0 or self.min_len > 0 or self.constrained


def eos_set(eos_token_id) -> tuple:
    """EOS ids as a tuple in first-seen order: None -> (), an int, a sequence or a tensor of ints -> their distinct non-negative ids
    (at most cabi.GEN_MAX_EOS)"""
    if eos_token_id is None:
        return ()
    if hasattr(eos_token_id, "tolist"):
        eos_token_id = eos_token_id.tolist()
    if isinstance(eos_token_id, (list, tuple)):
        ids = []
        for t in eos_token_id:
            if t is not None and int(t) >= 0 and int(t) not in ids:
                ids.append(int(t))
    else:
        ids = [int(eos_token_id)] if int(eos_token_id) >= 0 else []
    if len(ids) > cabi.GEN_MAX_EOS:
        raise cabi.LadeHipError(f"{len(ids)} EOS ids: the device step takes at most {cabi.GEN_MAX_EOS}")
    return tuple(ids)


@dataclass
class GenOut:
    tokens: List[int]            # prompt + generated, trimmed to max_length like the reference (:1221-1229)
    steps: int
    generated: int
    trace: List[dict] = field(default_factory=list)
    scores: Optional[torch.Tensor] = None      # emit request only: [generated, V] fp32 device rows, HF's `scores` (processed / warped)
    logits: Optional[torch.Tensor] = None      # ... and HF's `logits` (the model's rows, widened to fp32)


EMIT_FIELDS = ("scores", "logits")
LP_EMIT_REFUSAL = ("lookahead parallelism (DIST_WORKERS > 1 / FORCE_LP) does not implement return_dict_in_generate with output_scores / "
                   "output_logits: its verify runs inside lade_lp_reduce_apply, which keeps no rows; run on one GPU without FORCE_LP")


def emit_request(emit) -> Optional[tuple]:
    """An emit request in canonical form: None (off), or the requested subset of EMIT_FIELDS in that order"""
    if not emit:
        return None
    if isinstance(emit, str):
        emit = (emit,)
    unknown = [f for f in emit if f not in EMIT_FIELDS]
    if unknown:
        raise cabi.LadeHipError(f"emit={tuple(emit)!r}: unknown field {unknown[0]!r} (one or both of {EMIT_FIELDS})")
    return tuple(f for f in EMIT_FIELDS if f in emit) or None


def emit_capacity(max_length: int, n_prompt: int, gs: int) -> int:
    """rows of a run's emit buffers: every token up to max_length, plus what the last step may emit beyond it"""
    return max(int(max_length) - int(n_prompt), 0) + int(gs)


# ---- the shape of one decode step: plain host arithmetic, shared by the single-GPU decoder and lookahead parallelism -------------
def level_sizes(W: int, N: int, fill_level: int) -> List[int]:
    """Lengths of window levels 0..fill_level before the step with that fill level
    (init W+N-3 at lade/decoding.py:902; each fill step trims one: :1040, :1050-1051)."""
    if fill_level == 0:
        return [W + N - 3]
    if fill_level >= N - 2:
        return [W - 1] + [W] * (N - 2)
    return [W + N - 3 - fill_level] + [W + N - 2 - fill_level] * fill_level


class StepShape(NamedTuple):
    """What one step feeds: n_input re-fed tokens | the window levels | cand_rows candidate tokens.  phase: 0 prefill, 1 fill, 2 steady.
    (A tuple: the lookahead-parallel loop builds one per step between a synchronise and the next launch.)"""
    phase: int
    n_input: int
    level_sizes: tuple
    cand_rows: int

    @property
    def T(self) -> int:
        return self.n_input + sum(self.level_sizes) + self.cand_rows

    @property
    def n_inp(self) -> int:
        return self.level_sizes[-1]

    def rows(self) -> List[int]:
        """rows whose logits are needed: out row, last level's rows, candidate rows (:1578-1606)"""
        T = self.T
        return [self.n_input - 1] + list(range(T - self.cand_rows - self.n_inp, T))


def step_shape(W: int, N: int, step: int, g: int, n_input: int = 1) -> StepShape:
    """Shape of step number `step` of a run (0 = prefill, n_input = prompt length; then one fill step per level until fill level
    N-2, steady from there on) that carries g candidates of N-1 tokens - only a steady step verifies candidates."""
    fill_level = min(step, N - 2)
    phase = 0 if step == 0 else (2 if fill_level >= N - 2 else 1)
    return StepShape(phase, n_input, tuple(level_sizes(W, N, fill_level)), g * (N - 1) if phase == 2 else 0)


def capture_step_graph(body, state: Sequence[torch.Tensor], **graph_kw):
    """`body` as a hipGraph: one warm-up run on a side stream (library handles, allocator, autotune), then the integer `state` it
    advanced is restored - also when the warm-up failed -, then the capture.  The K/V rows the warm-up wrote lie at >= P and are
    rewritten by the real step before being read.  Returns (graph, what body returned under capture)."""
    saved = [t.clone() for t in state]
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    finally:
        for t, sv in zip(state, saved):
            t.copy_(sv)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, **graph_kw):
        out = body()
    return g, out


def generate_loop(run, step, max_length: int, keep_trace: bool, on_step, log: bool) -> GenOut:
    """step() until EOS or max_length (stopping criteria, lade/decoding.py:1204-1219) on a started `run` (tokens / prompt / steps /
    finished_by_eos: a LookaheadDecoder or a parallel.LPRunner).  on_step gets each step's accepted tokens, trimmed to max_length."""
    trace: List[dict] = []
    while True:
        info = step()
        if keep_trace:
            trace.append(info)
        if on_step is not None:
            on_step(info["accepted"][:max(0, max_length - (len(run.tokens) - len(info["accepted"])))])
        if run.finished_by_eos or len(run.tokens) >= max_length:
            break
    generated = min(len(run.tokens), max_length) - len(run.prompt)
    if log and CONFIG_MAP.get("DEBUG", 0):
        CONFIG_MAP.setdefault("log", []).append([generated, run.steps, round(generated / max(run.steps, 1), 2)])
    return GenOut(tokens=run.tokens[:max_length], steps=run.steps, generated=generated, trace=trace)


class LadeState:
    """Device-resident integer state of one sequence: window [N-1][wcap], pool [V][G][gs], control block."""

    def __init__(self, V: int, W: int, N: int, G: int, device, max_T: int):
        if not (3 <= N <= cabi.MAX_LEVEL):
            raise cabi.LadeHipError(f"LEVEL={N} unsupported (3..{cabi.MAX_LEVEL}; the reference itself needs LEVEL >= 3)")
        if not (0 <= G <= cabi.MAX_GUESS_SET):
            raise cabi.LadeHipError(f"GUESS_SET_SIZE={G} unsupported (0..{cabi.MAX_GUESS_SET}; <= 0 means no verification branch)")
        if W < 1 or W + N - 3 > cabi.MAX_WINDOW:
            raise cabi.LadeHipError(f"WINDOW_SIZE={W} unsupported")
        self.V, self.W, self.N, self.G, self.gs = V, W, N, G, N - 1
        self.wcap = W + N - 3
        i32 = dict(dtype=torch.int32, device=device)
        self.window = torch.zeros(N - 1, self.wcap, **i32)
        self.ctl = torch.zeros(CTL_WORDS, **i32)
        self.pool_tok = torch.zeros(V, max(G, 1), self.gs, **i32)
        self.pool_cnt = torch.zeros(V, **i32)
        self.guess = torch.zeros(max(G, 1) * self.gs, **i32)
        self.tail = torch.zeros(N + 2, **i32)
        self.ids = torch.zeros(max_T, **i32)
        self.pos = torch.zeros(max_T, **i32)
        self.sel = torch.zeros(1 + self.wcap + G * self.gs, **i32)
        self.am = torch.zeros(1 + self.wcap + G * self.gs, **i32)
        self.record = torch.zeros(REC_WORDS, **i32)
        self.record_host = torch.zeros(REC_WORDS, dtype=torch.int32).pin_memory()
        self.record_host_np = self.record_host.numpy()          # the same pinned bytes, for the polling read (poll_record)
        self.device = device

    def reset(self, window0: Sequence[int], n_prompt: int, prompt_tail: Sequence[int]) -> None:
        N = self.N
        ctl = [0] * CTL_WORDS
        ctl[CTL_N_INPUT] = n_prompt
        ctl[CTL_LST_POS] = n_prompt - 1
        ctl[CTL_WLEN] = len(window0)
        self.ctl.copy_(torch.tensor(ctl, dtype=torch.int32))
        self.window.zero_()
        self.window[0, :len(window0)] = torch.tensor(list(window0), dtype=torch.int32)
        self.pool_cnt.zero_()
        t = list(prompt_tail)[-N:]
        self.tail.copy_(torch.tensor([len(t)] + t + [0] * (N + 1 - len(t)), dtype=torch.int32))

    def read_record(self) -> List[int]:
        self.record_host.copy_(self.record, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self.record_host.tolist()

    POLL_TIMEOUT_S = float(os.environ.get("LADE_POLL_TIMEOUT_MS", "250")) * 1e-3
    POLL_READS_PER_YIELD = max(1, int(cabi.debug("poll_reads_per_yield", "256")))

    def poll_record(self, step_no: int, timeout_s: Optional[float] = None) -> Optional[List[int]]:
        """The record of step `step_no` as `lade_greedy_post_step` stored it into the pinned host buffer (mapped into the device: no
        copy node, no stream synchronisation).  The host spins on the buffer until the record carries that step number and its seal
        (`lade_record_seal` over the other words) matches what was read - a stale or half-landed record fails one of the two; the seal is
        the ONLY ordering guarantee (the kernel issues no system-scope fence behind the stores).
        The spin is bounded by WALL-CLOCK time (LADE_POLL_TIMEOUT_MS, default 250 ms - far beyond any step) and yields the GIL every 256
        reads, so that a streamer thread or lookahead-parallel rank threads of this process are not starved while this one waits.  None
        when the record does not arrive in time - e.g. pinned memory the device's stores do not reach coherently (HIP_HOST_COHERENT=0);
        the caller then synchronises the stream, reads the record the slow way and STOPS polling for good (LookaheadDecoder._polled_record)."""
        buf = self.record_host_np
        deadline = time.monotonic() + (self.POLL_TIMEOUT_S if timeout_s is None else timeout_s)
        while True:
            for _ in range(self.POLL_READS_PER_YIELD):
                if buf[7] == step_no:
                    rec = buf.tolist()
                    if rec[7] == step_no and (rec[REC_WORDS - 1] & 0xFFFFFFFF) == record_seal(rec, step_no):
                        return rec
            if time.monotonic() > deadline:
                return None
            time.sleep(0)                      # release the GIL: other threads of the process get to run


DRAW_WITH_TORCH = cabi.debug("draw_torch") == "1"


class LookaheadDecoder:
    """Greedy / sampling lookahead decoding of one sequence on a `StepEngine`."""

    def __init__(self, engine: StepEngine, W: int, N: int, G: int, pool_from_prompt: bool = False, lp=None, use_graph: bool = False):
        self.e = engine
        self.use_graph = bool(use_graph)
        # GUESS_SET_SIZE <= 0 (-1 = "unlimited" in the reference's README): both reference loops gate the verification
        # branch on `GUESS_SET_SIZE > 0` (lade/decoding.py:402, :948), so the pool is filled but never read and every
        # step accepts exactly one token.  Reproduced as G = 0: no pool, no candidates.
        G = max(int(G), 0)
        self.W, self.N, self.G, self.gs = W, N, G, N - 1
        self.pool_from_prompt = bool(pool_from_prompt)
        self.lp = lp                      # lookahead-parallel context (parallel.LPContext) or None
        self.poll = os.environ.get("LADE_POLL", "1") != "0"       # steady hipGraph steps: poll the host-mapped record instead of synchronising
        self._step_no = 0                 # device step counter (ctl[STEP]) as of the last record read
        self.device = engine.device
        self.st = LadeState(engine.V, W, N, G, engine.device, engine.max_T)
        if self.max_step_tokens() > engine.max_T:
            raise cabi.LadeHipError(f"W={W} N={N} G={G} needs {self.max_step_tokens()} tokens per step > engine.max_T={engine.max_T}")
        # host state of the current run (start / sample_start)
        self.prompt, self.window0, self.tokens = [], [], []
        self.eos_set, self._eos_host, self.controls = (), ops.host_ids(()), None
        self.steps, self.P, self.g, self.fill_level = 0, 0, 0, 0
        self.finished_by_eos = False
        self._s = None                    # the sampling run's warper, RNGs and forced-hits buffers (sample_start)
        # allocated on first use: a decoder that never gets controls / never samples holds neither
        self._gen = None                  # generation-control block (start)
        self._cons = None                 # token-constraint block, attached to _gen by its address (start)
        self._smp = None                  # pinned and device sampling buffers (_sampling_buffers)
        self._draw_warm = False           # the device draw's torch kernels have run once (sample_start)
        # per-token scores / logits (start(emit=...)): the request, the run's buffers, the device descriptor the captured steps read
        # (allocated once: its ADDRESS is baked into the graphs, its contents are rewritten per run), the rows of the last model step
        self.emit, self._emit_bufs, self._emit_desc, self._emit_src = None, {}, None, None
        self._sel_cache = {}              # device copies of the eager steps' logits-row selections (_set_sel)
        # captured steady steps, per candidate bucket (_capture_graphs); _graph_key: what they were captured for (_graph_key_for)
        self._graphs, self._graph_sel, self._graph_splits, self._graph_T, self._graph_logits, self._graph_src = {}, {}, {}, {}, {}, {}
        self._graph_key = None
        # every kernel decision the steady steps of this configuration need (GEMM shapes, the in-step pass, the attention launch
        # parameters) is taken NOW, not inside the first live step of each row class (a multi-second stall for that request)
        if lp is None and os.environ.get("LADE_PREPARE", "1") != "0":
            engine.prepare(sorted({(N - 1) * (W + b) for b in self._buckets()}))

    def max_step_tokens(self) -> int:
        return self.gs + (self.N - 1) * self.W + self.G * self.gs

    # ---- helpers --------------------------------------------------------------------------------
    def _set_sel(self, rows: List[int]) -> int:
        """Device copy of the logits-row selection.  The selections of a run are a handful of shapes (one per phase / candidate
        count), so each is uploaded once and kept: a steady eager step issues no host-to-device copy for it."""
        key = (rows[0], rows[1] if len(rows) > 1 else -1, len(rows), rows[-1])
        cache = self._sel_cache
        t = cache.get(key)
        if t is None:
            if len(cache) > 256:
                cache.clear()
            t = cache[key] = torch.tensor(rows, dtype=torch.int32, device=self.e.device)
        self.st.sel[:len(rows)].copy_(t, non_blocking=True)
        return len(rows)

    # ---- stepwise API (bench.py drives single steps; greedy() is start + step until done) ----------
    @torch.no_grad()
    @_on_device
    def start(self, prompt: Sequence[int], eos_token_id=None, rng: Optional[random.Random] = None,
              controls: Optional[GenControls] = None, emit=None, emit_cap: int = 0) -> None:
        """eos_token_id: an int, a sequence of ints or None.  controls: GenControls (repetition penalty / min length / token constraints) or None; with None,
        at most one EOS id and no emit request a step launches exactly the kernels of the plain step.
        emit: None, or one or both of "scores" / "logits": every step appends the fp32 rows that decided its tokens to per-run buffers of
        emit_cap rows (emit_capacity); emitted() returns them."""
        e, st = self.e, self.st
        W, N, G, gs = self.W, self.N, self.G, self.gs
        rng = rng if rng is not None else random
        self.prompt = [int(t) for t in prompt]
        # window init: W+N-3 random prompt tokens (lade/decoding.py:887-902, `copy_from`)
        self.window0 = [rng.choice(self.prompt) for _ in range(W + N - 3)]
        e.reset()
        st.reset(self.window0, len(self.prompt), self.prompt)
        if self.pool_from_prompt:                                   # :915-916
            pt = torch.tensor(self.prompt, dtype=torch.int32, device=e.device)
            call("lade_pool_fill_prompt", ptr(st.pool_tok), ptr(st.pool_cnt), st.V, G, gs, ptr(pt), len(self.prompt))
        self.eos_set = eos_set(eos_token_id)
        self._eos_host = ops.host_ids(self.eos_set)            # what every post-step of the run passes: built once, not per step
        self.controls = controls if controls is not None and controls.active else None
        if self.controls is not None:
            if self._gen is None:
                self._gen = torch.zeros(cabi.gen_words(st.V), dtype=torch.int32, device=e.device)
            c = self.controls
            mask_eos = self.eos_set if c.min_len_eos is None else eos_set(c.min_len_eos)
            prompt_d = torch.tensor(self.prompt, dtype=torch.int32, device=e.device)
            ops.gen_ctl_init(self._gen, st.V, c.penalty, c.min_len if mask_eos else 0, mask_eos, prompt_d)      # (detaches the last run's constraints)
            if c.constrained:               # rewritten in place per sequence: the captured steps find it through _gen
                if self._cons is None:
                    self._cons = torch.zeros(cabi.gen_cons_words(st.V), dtype=torch.int32, device=e.device)
                ops.gen_constraints_init(self._gen, self._cons, st.V, c.ban, c.begin_ban, c.begin_index, c.sequence_bias, c.add_bias, prompt_d)
        self.emit, self._emit_bufs, self._emit_src = emit_request(emit), {}, None
        if self.emit is not None:
            if self._emit_desc is None:
                self._emit_desc = torch.zeros(cabi.EMIT_WORDS, dtype=torch.int64, device=e.device)
            self._emit_bufs = {f: torch.empty(max(int(emit_cap), 1), st.V, dtype=torch.float32, device=e.device) for f in self.emit}
            ops.emit_init(self._emit_desc, self._emit_bufs.get("scores"), self._emit_bufs.get("logits"), st.V)
        self.tokens = list(self.prompt)
        self.steps, self.P, self.g, self.fill_level = 0, 0, 0, 0
        self._step_no = 0                  # st.reset zeroed ctl[STEP]
        self.finished_by_eos = False

    def _emit_step(self, n_inp: int, proc: Optional[torch.Tensor], idx=None) -> None:
        """Appends the rows of the tokens the step has just emitted (lade_emit_rows): behind the post-step, whose ctl words name them
        (greedy, idx None), or with the host verify's candidate per token (sampling).  proc: the rows `scores` are taken from."""
        raw = self._emit_src[0]
        ops.emit_rows(self._emit_desc, raw, n_inp, self.gs, proc=proc if "scores" in self.emit else None, ctl=self.st.ctl, idx=idx)

    def emitted(self, n: int) -> dict:
        """The first n emitted rows of the run per requested field ([n, V] fp32 views of the run's buffers).  Raises when the steps
        appended more rows than the buffers hold, or fewer than n."""
        if self.emit is None:
            return {}
        count = int(self._emit_desc[cabi.EMIT_COUNT].item())
        cap = next(iter(self._emit_bufs.values())).shape[0]
        if count > cap or count < n:
            raise cabi.LadeHipError(f"emit buffers: the steps appended {count} rows, the buffers hold {cap}, {n} tokens were returned")
        return {f: b[:n] for f, b in self._emit_bufs.items()}

    def _with_emitted(self, out: GenOut) -> GenOut:
        rows = self.emitted(out.generated)
        out.scores, out.logits = rows.get("scores"), rows.get("logits")
        return out

    def _post_step(self, am, n_inp: int, T: int, cand_rows: int, phase: int, forced=None, level_override=None, record_host=None) -> None:
        """The fused post-step with the run's EOS set (+ the seen-set update under controls)."""
        st = self.st
        call("lade_greedy_post_step", ptr(st.ctl), ptr(st.window), st.wcap, ptr(st.pool_tok), ptr(st.pool_cnt), st.V, self.W, self.N, self.G, ptr(am), n_inp,
             ptr(st.guess), T, cand_rows, phase, int(self.pool_from_prompt), ptr(st.tail), self._eos_host, len(self.eos_set), ptr(forced),
             ptr(level_override), ptr(st.record), ptr(record_host))
        if self.controls is not None:
            ops.gen_ctl_update(self._gen, st.ctl)

    def _logits_to_am(self, logits: Optional[torch.Tensor], shape: StepShape, pos: torch.Tensor, sel: Optional[torch.Tensor], want_rows: bool,
                      captured: bool = False) -> Optional[torch.Tensor]:
        """The step's argmax ids into st.am.  want_rows (sampling): also returns the fp32 rows the verify reads - logits.float() of every
        selected row (modeling_llama.py:1544), or under generation controls the PROCESSED out row and candidate rows only (lade_gen_rows:
        no window rows between).  logits None: the lm_head GEMM has taken the argmax already."""
        st = self.st
        if self.controls is not None:
            need_rows = want_rows or (self.emit is not None and "scores" in self.emit)      # (emit: the processed rows are HF's `scores`)
            rows_out = torch.empty(1 + shape.cand_rows, st.V, dtype=torch.float32, device=self.e.device) if need_rows else None
            ops.gen_argmax(logits, shape.n_inp, self.gs, self._gen, st.ctl, st.guess, pos, sel, st.am, rows_out)
            self._emit_src = (logits, rows_out)
            return rows_out if want_rows else None
        self._emit_src = (logits, None)
        if logits is None:
            return None
        if want_rows and not captured:                    # (the captured forward-only body converts AFTER the argmax: the order of its launches is kept)
            logits = logits.float()
        ops.argmax_rows(logits, out=st.am)                # window levels are filled by argmax (:459, :545)
        return logits.float() if want_rows else None      # (fp32 already: itself)

    def _model_step(self, shape: StepShape, want_rows: bool, P: int, g: int, sel: Optional[torch.Tensor] = None, c0: int = 0, c1: int = -1,
                    guess: Optional[int] = None, lp=(0, 1), **device_len) -> Optional[torch.Tensor]:
        """The front end of every decode step after the prefill: input assembly, the model over the step's T tokens, argmax ids into
        st.am; returns what _logits_to_am returns.  Eager: P and g (candidates among `guess`) are this step's values.  Captured:
        P = 0, g = -1, the logits rows `sel` of the capture and device_len (dyn_P, n_splits, ntk_pad) - the kernels read cache length
        and candidate count from the control block.  Lookahead parallelism feeds window columns [c0, c1), its share of the guesses
        and, captured, lp = (rank, world).
        Greedy steps take the row argmax inside the lm_head GEMM (argmax_out: the logits are never materialised); the sampling verify
        needs the rows themselves, and under generation controls or an emit request the lm_head materialises them (the argmax reads them
        once, lade_emit_rows copies the deciding ones)."""
        e, st, gs = self.e, self.st, self.gs
        mask = StepMask.from_levels(shape.n_input, shape.level_sizes, shape.cand_rows, gs, P)
        call("lade_build_inputs", None, None, shape.n_input, ptr(st.window), st.wcap, ptr(st.ctl), len(shape.level_sizes) - 1, c0, c1,
             ptr(st.guess) if guess is None else guess, g, gs, shape.cand_rows, ptr(st.ids), ptr(st.pos), None, *lp)
        if sel is None:                  # eager: shape.rows(), cached on the device per shape - no host-to-device copy in a steady step
            sel, n_sel = st.sel, self._set_sel(shape.rows())
        else:
            n_sel = sel.numel()
        logits = e.forward(st.ids, st.pos, mask, sel, n_sel, argmax_out=None if (want_rows or self.controls is not None or self.emit is not None) else st.am,
                           **device_len)
        return self._logits_to_am(logits, shape, st.pos, sel, want_rows, captured=bool(device_len))

    def _eager_model(self, want_rows: bool):
        """The prefill, or an eager decode step, up to the argmax ids in st.am: (shape, T, P_before, rows or None)"""
        e, st = self.e, self.st
        shape = step_shape(self.W, self.N, self.steps, self.g, len(self.prompt) if self.steps == 0 else 1)
        if shape.phase == 0:                                         # prefill: prompt + L0, plain causal
            # rows whose logits are read: the last prompt token and the window (:1578-1606)
            prows = shape.rows()
            logits, done = e.prefill(self.prompt + self.window0, prows)
            pos = torch.tensor(prows, dtype=torch.int32, device=e.device) if self.controls is not None else None      # a prefill feeds token i at position i
            return shape, shape.T - done, done, self._logits_to_am(logits, shape, pos, None, want_rows)
        rows = self._model_step(shape, want_rows, self.P, shape.cand_rows // self.gs)
        return shape, shape.T, self.P, rows

    # ---- steady step as ONE hipGraph ------------------------------------------------------------------
    # Fixed shapes: a graph is captured per candidate-count bucket gcap; a step with g candidates replays the
    # smallest bucket >= g and feeds T = (N-1)(W+gcap) tokens - the gcap-g unused candidate slots are padded
    # with token 0 (they only see themselves and the input token, and verify ignores them).  The cache length
    # P is read by the kernels from the control block (dyn_P), so the same graphs serve every step: a step is
    # one graph launch plus the read-back of the 24-word record.
    # The buckets follow the GEMM row classes of the engine (32-row activation blocks: a step of 61..64 rows
    # costs what one of 60 does, one of 65 pays for 96): bucket = the most candidates that still fit each
    # class (+ G/4).  Config 2 (W=15 N=5 G=15): {0, 1, 4, 9, 15} = 60 / 64 / 76 / 96 / 120 rows - a step that carries ONE
    # candidate (the common case while n-grams are being accepted) runs at the cold step's cost instead of a
    # 76-row step's (+12 %).  Beyond the last class (T > 256: library GEMMs) the old quartiles {0, G/4, G/2, G}.
    def _buckets(self) -> List[int]:
        G, W, n1 = self.G, self.W, self.N - 1
        classes = [c for c in getattr(self.e, "ROW_CLASSES", ()) if c >= n1 * W]
        if not classes or G == 0:
            return sorted({0, (G + 3) // 4, (G + 1) // 2, G})
        fit = {min(G, c // n1 - W) for c in classes}
        # + G/4: inside one GEMM class fewer padded rows still save attention / lm_head / glue rows (live hot regime of config 2:
        # g = 2..4 at 76 rows 4.33 ms, at 96 rows 4.45)
        return sorted({0, (G + 3) // 4, G} | {b for b in fit if b > 0})

    def _bucket_for(self, g: int) -> int:
        fits = [b for b in self._graphs if b >= g]
        if not fits:        # buckets that no longer fit the cache are not captured (_capture_graphs)
            raise cabi.LadeHipError(f"KV cache exhausted: P={self.P}, a step with {g} candidates no longer fits S_max={self.e.S_max}")
        return min(fits)

    def _graph_body(self, shape: StepShape, gcap: int, forward_only: bool):
        """forward_only (sampling): input assembly + model step + argmax; the fp32 logits of the selected rows stay in
        the graph's memory pool for the host-side verify, the post-step is launched afterwards with the forced hits."""
        e, st = self.e, self.st
        rows = self._model_step(shape, forward_only, 0, -1, self._graph_sel[gcap], dyn_P=st.ctl,
                                n_splits=self._graph_splits[gcap],
                                ntk_pad=(st.ctl[CTL_G:CTL_G + 1], gcap, self.gs))      # (dynamic-NTK RoPE only: the padded candidate slots are not sequence length)
        if forward_only:
            return rows
        # LADE_POLL (default on): the post-step stores the sealed record straight into the pinned host buffer and the host polls for it;
        # otherwise a copy node carries it and the host synchronises the stream
        self._post_step(st.am, shape.n_inp, shape.T, shape.cand_rows, 2, record_host=st.record_host if self.poll else None)
        if self.emit is not None:           # which rows: ctl[N_ACCEPT] / ctl[MAX_HIT_IDX] as the post-step left them - no host round trip
            self._emit_step(shape.n_inp, self._emit_src[1])
        ops.kv_commit(e.kv, 0, 0, 0, ctl=st.ctl)
        if not self.poll:
            st.record_host.copy_(st.record, non_blocking=True)

    def _graph_key_for(self, forward_only: bool) -> tuple:
        """What captured graphs depend on: the kind of body, whether it launches the generation controls (their VALUES live in device
        memory: no re-capture), the emit request (the lm_head materialises its logits and the body launches lade_emit_rows; the BUFFERS are
        named by the device descriptor: no re-capture), the engine's generation, and - only for the body that contains the post-step - the
        EOS set."""
        return (forward_only, self.controls is not None, self.emit, self.e.generation, None if forward_only else self.eos_set)

    def _capture_graphs(self, forward_only: bool = False) -> None:
        e, st = self.e, self.st
        self._graphs, self._graph_sel, self._graph_splits, self._graph_T, self._graph_logits, self._graph_src = {}, {}, {}, {}, {}, {}
        state = (st.ctl, st.window, st.pool_cnt, st.pool_tok, st.guess, st.tail) + (() if e.ntk_state is None else (e.ntk_state,))
        if self.controls is not None:
            state += (self._gen,)           # the warm-up's post-step adds its tokens to the seen set
            if self._cons is not None:
                state += (self._cons,)      # ... and shifts them into an attached constraint block's tail
        if self.emit is not None and not forward_only:
            state += (self._emit_desc,)     # ... and its lade_emit_rows advances the row counter (the rows it wrote are overwritten by the real step)
        for gcap in self._buckets():
            shape = StepShape(2, 1, tuple(level_sizes(self.W, self.N, self.N - 2)), gcap * self.gs)
            T = shape.T
            if self.P + T > e.S_max:
                # the warm-up runs the whole step body at the current cache length: a bucket that no longer fits would
                # write its K/V rows past the cache.  Such a bucket can never be replayed either (_replay checks), skip it.
                continue
            self._graph_sel[gcap] = torch.tensor(shape.rows(), dtype=torch.int32, device=e.device)
            self._graph_splits[gcap] = e.n_splits_for(T, min(e.S_max, max(self.P + T, 1024)))
            self._graph_T[gcap] = T
            self._graphs[gcap], self._graph_logits[gcap] = capture_step_graph(lambda: self._graph_body(shape, gcap, forward_only), state)
            self._graph_src[gcap] = self._emit_src          # the captured step's logits (and processed rows) in the graph's memory pool
        torch.cuda.synchronize()
        st.record_host.zero_()              # the warm-up passes left records of the step number the first replay will produce: never mistake one for it
        self._graph_key = self._graph_key_for(forward_only)

    def _replay(self, forward_only: bool):
        """A steady step as one graph launch: (re-)captures when the graphs are not those of _graph_key_for or the cache outgrew the
        captured KV split count, replays the smallest bucket that holds the g candidates.  Returns (T, cand_rows, the body's rows)."""
        e = self.e
        if self._graph_key != self._graph_key_for(forward_only):
            self._capture_graphs(forward_only=forward_only)
        gcap = self._bucket_for(self.g)
        T = self._graph_T[gcap]
        if abs(e.n_splits_for(T, self.P + T) - self._graph_splits[gcap]) >= 2:      # the cache outgrew the captured KV split count
            self._capture_graphs(forward_only=forward_only)
        if self.P + T > e.S_max:
            raise cabi.LadeHipError(f"KV cache exhausted: P={self.P} + T={T} > S_max={e.S_max}")
        self._graphs[gcap].replay()
        self._emit_src = self._graph_src[gcap]
        return T, gcap * self.gs, self._graph_logits[gcap]

    def _polled_record(self) -> List[int]:
        """The record of the step a replayed graph has just launched"""
        st = self.st
        rec = st.poll_record(self._step_no + 1) if self.poll else None
        if rec is None:
            torch.cuda.current_stream().synchronize()
            if self.poll:
                # The spin ran out.  Two different things end here: a step that merely took longer than the time-out (the host was descheduled,
                # a profiler attached, another process held the GPU) - its record IS in the mapped buffer now that the stream has drained,
                # and polling stays on; or memory the device's stores do not reach coherently - the record is still absent after the
                # synchronise: read the device copy and stop polling for good (every later step would pay the same time-out; the graphs are
                # re-captured with the copy node instead of the mapped store).
                rec = st.poll_record(self._step_no + 1, timeout_s=0.0)
                if rec is None:
                    rec = st.read_record()
                    self.poll = False
                    self._graph_key = None
                    print("[lade] the step record did not arrive through the host-mapped buffer (absent even after the stream had drained): "
                          "falling back to stream synchronisation for this decoder", file=sys.stderr, flush=True)
            else:
                rec = st.record_host.tolist()
        return rec

    def _take_record(self, rec: List[int], phase: int) -> dict:
        """A step's record into the host state; returns the fields every step's info carries"""
        self._step_no = rec[7]
        self.steps += 1
        n_accept, eos_hit, self.g, self.P = rec[1], rec[2], rec[3], rec[4]
        accepted = rec[8:8 + n_accept]                               # (sampling: = hits[:n_accept]; the record also carries a device-drawn token)
        self.tokens += accepted
        if phase != 2:
            self.fill_level += 1
        self.finished_by_eos = bool(eos_hit)
        return dict(accepted=list(accepted), g_next=self.g, P_after=self.P, phase=phase)

    def _steady_graph(self) -> bool:
        return self.use_graph and self.steps > 0 and self.fill_level >= self.N - 2

    @torch.no_grad()
    @_on_device
    def step(self) -> dict:
        """One decode step = one model forward over T tokens + the device-side post-step; returns the
        host-visible record (accepted tokens, max_hit ...)."""
        e, st = self.e, self.st
        if self._steady_graph():                                     # ONE graph launch, post-step included
            phase, n_input, P_before = 2, 1, self.P
            T, _, _ = self._replay(forward_only=False)
            rec = self._polled_record()
        else:
            shape, T, P_before, _ = self._eager_model(want_rows=False)
            phase, n_input = shape.phase, shape.n_input - (P_before if shape.phase == 0 else 0)      # prefill: out row = last prompt token of the last chunk
            self._post_step(st.am, shape.n_inp, T, shape.cand_rows, phase)
            if self.emit is not None:
                self._emit_step(shape.n_inp, self._emit_src[1])
            ops.kv_commit(e.kv, 0, 0, 0, ctl=st.ctl)
            rec = st.read_record()
        return dict(T=T, P_before=P_before, n_input=n_input, max_hit=rec[0], max_hit_idx=rec[5], first_guess=rec[6], **self._take_record(rec, phase))

    @torch.no_grad()
    @_on_device
    def greedy(self, prompt: Sequence[int], max_length: int, eos_token_id=None,
               rng: Optional[random.Random] = None, keep_trace: bool = False, on_step=None, controls: Optional[GenControls] = None,
               emit=None) -> GenOut:
        """`jacobi_greedy_search_multilevel` (lade/decoding.py:697-1259), single GPU or lookahead parallel.
        on_step(accepted_tokens): called after every step with the tokens it accepted (chat printing / HF streamers,
        lade/decoding.py:1179-1200).  emit: None, or one or both of "scores" / "logits" - the result then carries the [generated, V] fp32
        rows HF's generate() returns under return_dict_in_generate (the reference refuses that, lade/decoding.py:967)."""
        if self.lp is not None and (self.lp.R > 1 or self.lp.force):
            if emit_request(emit) is not None:
                raise cabi.LadeHipError(LP_EMIT_REFUSAL)
            # the lookahead-parallel verify and EOS scan (lade_lp_reduce_apply) know neither the controls nor an EOS set
            if controls is not None and controls.active:
                raise cabi.LadeHipError("lookahead parallelism (DIST_WORKERS > 1 / FORCE_LP) does not implement repetition_penalty / "
                                        "min_length / min_new_tokens / bad_words_ids / suppress_tokens / begin_suppress_tokens / "
                                        "sequence_bias: run on one GPU without FORCE_LP")
            eos = eos_set(eos_token_id)
            if len(eos) > 1:
                raise cabi.LadeHipError(f"lookahead parallelism (DIST_WORKERS > 1 / FORCE_LP) stops on one EOS id only, got {list(eos)}: "
                                        "run on one GPU without FORCE_LP")
            from .parallel import greedy_lp
            return greedy_lp(self, prompt, max_length, eos[0] if eos else None, rng, keep_trace, on_step=on_step)
        self.start(prompt, eos_token_id, rng, controls, emit, emit_capacity(max_length, len(prompt), self.gs))
        return self._with_emitted(generate_loop(self, self.step, max_length, keep_trace, on_step, log=True))


    # ---- sampling ------------------------------------------------------------------------------------
    def _sampling_buffers(self):
        if self._smp is None:
            e, G, gs = self.e, max(self.G, 1), self.gs
            rows = 1 + G * gs
            dev = e.device
            self._smp = dict(scal=torch.zeros(rows * G, dtype=torch.float32, device=dev), stats=torch.zeros(rows * 2, dtype=torch.float32, device=dev),
                             scal_host=torch.zeros(rows * G, dtype=torch.float32).pin_memory(), guess_host=torch.zeros(G * gs, dtype=torch.int32).pin_memory(),
                             probs=torch.zeros(1, e.V, dtype=torch.float32, device=dev), probs_host=torch.zeros(e.V, dtype=torch.float32).pin_memory(),
                             am_host=torch.zeros(self.W, dtype=torch.int32).pin_memory(),
                             forced_host=torch.zeros(2 + cabi.MAX_LEVEL, dtype=torch.int32).pin_memory())
            self._smp["forced_np"] = self._smp["forced_host"].numpy()
        return self._smp

    def _draw(self, src: torch.Tensor, row: int, temperature: float, struck: Sequence[int], torch_gen: Optional[torch.Generator]):
        """One token from the distribution of logits row `row` (softmax on the device) with the struck drafts removed.  A CUDA
        generator keeps the draw on the device (what the reference does with the model on a GPU): the token is returned as a
        device tensor and reaches the host with the step's record.  Otherwise the one row goes to the host and
        torch.multinomial consumes the CPU generator (reproducible against the CPU-generated reference traces): returns an int."""
        from .sampling import final_distribution, multinomial_one
        b = self._sampling_buffers()
        probs = ops.softmax_rows(src[row:row + 1], temperature, out=b["probs"])[0]
        if torch_gen is not None and torch_gen.device.type == "cuda":
            if DRAW_WITH_TORCH:                   # LADE_DEBUG=draw_torch: torch.multinomial itself, input checks included (the same token, 12 launches more)
                return torch.multinomial(final_distribution(probs, struck), num_samples=1, generator=torch_gen)
            return multinomial_one(final_distribution(probs, struck), torch_gen)
        b["probs_host"].copy_(probs, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return int(torch.multinomial(final_distribution(b["probs_host"].clone(), struck), num_samples=1, generator=torch_gen).item())

    @torch.no_grad()
    @_on_device
    def sample_start(self, prompt: Sequence[int], warp=None, eos_token_id=None, rng: Optional[random.Random] = None,
                     torch_gen: Optional[torch.Generator] = None, controls: Optional[GenControls] = None, emit=None, emit_cap: int = 0) -> None:
        """Begins a sampling run (`sample` = sample_start + sample_step until done; bench.py drives single steps).  emit / emit_cap: as in start."""
        e, W = self.e, self.W
        rng = rng if rng is not None else random
        self.start(prompt, eos_token_id, rng, controls, emit, emit_cap)
        if torch_gen is not None and torch_gen.device.type == "cuda" and not self._draw_warm:
            # the draw's torch kernels (exponential, divide, argmax, and the strike-and-renormalise ops of a rejected draft) load their code
            # objects on first use: 10-26 ms in the middle of the first step that rejects a draft.  One dry run on a throw-away generator -
            # the caller's generator is not touched
            from .sampling import final_distribution, multinomial_one
            tg = torch.Generator(device=e.device).manual_seed(0)
            tok = multinomial_one(final_distribution(torch.full((e.V,), 1.0 / e.V, dtype=torch.float32, device=e.device), [0, 1]), tg)
            torch.zeros(4, dtype=torch.int32, device=e.device)[1:2].copy_(tok)
            self._draw_warm = True
        self._s = dict(warp=warp, fused_T=1.0 if warp is None else getattr(warp, "fused_temperature", None), rng=rng, torch_gen=torch_gen,
                       old=list(self.prompt), forced=torch.zeros(2 + cabi.MAX_LEVEL, dtype=torch.int32, device=e.device),
                       override=torch.zeros(W, dtype=torch.int32, device=e.device))

    @torch.no_grad()
    @_on_device
    def sample(self, prompt: Sequence[int], max_length: int, warp=None, eos_token_id=None,
               rng: Optional[random.Random] = None, torch_gen: Optional[torch.Generator] = None, keep_trace: bool = False,
               on_step=None, controls: Optional[GenControls] = None, emit=None) -> GenOut:
        """`jacobi_sample_multilevel` (lade/decoding.py:137-692), single GPU (the reference has no LP here).

        The model step, input assembly, pool and window stay on the GPU, and so do the probabilities: `lade_softmax_gather`
        hands the host one small table of draft probabilities per step (sampling.py).  What runs on the host is exactly what
        consumes the reference's RNG streams, in the reference's order: `rng.random()` once per verification trial,
        one `torch.multinomial` for the token that ends the step (:484-540), and the `filter_window` draws (:578-580).
        `warp`: a sampling.Warper (temperature / top-k / top-p; temperature alone is applied inside the kernels) or any callable
        mapping fp32 logits rows [r, V] to warped logits (the HF warpers the reference admits, :375-377).
        emit: as in greedy; `scores` are the warped rows (after temperature, top-k and top-p) as the verify read them - the strikes of
        rejected drafts edit the probabilities of the final draw, never these rows."""
        if self.lp is not None and (self.lp.R > 1 or self.lp.force) and emit_request(emit) is not None:
            raise cabi.LadeHipError(LP_EMIT_REFUSAL)
        self.sample_start(prompt, warp, eos_token_id, rng, torch_gen, controls, emit, emit_capacity(max_length, len(prompt), self.gs))
        return self._with_emitted(generate_loop(self, lambda: self.sample_step(keep_trace), max_length, keep_trace, on_step, log=True))

    @torch.no_grad()
    @_on_device
    def sample_step(self, keep_trace: bool = False) -> dict:
        """One sampling step: model forward (eager or the forward-only hipGraph), device-side probability table, host-side
        acceptance walk, one draw, device-side post-step."""
        from .sampling import resolve_drafts
        e, st = self.e, self.st
        W, N, G, gs = self.W, self.N, self.G, self.gs
        S = self._s
        warp, fused_T, rng, torch_gen, all_old_tokens, forced, override = S["warp"], S["fused_T"], S["rng"], S["torch_gen"], S["old"], S["forced"], S["override"]
        buf = self._sampling_buffers()
        g, fill_level = self.g, self.fill_level
        if self._steady_graph():
            # steady step: input assembly + model step + argmax replayed as one hipGraph (candidate rows padded to the bucket)
            # controls on: the body returns the processed out / candidate rows (no window rows); off: logits.float() of every row
            phase, n_inp, P_before = 2, W, self.P
            T, cand_rows, logits = self._replay(forward_only=True)
        else:
            shape, T, P_before, logits = self._eager_model(want_rows=True)
            phase, n_inp, cand_rows = shape.phase, shape.n_inp, shape.cand_rows
        # generation controls: `logits` holds the processed fp32 out row and candidate rows only (lade_gen_rows), no window rows between
        n_skip = 0 if self.controls is not None else n_inp
        step_inputs = {}
        if keep_trace and phase != 0:                            # what the step fed and judged (tests re-derive the probabilities)
            step_inputs = dict(ids=st.ids[:T].tolist(), pos=st.pos[:T].tolist(), level_sizes=level_sizes(W, N, fill_level),
                               cand_rows=cand_rows, g=g, drafts=st.guess[:g * gs].tolist() if phase == 2 else [])
        # ---- the step's token(s): rejection-sampling verify over the candidates, or a plain draw (:453-540) ----
        verify = phase == 2 and g > 0
        rows = 1 + g * gs if verify else 1
        if fused_T is not None:                              # temperature only: the kernels scale the logits themselves
            src, skip, temp = logits, n_skip, fused_T
        else:
            # top-k / top-p: one device launch over the out row and the candidate rows (lade_warp_rows); HF warper objects and
            # vocabularies beyond that kernel: torch ops on the device
            src = warp.warp_rows(logits, rows, n_skip) if hasattr(warp, "warp_rows") else None
            if src is None:
                picked = logits[0:1] if not verify else torch.cat([logits[0:1], logits[1 + n_skip:1 + n_skip + g * gs]])
                src = warp(picked)
            skip, temp = 0, 1.0
        max_hit_idx = 0
        if verify:
            ops.softmax_gather(src, rows, skip, st.guess, g, gs, max(G, 1), temp, buf["scal"], buf["stats"])
            buf["scal_host"].copy_(buf["scal"], non_blocking=True)
            buf["guess_host"].copy_(st.guess, non_blocking=True)
            torch.cuda.current_stream().synchronize()                      # the step's one table read-back
            table = buf["scal_host"].view(-1, max(G, 1))[:rows].tolist()
            if keep_trace:
                step_inputs["table"] = table
            verdict = resolve_drafts(table, buf["guess_host"][:g * gs].tolist(), g, gs, rng.random)
            hits, max_hit_idx = list(verdict.accepted), verdict.winner
            if verdict.final_row is not None:
                hits.append(self._draw(src, 0 if verdict.final_row == 0 else verdict.final_row + skip, temp, verdict.struck, torch_gen))
        else:
            hits = [self._draw(src, 0, temp, (), torch_gen)]
        max_hit = len(hits) - 1
        drawn_on_device = hits[-1] if torch.is_tensor(hits[-1]) else None
        if drawn_on_device is not None:
            hits[-1] = 0
        level_override = None
        if phase == 2 and self.eos_set:                                       # filter_window on the new level (:578-580), any EOS id
            buf["am_host"].copy_(st.am[1:1 + W], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            repl = [rng.choice(all_old_tokens) if tok in self.eos_set else -1 for tok in buf["am_host"].tolist()]
            if any(x >= 0 for x in repl):
                override.copy_(torch.tensor(repl, dtype=torch.int32))
                level_override = override
        # pinned staging (a pageable source would make the copy wait for the draw's kernels on the host); the previous step's copy is long
        # done: every step ends with the record's stream synchronisation
        buf["forced_np"][:] = [max_hit, max_hit_idx] + hits + [0] * (cabi.MAX_LEVEL - len(hits))
        forced.copy_(buf["forced_host"], non_blocking=True)
        if drawn_on_device is not None:
            forced[2 + max_hit:3 + max_hit].copy_(drawn_on_device)          # the drawn token never left the device
        self._post_step(st.am, n_inp, T, cand_rows, phase, forced=forced, level_override=level_override)
        ops.kv_commit(e.kv, 0, 0, 0, ctl=st.ctl)
        info = self._take_record(st.read_record(), phase)
        if self.emit is not None and info["accepted"]:
            # the rows of the tokens the record says were emitted (an EOS inside the step drops those behind it): token 0 from the out
            # row, token k from position k-1 of the winning candidate - every draft it accepted was judged under a row of that prefix
            proc = None
            if "scores" in self.emit:
                if fused_T is None:
                    proc = src if (src.dtype == torch.float32 and src.stride(-1) == 1) else src.float().contiguous()
                elif temp != 1.0:          # temperature alone runs inside the probability kernels: materialise logits / T for the record
                    proc = ops.warp_rows(logits, rows, n_skip, temperature=temp)
                elif self.controls is not None:
                    proc = logits          # the processed rows themselves
            self._emit_step(n_inp, proc, idx=[0] + [max_hit_idx] * (len(info["accepted"]) - 1))
        all_old_tokens += info["accepted"]
        return dict(T=T, P_before=P_before, max_hit=max_hit, max_hit_idx=max_hit_idx, **info, **step_inputs)
