"""Tensor-level wrappers over the C ABI (one python function per HIP entry point).

Every function validates shapes/dtypes on the host, passes raw device pointers to liblade_hip.so
and returns torch tensors that live on the GPU.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import cabi
from .cabi import AttnArgs, MaskParams, call, dtype_code, ptr


@dataclass
class StepMask:
    """Closed-form description of the lookahead mask of one step (see include/lade_hip.h).
    Reference: j_make_causal_mask_multilevel, lade/models/modeling_llama.py:115-207."""
    T: int
    P: int
    is_prefill: bool
    s: int = 1
    lguess: int = 0
    gs: int = 1
    level_offset: int = 0
    dist_offset: int = 0
    layout: int = 0          # 0: rows level-major (eager order); 1: levels >= 1 column-major (the reference's flash order)

    @staticmethod
    def from_levels(n_input: int, level_sizes, lguess: int, gs: int, P: int, is_prefill: bool = False, layout: int = 0) -> "StepMask":
        T = n_input + sum(level_sizes) + lguess
        return StepMask(T=T, P=P, is_prefill=is_prefill, s=level_sizes[-1], lguess=lguess, gs=gs, level_offset=n_input - 1,
                        dist_offset=1 + level_sizes[0] - level_sizes[-1], layout=layout)

    def c_struct(self) -> MaskParams:
        return MaskParams(self.T, self.P, int(self.is_prefill), self.s, self.lguess, self.gs, self.level_offset, self.dist_offset, self.layout)


def _dev(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise cabi.LadeHipError(f"{name} must be a GPU tensor (the HIP path has no CPU fallback)")


def attn_block_rows(n_rep: int, T: int) -> int:
    """query rows of one attention work-group (the kernel's shapes: 32 / 64 / 128 rows of the (head-in-group, token) space)"""
    rows = n_rep * T
    return 32 if rows <= 32 else (64 if rows <= 64 else 128)


def choose_splits(H: int, n_rep: int, T: int, S_tot: int, n_cu: int = 256, allow_single: bool = True, block_rows: int = 0, mode: int = 0) -> int:
    """KV splits of the lookahead attention.  One CU ingests only ~55-68 GB/s from HBM (tools/hbm_probe), so the
    grid (row blocks x KV heads x splits) should cover the CUs; a split is a contiguous range of 64-key tiles.
    block_rows: the work-group shape the launch will use (0: the 128-row default for more than 64 rows, else the smallest that holds them).
    mode 0: the sqrt rule below; 1: fill the CUs regardless of the merge cost; 2: half the sqrt rule's count (GQA heads whose partial
    round trip dominates) - the engine's in-step autotune picks (shape, mode) per row class (StepEngine._refine_in_step)."""
    br = block_rows or attn_block_rows(n_rep, T)
    blocks = (H // n_rep) * ((n_rep * T + br - 1) // br)
    tiles = max(1, (S_tot + 63) // 64)
    if tiles <= 5 and allow_single:               # <= 320 keys: one work-group per head beats a second (merge) launch
        return 1
    forced = int(cabi.debug("attn_split_rule", "0"))     # experiments: 1 = fill the CUs regardless of the merge cost
    fill = max(1, n_cu // max(blocks, 1))
    if forced == 1 or mode == 1:
        want = max(1, min(fill, tiles, 32))
    else:
        # streaming time per work-group falls as tiles/splits, the merge (and the partial round trip) grows with splits: the measured
        # optimum follows sqrt(tiles) - 5 splits at 18 tiles, 6 at 34, 8 at 65 (round 2, isolated pair at 34 tiles: 16.8 us with 6
        # splits, 17.1 us with 8)
        want = max(1, min(fill, math.isqrt(max(tiles - 1, 0)) + 1, tiles, 32))
        if mode == 2:
            want = max(1 if allow_single else 2, (want + 1) // 2)
    tps = (tiles + want - 1) // want              # tiles per split
    return (tiles + tps - 1) // tps               # drop the splits that would be empty


def attn_fwd(q: torch.Tensor, k_cache: torch.Tensor, vt_cache: torch.Tensor, mask: StepMask, *, H: int, Hkv: int, d: int,
             out: Optional[torch.Tensor] = None, n_splits: Optional[int] = None, scale: Optional[float] = None,
             q_row_stride: Optional[int] = None, part_o: Optional[torch.Tensor] = None, part_ml: Optional[torch.Tensor] = None,
             dyn_P: Optional[torch.Tensor] = None, wg_rows: int = 0) -> torch.Tensor:
    """Lookahead attention for one step.  q: [T, >=H*d] rows (token stride q_row_stride elements, default
    q.stride(0)); k_cache [Hkv, S_max, d]; vt_cache [Hkv, d, S_max]; returns out [T, H*d].
    wg_rows: work-group shape (0 = default, 32 | 64 | 128 query rows per work-group)."""
    for n, t in (("q", q), ("k_cache", k_cache), ("vt_cache", vt_cache)):
        _dev(t, n)
    T = mask.T
    S_max = k_cache.shape[1]
    assert k_cache.shape == (Hkv, S_max, d) and vt_cache.shape == (Hkv, d, S_max), (k_cache.shape, vt_cache.shape)
    assert k_cache.is_contiguous() and vt_cache.is_contiguous()
    dt = k_cache.dtype
    assert q.stride(-1) == 1 and q.dtype == dt
    dev = k_cache.device
    if out is None:
        out = torch.empty(T, H * d, dtype=dt, device=dev)
    if n_splits is None:
        n_splits = 1 if dt == torch.float32 else choose_splits(H, H // Hkv, T, mask.P + T)
    if dt == torch.float32:
        n_splits = 1
    if n_splits > 1:
        if part_o is None:
            part_o = torch.empty(n_splits, T, H, d, dtype=dt, device=dev)
        if part_ml is None:
            part_ml = torch.empty(n_splits, H, T, 2, dtype=torch.float32, device=dev)
    a = AttnArgs(ptr(q), ptr(k_cache), ptr(vt_cache), ptr(out), ptr(part_o), ptr(part_ml), ptr(dyn_P),
                 q_row_stride if q_row_stride is not None else q.stride(0), out.stride(0), H, Hkv, d, S_max,
                 DTYPE_CODE_OF(dt), n_splits, scale if scale is not None else 1.0 / math.sqrt(d), mask.c_struct(), int(wg_rows))
    call("lade_attn_fwd", C.byref(a))
    if n_splits > 1:
        call("lade_attn_combine", C.byref(a))
    return out


PREFILL_ATTN_CALLS = 0      # launches of lade_attn_prefill by this process (tests assert that the entry point was reached, or was not)


def attn_prefill(q: torch.Tensor, k_cache: torch.Tensor, vt_cache: torch.Tensor, mask: StepMask, *, H: int, Hkv: int, d: int,
                 out: Optional[torch.Tensor] = None, scale: Optional[float] = None, q_row_stride: Optional[int] = None) -> torch.Tensor:
    """One-pass causal attention of a prefill chunk (lade_attn_prefill: bf16 / f16, d = 64 | 128, mask.is_prefill): row t sees keys 0 .. P + t.
    q: [T, >= H*d] rows (token stride q_row_stride elements, default q.stride(0): a view into the qkv buffer is fine); k_cache [Hkv, S_max, d];
    vt_cache [Hkv, d, S_max] with the chunk's rows P .. P+T already appended; returns out [T, H*d].  One launch, no partial buffers.
    What the library refuses (fp32, lookahead masks, other head sizes) raises LadeHipError: there is no fall-back to lade_attn_fwd here -
    the caller decides which kernel a step runs on (tuning.use_prefill_attn)."""
    global PREFILL_ATTN_CALLS
    for n, t in (("q", q), ("k_cache", k_cache), ("vt_cache", vt_cache)):
        _dev(t, n)
    T = mask.T
    S_max = k_cache.shape[1]
    assert k_cache.shape == (Hkv, S_max, d) and vt_cache.shape == (Hkv, d, S_max), (k_cache.shape, vt_cache.shape)
    assert k_cache.is_contiguous() and vt_cache.is_contiguous()
    dt = k_cache.dtype
    assert q.stride(-1) == 1 and q.dtype == dt
    if out is None:
        out = torch.empty(T, H * d, dtype=dt, device=k_cache.device)
    assert out.dtype == dt and out.dim() == 2 and out.shape[0] >= T and out.shape[1] == H * d and out.stride(-1) == 1 and q.shape[0] >= T, (out.shape, out.dtype)
    a = AttnArgs(ptr(q), ptr(k_cache), ptr(vt_cache), ptr(out), None, None, None,
                 q_row_stride if q_row_stride is not None else q.stride(0), out.stride(0), H, Hkv, d, S_max,
                 DTYPE_CODE_OF(dt), 1, scale if scale is not None else 1.0 / math.sqrt(d), mask.c_struct(), 0)
    call("lade_attn_prefill", C.byref(a))
    PREFILL_ATTN_CALLS += 1
    return out


def DTYPE_CODE_OF(dt: torch.dtype) -> int:
    try:
        return cabi.DTYPE_CODE[dt]
    except KeyError:
        raise cabi.LadeHipError(f"unsupported dtype {dt}")


def time_attn(q, k_cache, vt_cache, mask: StepMask, *, H, Hkv, d, n_splits: int, reps: int = 20, debug_timeline: bool = False, wg_rows: int = 0):
    """Mean duration in microseconds of one attention launch (+combine), measured with hipEvents on the launch stream
    inside the library.  k_cache / vt_cache may be LISTS of caches: they are used round-robin, one per repetition, so
    that with enough of them (total > the 256 MB Infinity Cache) every launch streams its K/V from HBM like the
    consecutive layers of a decode step; a single cache stays Infinity-Cache resident across repetitions."""
    ks = list(k_cache) if isinstance(k_cache, (list, tuple)) else [k_cache]
    vs = list(vt_cache) if isinstance(vt_cache, (list, tuple)) else [vt_cache]
    assert len(ks) == len(vs)
    T, S_max = mask.T, ks[0].shape[1]
    out = torch.empty(T, H * d, dtype=q.dtype, device=q.device)
    part_o = torch.empty(max(n_splits, 1), T, H, d, dtype=q.dtype, device=q.device)
    n_ml = max(n_splits, 1) * H * T * 2
    part_ml = torch.zeros(n_ml + 16 * 4096, dtype=torch.float32, device=q.device)   # + room for LADE_DEBUG=attn_dbg=16 timestamps
    arr = (AttnArgs * len(ks))()
    for i, (k, v) in enumerate(zip(ks, vs)):
        arr[i] = AttnArgs(ptr(q), ptr(k), ptr(v), ptr(out), ptr(part_o), ptr(part_ml), None, q.stride(0), out.stride(0),
                          H, Hkv, d, S_max, dtype_code(q), n_splits, 1.0 / math.sqrt(d), mask.c_struct(), int(wg_rows))
    us = C.c_float(0.0)
    if len(ks) == 1:
        call("lade_time_attn", C.byref(arr[0]), reps, C.byref(us))
    else:
        call("lade_time_attn_rot", arr, len(ks), reps, C.byref(us))
    if debug_timeline:
        torch.cuda.synchronize()
        return float(us.value), part_ml[n_ml:].view(torch.int64).view(-1, 8).cpu()
    return float(us.value)


def mask_render(mask: StepMask, device="cuda") -> torch.Tensor:
    out = torch.zeros(mask.T, mask.P + mask.T, dtype=torch.uint8, device=device)
    m = mask.c_struct()
    call("lade_mask_render", C.byref(m), ptr(out))
    return out


def qkv_epilogue(bias: Optional[torch.Tensor] = None, q_norm: Optional[torch.Tensor] = None, k_norm: Optional[torch.Tensor] = None,
                 eps: float = 1e-6) -> cabi.QkvEpilogue:
    """lade_qkv_epilogue over device tensors in the model dtype: bias [(H+2Hkv)*d] (Qwen2's q / k / v bias, fused like wqkv), q_norm / k_norm [d]
    (Qwen3's per-head RMSNorm weights).  The struct holds raw pointers: the tensors must outlive every launch (and every captured graph) that
    uses it."""
    for name, t in (("bias", bias), ("q_norm", q_norm), ("k_norm", k_norm)):
        if t is not None:
            _dev(t, name)
            assert t.dim() == 1 and t.is_contiguous(), f"{name} must be a contiguous vector"
    return cabi.QkvEpilogue(ptr(bias), ptr(q_norm), ptr(k_norm), float(eps))


def _rope_kv_append(qkv, part, n_parts, q_out, positions, cos, sin, k_cache, vt_cache, T, P, H, Hkv, d, dyn_P, epi) -> None:
    """the one call behind both RoPE wrappers: exactly one of qkv / part"""
    call("lade_rope_kv_append", ptr(qkv), ptr(part), n_parts, T * (H + 2 * Hkv) * d, ptr(q_out), ptr(positions), ptr(cos), ptr(sin), ptr(k_cache),
         ptr(vt_cache), T, P, ptr(dyn_P), H, Hkv, d, k_cache.shape[1], cos.shape[0], dtype_code(q_out if qkv is None else qkv),
         None if epi is None else C.byref(epi))


def rope_kv_append(qkv: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, k_cache: torch.Tensor,
                   vt_cache: torch.Tensor, P: int, *, H: int, Hkv: int, d: int, dyn_P: Optional[torch.Tensor] = None,
                   epi: Optional[cabi.QkvEpilogue] = None) -> None:
    """qkv [T, (H+2Hkv)*d] (q rotated in place); k_cache [Hkv,S_max,d]; vt_cache [Hkv,d,S_max]; epi: the qkv epilogue (`qkv_epilogue`; None =
    the plain kernel)."""
    _dev(qkv, "qkv")
    T = qkv.shape[0]
    assert qkv.is_contiguous() and qkv.shape[1] == (H + 2 * Hkv) * d
    assert positions.dtype == torch.int32 and positions.numel() >= T
    assert cos.dtype == qkv.dtype and cos.shape[1] == d and cos.is_contiguous() and sin.is_contiguous()
    _rope_kv_append(qkv, None, 0, None, positions, cos, sin, k_cache, vt_cache, T, P, H, Hkv, d, dyn_P, epi)


def kv_commit(cache: torch.Tensor, src: int, dst: int, cnt: int, ctl: Optional[torch.Tensor] = None) -> None:
    """cache [L, 2, Hkv*S_max*d] viewed as K [Hkv,S_max,d] / V^T [Hkv,d,S_max] per layer."""
    L = cache.shape[0]
    meta = cache._lade_meta
    call("lade_kv_commit", ptr(cache), cache.stride(0), cache.stride(1), L, meta["Hkv"], meta["d"], meta["S_max"], src, dst, cnt,
         ptr(ctl), 0, cache.element_size())


def argmax_rows(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev(logits, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    rows, V = logits.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.int32, device=logits.device)
    call("lade_argmax_rows", ptr(logits), logits.stride(0), rows, V, dtype_code(logits), ptr(out))
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert x.is_contiguous() and x.dim() == 2
    if out is None:
        out = torch.empty_like(x)
    call("lade_rmsnorm", ptr(x), ptr(w), ptr(out), x.shape[0], x.shape[1], eps, dtype_code(x))
    return out


def embed_rmsnorm(table: torch.Tensor, ids: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float, out: torch.Tensor, rows: int) -> torch.Tensor:
    """x[r] = table[ids[r]]; out[r] = rmsnorm(x[r]) for r < rows: the step's embedding lookup and its first norm in one launch."""
    assert table.is_contiguous() and x.is_contiguous() and out.is_contiguous() and ids.dtype == torch.int32 and table.shape[1] == x.shape[1]
    call("lade_embed_rmsnorm", ptr(table), table.shape[0], ptr(ids), ptr(x), ptr(w), ptr(out), rows, x.shape[1], eps, dtype_code(x))
    return out


def add_rmsnorm(x: torch.Tensor, r: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x += r (in place); returns rmsnorm(x)."""
    assert x.is_contiguous() and r.is_contiguous() and x.shape == r.shape
    if out is None:
        out = torch.empty_like(x)
    call("lade_add_rmsnorm", ptr(x), ptr(r), None, 0, 0, None, 0, ptr(w), ptr(out), x.shape[0], x.shape[1], eps, dtype_code(x))
    return out


def add_rmsnorm_rows(x: torch.Tensor, sel: torch.Tensor, n_sel: int, w: torch.Tensor, eps: float, *, r: Optional[torch.Tensor] = None,
                     part: Optional[torch.Tensor] = None, n_parts: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[j] = rmsnorm(x[sel[j]] + res[sel[j]]), res = r or the sum of the first n_parts fp32 split-K partials in `part`
    ([n_parts][rows][hidden]); x stays as it is.  The step's tail: only the rows whose logits are read."""
    rows, hidden = x.shape
    assert x.is_contiguous() and sel.dtype == torch.int32 and (r is None) != (part is None)
    if out is None:
        out = torch.empty(n_sel, hidden, dtype=x.dtype, device=x.device)
    call("lade_add_rmsnorm", ptr(x), ptr(r), ptr(part), n_parts, rows * hidden, ptr(sel), rows, ptr(w), ptr(out), n_sel, hidden, eps, dtype_code(x))
    return out[:n_sel]


def silu_mul(gu: torch.Tensor, out: Optional[torch.Tensor] = None, layout: int = 0) -> torch.Tensor:
    """layout 0: gu rows = [gate | up]; 1: 16-row interleaved groups (the engine's fused gate/up order, see interleave_gate_up)"""
    assert gu.is_contiguous() and gu.shape[1] % 2 == 0
    inter = gu.shape[1] // 2
    if out is None:
        out = torch.empty(gu.shape[0], inter, dtype=gu.dtype, device=gu.device)
    call("lade_silu_mul", ptr(gu), None, 0, 0, ptr(out), gu.shape[0], inter, layout, dtype_code(gu))
    return out


def interleave_gate_up(wg: torch.Tensor, wu: torch.Tensor) -> torch.Tensor:
    """[inter, hid] x 2 -> fused [2*inter, hid] in groups of 16 rows: rows 32p .. 32p+15 = gate[16p ..], rows 32p+16 .. 32p+31 =
    up[16p ..].  In an MFMA 32x32 output tile a lane's accumulators e and e+8 are then gate and up of the same column."""
    inter, hid = wg.shape
    assert wu.shape == wg.shape and inter % 16 == 0
    return torch.stack([wg.view(inter // 16, 16, hid), wu.view(inter // 16, 16, hid)], dim=1).reshape(2 * inter, hid).contiguous()


def gather_rows(src: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None, rows: Optional[int] = None) -> torch.Tensor:
    assert src.is_contiguous() and idx.dtype == torch.int32
    rows = idx.numel() if rows is None else rows
    if out is None:
        out = torch.empty(rows, src.shape[1], dtype=src.dtype, device=src.device)
    call("lade_gather_rows", ptr(src), ptr(idx), ptr(out), rows, src.shape[1], src.element_size(), src.shape[0])
    return out


def softmax_rows(logits: torch.Tensor, temperature: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert logits.dim() == 2 and logits.stride(1) == 1
    probs = out if out is not None else torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
    assert probs.dtype == torch.float32 and probs.numel() >= logits.numel()
    call("lade_softmax_rows", ptr(logits), logits.stride(0), logits.shape[0], logits.shape[1], dtype_code(logits), float(temperature), ptr(probs))
    return probs


WARP_MAX_V = 1 << 24      # lade_warp_rows: a row of <= 32768 tokens lives in one work-group's registers, a larger one in the output row (L2)


def _warp_rows_args(logits: torch.Tensor, rows: int, skip: int, out: Optional[torch.Tensor]) -> torch.Tensor:
    """the checks both warp entry points make before a raw pointer leaves; returns `out` (allocated when None)"""
    _dev(logits, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    V = logits.shape[1]
    assert logits.shape[0] >= (rows + skip if rows > 1 else 1)
    if out is None:
        out = torch.empty(rows, V, dtype=torch.float32, device=logits.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= rows * V
    return out


def warp_rows(logits: torch.Tensor, rows: int, skip: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
              out: Optional[torch.Tensor] = None, *, min_p: float = 0.0, typical_p: float = 1.0, epsilon_cutoff: float = 0.0,
              eta_cutoff: float = 0.0) -> torch.Tensor:
    """Temperature -> top-k -> top-p -> min-p -> typical -> epsilon cutoff -> eta cutoff (HF warper semantics and order) in one launch.
    logits [>= rows + skip, V]: logical row 0 is physical row 0, logical row r > 0 is physical row r + skip (out row + the candidate rows
    behind the window rows).  Returns fp32 [rows, V] with the removed tokens at -inf.  The four keywords default to "off"; with all of them
    off this is lade_warp_rows, else lade_warp_rows_ex."""
    if min_p > 0.0 or typical_p < 1.0 or epsilon_cutoff > 0.0 or eta_cutoff > 0.0:
        return _warp_rows_ex(logits, rows, skip, temperature, top_k, top_p, out, min_p, typical_p, epsilon_cutoff, eta_cutoff)
    out = _warp_rows_args(logits, rows, skip, out)
    call("lade_warp_rows", ptr(logits), logits.stride(0), rows, logits.shape[1], dtype_code(logits), float(temperature), int(top_k), float(top_p),
         int(skip), ptr(out))
    return out[:rows] if out.dim() == 2 else out


def _warp_rows_ex(logits: torch.Tensor, rows: int, skip: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                  out: Optional[torch.Tensor] = None, min_p: float = 0.0, typical_p: float = 1.0, epsilon_cutoff: float = 0.0,
                  eta_cutoff: float = 0.0) -> torch.Tensor:
    """lade_warp_rows_ex as it is, whatever the values (with the four later stages off it runs the kernels of lade_warp_rows: the tests
    compare the two entry points through this)"""
    import ctypes as C
    from .cabi import WarpParams
    out = _warp_rows_args(logits, rows, skip, out)
    params = WarpParams(float(temperature), int(top_k), float(top_p), float(min_p), float(typical_p), float(epsilon_cutoff), float(eta_cutoff))
    call("lade_warp_rows_ex", ptr(logits), logits.stride(0), rows, logits.shape[1], dtype_code(logits), C.byref(params), int(skip), ptr(out))
    return out[:rows] if out.dim() == 2 else out


def softmax_gather(logits: torch.Tensor, rows: int, skip: int, guess: torch.Tensor, g: int, gs: int, g_cap: int, temperature: float,
                   scal: torch.Tensor, stats: torch.Tensor, g_dev: Optional[torch.Tensor] = None) -> None:
    """Device side of the sampling verify: per-row softmax statistics + the draft probabilities the acceptance loop reads
    (see lade_softmax_gather in include/lade_hip.h).  logits [>= rows + skip, V]; scal [rows, g_cap] fp32; stats [rows, 2] fp32."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and scal.dtype == torch.float32 and stats.dtype == torch.float32
    V = logits.shape[1]
    assert logits.shape[0] >= (rows + skip if rows > 1 else 1) and scal.numel() >= rows * g_cap and stats.numel() >= 2 * rows
    call("lade_softmax_gather", ptr(logits), logits.stride(0), rows, V, dtype_code(logits), float(temperature), skip, ptr(guess), ptr(g_dev), g, gs,
         g_cap, ptr(scal), ptr(stats))


def to_ktile(w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row-major weight [N, K] -> the K-tile-major copy [K/64, N, 64] the skinny GEMM streams fastest (`lade_weight_to_ktile`): the
    128-byte segments of all N rows of one 64-deep K tile are contiguous.  The GEMM wrappers below tell the two layouts apart by the
    number of dimensions."""
    N, K = w.shape
    assert w.stride(1) == 1 and K % 64 == 0
    if out is None:
        out = torch.empty(K // 64, N, 64, dtype=w.dtype, device=w.device)
    assert out.shape == (K // 64, N, 64) and out.is_contiguous() and out.dtype == w.dtype
    call("lade_weight_to_ktile", ptr(w), w.stride(0), ptr(out), N, K, dtype_code(w))
    return out


def from_ktile(wkt: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K-tile-major [K/64, N, 64] -> row-major [N, K] (`lade_weight_from_ktile`), into `out` when given (a reused scratch)"""
    KT, N, _ = wkt.shape
    assert wkt.is_contiguous() and wkt.shape[2] == 64
    if out is None:
        out = torch.empty(N, KT * 64, dtype=wkt.dtype, device=wkt.device)
    assert out.shape == (N, KT * 64) and out.stride(1) == 1 and out.dtype == wkt.dtype
    call("lade_weight_from_ktile", ptr(wkt), ptr(out), out.stride(0), N, KT * 64, dtype_code(wkt))
    return out


def _gemm(a: torch.Tensor, w: torch.Tensor, c, ldc: int, part, n_split: int, bn: int, mb: int, mt: int, nt: int, epilogue: int, ring: int = 0) -> None:
    M, K = a.shape
    assert a.stride(1) == 1
    if w.dim() == 3:                          # K-tile-major [K/64, N, 64]
        assert w.is_contiguous() and w.shape[0] * 64 == K and w.shape[2] == 64
        call("lade_gemm_skinny_kt", ptr(a), a.stride(0), ptr(w), c, ldc, part, M, w.shape[1], K, n_split, bn, mb, mt, nt, ring, epilogue, dtype_code(a))
    else:
        assert w.shape[1] == K and w.stride(1) == 1
        call("lade_gemm_skinny", ptr(a), a.stride(0), ptr(w), w.stride(0), c, ldc, part, M, w.shape[0], K, n_split, bn, mb, mt, nt, ring, epilogue, dtype_code(a))


def weight_rows(w: torch.Tensor) -> int:
    """N of a projection weight in either layout"""
    return w.shape[1] if w.dim() == 3 else w.shape[0]


def gemm_skinny(a: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None, n_split: int = 1, bn: int = 128,
                part: Optional[torch.Tensor] = None, mb: int = 0, mt: int = 0, nt: int = 0, ring: int = 0) -> torch.Tensor:
    """out[M,N] = a[M,K] @ w[N,K]^T on the hand-written weight-streaming kernel (bf16 / f16); w row-major or K-tile-major (to_ktile).
    ring: stages of the LDS ring (0 = the shape's default)."""
    M, N = a.shape[0], weight_rows(w)
    if out is None:
        out = torch.empty(M, N, dtype=a.dtype, device=a.device)
    if n_split > 1 and part is None:
        part = torch.empty(n_split, M, N, dtype=torch.float32, device=a.device)
    _gemm(a, w, ptr(out), out.stride(0), ptr(part), n_split, bn, mb, mt, nt, 0, ring)
    if n_split > 1:
        call("lade_splitk_reduce", ptr(part), ptr(out), out.stride(0), M, N, n_split, dtype_code(a))
    return out


def gemm_argmax(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, pairs: Optional[torch.Tensor] = None, bn: int = 128, mb: int = 0, mt: int = 0,
                nt: int = 0, ring: int = 0) -> torch.Tensor:
    """out[m] = argmax_n (a @ w^T)[m][n] (int32, the value compared after rounding to the model dtype, first index wins ties) without
    materialising the product: the GEMM's epilogue leaves one (value, column) pair per row and column block in `pairs`
    (fp32 [M, ceil(N / bn), 2]), lade_argmax_pairs merges them.  Same ids as argmax_rows(gemm_skinny(a, w))."""
    M, N = a.shape[0], weight_rows(w)
    assert bn in (32, 64, 96, 128, 192, 224, 256) and M <= 128, "the pair buffer is indexed by the kernel's own column-block count"
    nb = (N + bn - 1) // bn
    if pairs is None:
        pairs = torch.empty(M * nb * 2, dtype=torch.float32, device=a.device)
    assert pairs.dtype == torch.float32 and pairs.numel() >= M * nb * 2 and out.dtype == torch.int32 and out.numel() >= M
    _gemm(a, w, None, 0, ptr(pairs), 1, bn, mb, mt, nt, 2, ring)
    call("lade_argmax_pairs", ptr(pairs), M, nb, ptr(out))
    return out


def gemm_swiglu(a: torch.Tensor, w_gu: torch.Tensor, out: torch.Tensor, bn: int, mb: int, mt: int = 0, nt: int = 0, ring: int = 0) -> torch.Tensor:
    """out[M, inter] = silu(a @ gate^T) * (a @ up^T) in ONE launch: w_gu is the 16-row interleaved fused weight (interleave_gate_up),
    row-major or K-tile-major; no split-K, no fp32 partials, no SwiGLU kernel."""
    assert out.shape == (a.shape[0], weight_rows(w_gu) // 2) and out.stride(1) == 1
    _gemm(a, w_gu, ptr(out), out.stride(0), None, 1, bn, mb, mt, nt, 1, ring)
    return out


def gemm_parts(a: torch.Tensor, w: torch.Tensor, part: torch.Tensor, n_split: int, bn: int, mb: int, mt: int = 0, nt: int = 0, ring: int = 0) -> None:
    """split-K GEMM that leaves its result as n_split fp32 partials in `part` ([n_split][M][N], contiguous) for a
    `*_parts` consumer kernel - no reduce pass."""
    M, N = a.shape[0], weight_rows(w)
    if n_split * M * N > part.numel():
        raise cabi.LadeHipError(f"split-K workspace too small: {n_split} x {M} x {N} fp32 partials > {part.numel()}")
    _gemm(a, w, None, 0, ptr(part), n_split, bn, mb, mt, nt, 0, ring)


QKV_ROPE_SHAPES = {(1, 1), (2, 1), (3, 3), (4, 2)}       # (mb, mt) the fused qkv kernel is built for, at bn = 96, nt = 1 (csrc/gemm_qkv_rope.hip)


def gemm_qkv_rope(a: torch.Tensor, w: torch.Tensor, part: torch.Tensor, tickets: torch.Tensor, q_out: torch.Tensor, positions: torch.Tensor,
                  cos: torch.Tensor, sin: torch.Tensor, k_cache: torch.Tensor, vt_cache: torch.Tensor, P: int, *, H: int, Hkv: int, d: int,
                  bn: int, mb: int, mt: int, nt: int, ring: int = 0, dyn_P: Optional[torch.Tensor] = None) -> None:
    """gemm_parts with two splits + rope_kv_append_parts in ONE launch (`lade_gemm_qkv_rope`): the two work-groups of an n-block reduce their
    pair themselves and the second to arrive rotates q / k and appends K / V^T.  Same bits in q_out and the cache rows as the two launches.
    part: the hand-off space (fp32; its contents afterwards mean nothing to a caller); tickets: int32, zero before the first launch, left zero."""
    M, N = a.shape[0], weight_rows(w)
    assert a.stride(1) == 1 and part.dtype == torch.float32 and tickets.dtype == torch.int32 and positions.dtype == torch.int32 and positions.numel() >= M
    assert cos.dtype == a.dtype and cos.shape[1] == d and cos.is_contiguous() and sin.is_contiguous() and q_out.is_contiguous() and q_out.dtype == a.dtype
    assert q_out.numel() >= M * H * d and k_cache.dtype == a.dtype and vt_cache.dtype == a.dtype
    kt = w.dim() == 3
    if kt:
        assert w.is_contiguous() and w.shape[0] * 64 == a.shape[1] and w.shape[2] == 64
    else:
        assert w.shape[1] == a.shape[1] and w.stride(1) == 1
    rope = cabi.QkvRopeArgs(ptr(q_out), ptr(positions), ptr(cos), ptr(sin), ptr(k_cache), ptr(vt_cache), ptr(dyn_P), P, H, Hkv, d, k_cache.shape[1],
                            cos.shape[0])
    call("lade_gemm_qkv_rope", ptr(a), a.stride(0), ptr(w), 8 if kt else w.stride(0), int(kt), ptr(part), part.numel(), ptr(tickets), tickets.numel(), M, N,
         a.shape[1], bn, mb, mt, nt, ring, C.byref(rope), dtype_code(a))


def qkv_pair_row(n: int, H: int, Hkv: int, d: int) -> int:
    """the weight row the fused qkv kernel streams into row n of its tile order (`lade_qkv_pair_row`; host only)"""
    r = cabi.lib().lade_qkv_pair_row(n, H, Hkv, d)
    if r < 0:
        raise cabi.LadeHipError(f"lade_qkv_pair_row: n={n} H={H} Hkv={Hkv} d={d}")
    return r


def add_rmsnorm_parts(x: torch.Tensor, part: torch.Tensor, n_parts: int, w: torch.Tensor, eps: float, out: torch.Tensor) -> torch.Tensor:
    """add_rmsnorm with the residual as the first n_parts fp32 split-K partials of `part` ([n_parts][rows][hidden])"""
    rows, hidden = x.shape
    call("lade_add_rmsnorm", ptr(x), None, ptr(part), n_parts, rows * hidden, None, 0, ptr(w), ptr(out), rows, hidden, eps, dtype_code(x))
    return out


def silu_mul_parts(part: torch.Tensor, n_parts: int, rows: int, inter: int, out: torch.Tensor, layout: int = 0) -> torch.Tensor:
    """silu_mul on the first n_parts fp32 split-K partials of `part` ([n_parts][rows][2 * inter])"""
    call("lade_silu_mul", None, ptr(part), n_parts, rows * 2 * inter, ptr(out), rows, inter, layout, dtype_code(out))
    return out


def rope_kv_append_parts(part: torch.Tensor, n_parts: int, q_out: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                         k_cache: torch.Tensor, vt_cache: torch.Tensor, T: int, P: int, *, H: int, Hkv: int, d: int,
                         dyn_P: Optional[torch.Tensor] = None, epi: Optional[cabi.QkvEpilogue] = None) -> None:
    """rope_kv_append on the first n_parts fp32 split-K partials of `part` ([n_parts][T][(H+2Hkv)*d]); the rotated q goes to q_out [T, H*d].
    The epilogue's bias joins the fp32 sum of the partials before its one rounding."""
    _rope_kv_append(None, part, n_parts, q_out, positions, cos, sin, k_cache, vt_cache, T, P, H, Hkv, d, dyn_P, epi)


# the names the epilogue arrived under: the same two functions (tests/test_gpu_qkv_epilogue.py compares `x(..)` with `x_ex(.., epi=None)`)
rope_kv_append_ex = rope_kv_append
rope_kv_append_parts_ex = rope_kv_append_parts


# ---- generation controls (repetition penalty, min length, token constraints; include/lade_hip.h "generation controls") -------------------------------
def host_ids(ids) -> "C.Array":
    """a host int32 array for the entry points that copy a short id list into their launch (EOS sets)"""
    import ctypes as C
    return (C.c_int32 * max(len(ids), 1))(*[int(t) for t in ids])


def gen_ctl_init(gen: torch.Tensor, V: int, penalty: float, min_len: int, eos_ids, prompt: torch.Tensor) -> None:
    """penalty / min_len / the min-length EOS ids into the control block, seen set = the prompt tokens (device int32)"""
    assert gen.dtype == torch.int32 and gen.numel() >= cabi.gen_words(V) and prompt.dtype == torch.int32
    call("lade_gen_ctl_init", ptr(gen), V, float(penalty), int(min_len), host_ids(eos_ids), len(eos_ids), ptr(prompt), prompt.numel())


def gen_constraints_init(gen: torch.Tensor, cons: torch.Tensor, V: int, ban, begin_ban, begin_index: int, sequence_bias, add_bias: bool,
                         prompt: torch.Tensor) -> None:
    """Writes the token-constraint block `cons` (int32 [cabi.gen_cons_words(V)]) and attaches it to `gen` (lade_gen_constraints_init):
    ban / begin_ban id lists, sequence_bias = ((tokens, bias), ...) in HF's dict order, prompt (device int32) seeds the tail.  After
    gen_ctl_init, once per sequence."""
    import numpy as np
    assert gen.dtype == torch.int32 and cons.dtype == torch.int32 and cons.numel() >= cabi.gen_cons_words(V) and prompt.dtype == torch.int32
    ban_a = np.asarray(list(ban), dtype=np.int32).reshape(-1)
    begin_a = np.asarray(list(begin_ban), dtype=np.int32).reshape(-1)
    off = np.zeros(len(sequence_bias) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(seq) for seq, _ in sequence_bias], dtype=np.int64)
    tok = np.asarray([t for seq, _ in sequence_bias for t in seq], dtype=np.int32).reshape(-1)
    bias = np.asarray([b for _, b in sequence_bias], dtype=np.float32).reshape(-1)

    def host(a):
        return a.ctypes.data if a.size else None

    call("lade_gen_constraints_init", ptr(gen), ptr(cons), V, host(ban_a), ban_a.size, host(begin_a), begin_a.size, int(begin_index),
         off.ctypes.data, host(tok), host(bias), len(sequence_bias), int(bool(add_bias or len(sequence_bias))), ptr(prompt), prompt.numel())


def gen_ctl_update(gen: torch.Tensor, ctl: torch.Tensor) -> None:
    call("lade_gen_ctl_update", ptr(gen), ptr(ctl))


def gen_argmax(logits: torch.Tensor, n_inp: int, gs: int, gen: torch.Tensor, ctl: torch.Tensor, guess: torch.Tensor, pos: torch.Tensor,
               sel: Optional[torch.Tensor], am: torch.Tensor, rows_out: Optional[torch.Tensor] = None) -> None:
    """Processed row argmax of a step's logits [out | n_inp window | candidates] (lade_gen_argmax); with rows_out [1 + cand_rows, V]
    fp32 also the processed out / candidate rows (lade_gen_rows)."""
    _dev(logits, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1 and am.dtype == torch.int32 and am.numel() >= logits.shape[0]
    rows, V = logits.shape
    args = (ptr(logits), logits.stride(0), rows, V, dtype_code(logits), n_inp, gs, ptr(gen), ptr(ctl), ptr(guess), ptr(pos), ptr(sel), ptr(am))
    if rows_out is None:
        call("lade_gen_argmax", *args)
    else:
        assert rows_out.dtype == torch.float32 and rows_out.is_contiguous() and rows_out.numel() >= (rows - n_inp) * V
        call("lade_gen_rows", *args, ptr(rows_out))


# ---- emitted rows (per-token scores / logits of generate(); include/lade_hip.h "emitted rows") ------------------------------------
def emit_init(desc: torch.Tensor, scores: Optional[torch.Tensor], logits: Optional[torch.Tensor], V: int) -> None:
    """Points the device descriptor (int64 [cabi.EMIT_WORDS]) at the fp32 [cap_rows, V] destination buffers (either may be None) and
    zeroes its row counter: once per generate() call, captured steps keep reading the same descriptor."""
    assert desc.dtype == torch.int64 and desc.numel() >= cabi.EMIT_WORDS
    cap = None
    for name, t in (("scores", scores), ("logits", logits)):
        if t is not None:
            _dev(t, name)
            assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.shape[1] == V, (name, t.shape, t.dtype)
            assert cap is None or cap == t.shape[0]
            cap = t.shape[0]
    call("lade_emit_init", ptr(desc), ptr(scores), ptr(logits), 0 if cap is None else cap, V)


def emit_rows(desc: torch.Tensor, raw: torch.Tensor, n_inp: int, gs: int, proc: Optional[torch.Tensor] = None, ctl: Optional[torch.Tensor] = None,
              idx=None) -> None:
    """Appends the rows of the tokens one step emitted to the descriptor's buffers (lade_emit_rows).  raw: the step's logits [out | n_inp
    window rows | candidate rows] in the model dtype; proc: the processed fp32 rows [out | candidate rows] that become `scores` (None: the
    widened raw rows).  idx None: count and candidate are read from ctl on the device (greedy); else a host sequence, one entry per token:
    the candidate that supplied it (entry 0 is the out row's and is ignored)."""
    _dev(raw, "raw")
    assert raw.dim() == 2 and raw.stride(1) == 1 and desc.dtype == torch.int64
    if proc is not None:
        assert proc.dtype == torch.float32 and proc.dim() == 2 and proc.stride(1) == 1 and proc.shape[1] == raw.shape[1]
    if idx is None:
        need = None              # decided on the device: the caller's candidate rows are those the post-step verified
        harr, n_idx = None, 0
    else:
        n_idx = len(idx)
        need = (0 if n_idx <= 1 else max(int(c) for c in idx[1:]) * gs + n_idx - 1)
        harr = host_ids(idx)
    if need is not None and (raw.shape[0] < 1 + (n_inp + need if need else 0) or (proc is not None and proc.shape[0] < 1 + need)):
        raise cabi.LadeHipError(f"emit_rows: candidate row {need} lies outside the step's rows (raw {tuple(raw.shape)}, n_inp={n_inp})")
    call("lade_emit_rows", ptr(desc), ptr(raw), raw.stride(0), dtype_code(raw), n_inp, gs, ptr(proc), 0 if proc is None else proc.stride(0),
         ptr(ctl), harr, n_idx, raw.shape[1])
