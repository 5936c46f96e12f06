// Per-token scores / logits of generate(): the rows that decided the tokens one step emitted, appended to the caller's [tokens][V] fp32
// buffers in emission order (include/lade_hip.h, "emitted rows").
//
// The destinations live in a device descriptor (`desc`: two pointers, capacity, row stride, row counter), never in kernel arguments: a
// captured step appends through whatever the descriptor holds at replay, so a new generate() call only rewrites it.  Which rows a greedy
// step emitted is known on the device alone (ctl[N_ACCEPT], ctl[MAX_HIT_IDX] of the post-step): the row kernel reads them there.  It is a
// copy of at most (gs + 1) rows - latency bound: every thread issues all of its 16-byte loads, then stores.  The counter is advanced by a
// one-thread launch BEHIND the row kernel (every work-group of the row kernel reads the old value; no flag, no waiting between groups).
#include "common.hpp"

namespace lade {

// which rows: n < 0 = read the control block; otherwise n tokens, token k >= 1 from candidate cand[k] (passed by value into the launch)
struct EmitIdx {
    int32_t n;
    int32_t cand[LADE_MAX_LEVEL];
};

__device__ __forceinline__ int emit_count(const int32_t* ctl, const EmitIdx& idx, int gs) {
    const int n = idx.n >= 0 ? idx.n : ctl[LADE_CTL_N_ACCEPT];
    return min(max(n, 0), gs + 1);
}

__global__ void emit_init_kernel(int64_t* desc, float* scores, float* logits, int64_t cap_rows, int64_t ld) {
    desc[LADE_EMIT_SCORES] = (int64_t)scores;
    desc[LADE_EMIT_LOGITS] = (int64_t)logits;
    desc[LADE_EMIT_CAP] = cap_rows;
    desc[LADE_EMIT_LD] = ld;
    desc[LADE_EMIT_COUNT] = 0;
}

__global__ void emit_advance_kernel(int64_t* desc, const int32_t* ctl, EmitIdx idx, int gs) {
    desc[LADE_EMIT_COUNT] += emit_count(ctl, idx, gs);
}

constexpr int EMIT_THREADS = 256;
constexpr int EMIT_UNROLL = 4;      // 16-byte loads of the raw row per thread, all in flight before the first store

// grid: (gs + 1 token slots) x (column blocks of EMIT_THREADS * EMIT_UNROLL vectors).  PROC: scores come from the processed fp32 rows.
template <typename T, bool PROC>
__global__ __launch_bounds__(EMIT_THREADS) void emit_rows_kernel(const int64_t* desc, const void* raw, int64_t raw_ld, int n_inp, int gs,
                                                                 const float* proc, int64_t proc_ld, const int32_t* ctl, EmitIdx idx, int V) {
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= emit_count(ctl, idx, gs)) return;                   // a slot at or above the accepted count
    const int64_t drow = desc[LADE_EMIT_COUNT] + k, dld = desc[LADE_EMIT_LD];
    if (drow < 0 || drow >= desc[LADE_EMIT_CAP] || dld < V) return;      // beyond the capacity: not written (the counter still advances)
    int c = idx.n >= 0 ? idx.cand[k] : ctl[LADE_CTL_MAX_HIT_IDX];
    c = min(max(c, 0), LADE_MAX_GUESS_SET - 1);
    // token 0: the out row; token k >= 1: position k-1 of candidate c (raw rows carry the n_inp window rows between, proc rows do not)
    const int64_t cand_row = (int64_t)c * gs + (k - 1);
    const int64_t rrow = k == 0 ? 0 : 1 + n_inp + cand_row;
    const int64_t prow = k == 0 ? 0 : 1 + cand_row;
    float* sc = (float*)desc[LADE_EMIT_SCORES];
    float* lg = (float*)desc[LADE_EMIT_LOGITS];
    if (sc) sc += drow * dld;
    if (lg) lg += drow * dld;
    constexpr bool is16 = !__is_same(T, F32);
    constexpr int VEC = is16 ? 8 : 4;           // elements per 16-byte load of the raw row
    const size_t ebytes = is16 ? 2 : 4;
    const char* rp = (const char*)raw + (size_t)rrow * raw_ld * ebytes;
    const float* pp = PROC ? proc + (size_t)prow * proc_ld : nullptr;
    const bool use_proc = PROC && sc;
    const bool aligned = (((size_t)rp | (size_t)sc | (size_t)lg | (use_proc ? (size_t)pp : 0)) & 15) == 0;
    const int vend = aligned ? (V / VEC) * VEC : 0;
    const int b0 = blockIdx.y * (EMIT_THREADS * EMIT_UNROLL * VEC);
    const int b1 = min(b0 + EMIT_THREADS * EMIT_UNROLL * VEC, V);

    if (b0 < vend) {                            // (uniform) clamped addresses: every load is unconditional and issued before the first store
        uint4 ru[EMIT_UNROLL];
        float4 pu[EMIT_UNROLL][VEC / 4];
#pragma unroll
        for (int u = 0; u < EMIT_UNROLL; ++u) {
            const int i = min(b0 + (u * EMIT_THREADS + tid) * VEC, vend - VEC);
            ru[u] = *reinterpret_cast<const uint4*>(rp + (size_t)i * ebytes);
        }
#pragma unroll
        for (int u = 0; u < EMIT_UNROLL; ++u) {
            const int i = min(b0 + (u * EMIT_THREADS + tid) * VEC, vend - VEC);
#pragma unroll
            for (int q = 0; q < VEC / 4; ++q) pu[u][q] = use_proc ? *reinterpret_cast<const float4*>(pp + i + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < EMIT_UNROLL; ++u) {
            const int i = b0 + (u * EMIT_THREADS + tid) * VEC;
            if (i < vend) {
                const uint32_t w[4] = {ru[u].x, ru[u].y, ru[u].z, ru[u].w};
                float4 f[VEC / 4];
                if constexpr (is16) {           // widened like .to(float32): exact
                    f[0] = make_float4(to_f32<T>((uint16_t)(w[0] & 0xffffu)), to_f32<T>((uint16_t)(w[0] >> 16)),
                                       to_f32<T>((uint16_t)(w[1] & 0xffffu)), to_f32<T>((uint16_t)(w[1] >> 16)));
                    f[1] = make_float4(to_f32<T>((uint16_t)(w[2] & 0xffffu)), to_f32<T>((uint16_t)(w[2] >> 16)),
                                       to_f32<T>((uint16_t)(w[3] & 0xffffu)), to_f32<T>((uint16_t)(w[3] >> 16)));
                } else {
                    f[0] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
                }
#pragma unroll
                for (int q = 0; q < VEC / 4; ++q) {
                    if (lg) *reinterpret_cast<float4*>(lg + i + 4 * q) = f[q];
                    if (sc) *reinterpret_cast<float4*>(sc + i + 4 * q) = use_proc ? pu[u][q] : f[q];
                }
            }
        }
    }
    // scalar tail: the columns behind the last whole vector, or the whole block of a row whose addresses are not 16-byte aligned
    for (int i = max(b0, vend) + tid; i < b1; i += EMIT_THREADS) {
        float v;
        if constexpr (is16) v = to_f32<T>(((const uint16_t*)rp)[i]);
        else v = ((const float*)rp)[i];
        const float s = use_proc ? pp[i] : v;
        if (lg) lg[i] = v;
        if (sc) sc[i] = s;
    }
}

template <typename T>
static void launch_emit(dim3 grid, hipStream_t st, const int64_t* desc, const void* raw, int64_t raw_ld, int n_inp, int gs, const float* proc,
                        int64_t proc_ld, const int32_t* ctl, const EmitIdx& idx, int V) {
    if (proc) hipLaunchKernelGGL((emit_rows_kernel<T, true>), grid, dim3(EMIT_THREADS), 0, st, desc, raw, raw_ld, n_inp, gs, proc, proc_ld, ctl, idx, V);
    else hipLaunchKernelGGL((emit_rows_kernel<T, false>), grid, dim3(EMIT_THREADS), 0, st, desc, raw, raw_ld, n_inp, gs, proc, proc_ld, ctl, idx, V);
}

}  // namespace lade

using namespace lade;

extern "C" int lade_emit_init(int64_t* desc, float* scores_buf, float* logits_buf, int64_t cap_rows, int32_t V, void* stream) {
    LADE_REQUIRE(desc, LADE_E_ARG, "lade_emit_init: null descriptor");
    LADE_REQUIRE(V > 0 && cap_rows >= 0, LADE_E_ARG, "lade_emit_init: V=%d cap_rows=%lld", V, (long long)cap_rows);
    LADE_REQUIRE(scores_buf || logits_buf, LADE_E_ARG, "lade_emit_init: both destinations are null");
    hipLaunchKernelGGL(emit_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, desc, scores_buf, logits_buf, cap_rows, (int64_t)V);
    return check_launch("lade_emit_init");
}

extern "C" int lade_emit_rows(int64_t* desc, const void* raw, int64_t raw_ld, int32_t raw_dtype, int32_t n_inp, int32_t gs, const float* proc,
                              int64_t proc_ld, const int32_t* ctl, const int32_t* idx, int32_t n_idx, int32_t V, void* stream) {
    LADE_REQUIRE(desc && raw, LADE_E_ARG, "lade_emit_rows: null %s", desc ? "raw rows" : "descriptor");
    LADE_REQUIRE(V > 0 && raw_ld >= V && n_inp >= 0 && gs > 0 && gs < LADE_MAX_LEVEL && (!proc || proc_ld >= V), LADE_E_ARG,
                 "lade_emit_rows: V=%d raw_ld=%lld proc_ld=%lld n_inp=%d gs=%d", V, (long long)raw_ld, (long long)proc_ld, n_inp, gs);
    LADE_REQUIRE(raw_dtype == LADE_BF16 || raw_dtype == LADE_F16 || raw_dtype == LADE_F32, LADE_E_DTYPE, "lade_emit_rows: dtype=%d", raw_dtype);
    EmitIdx e = {};
    e.n = -1;
    if (idx) {
        LADE_REQUIRE(n_idx >= 1 && n_idx <= gs + 1, LADE_E_ARG, "lade_emit_rows: n_idx=%d (1..gs + 1 = %d)", n_idx, gs + 1);
        e.n = n_idx;
        for (int k = 0; k < n_idx; ++k) {
            LADE_REQUIRE(idx[k] >= 0 && idx[k] < LADE_MAX_GUESS_SET, LADE_E_ARG, "lade_emit_rows: idx[%d]=%d (candidate 0..%d)", k, idx[k],
                         LADE_MAX_GUESS_SET - 1);
            e.cand[k] = idx[k];
        }
    } else {
        LADE_REQUIRE(ctl, LADE_E_ARG, "lade_emit_rows: neither idx nor a control block");
    }
    const int vec = raw_dtype == LADE_F32 ? 4 : 8;
    const dim3 grid(gs + 1, cdiv(V, EMIT_THREADS * EMIT_UNROLL * vec));
    hipStream_t st = (hipStream_t)stream;
    switch (raw_dtype) {
        case LADE_BF16: launch_emit<BF16>(grid, st, desc, raw, raw_ld, n_inp, gs, proc, proc_ld, ctl, e, V); break;
        case LADE_F16: launch_emit<F16>(grid, st, desc, raw, raw_ld, n_inp, gs, proc, proc_ld, ctl, e, V); break;
        default: launch_emit<F32>(grid, st, desc, raw, raw_ld, n_inp, gs, proc, proc_ld, ctl, e, V); break;
    }
    const int rc = check_launch("lade_emit_rows");
    if (rc != 0) return rc;
    hipLaunchKernelGGL(emit_advance_kernel, dim3(1), dim3(1), 0, st, desc, ctl, e, gs);
    return check_launch("lade_emit_rows");
}
