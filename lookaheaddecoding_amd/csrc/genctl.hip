// Generation controls of a lookahead step on the device: HF's repetition penalty and min-length family applied to the logits rows
// of one step, each row with the input_ids it would have in plain decoding (include/lade_hip.h, "generation controls").
//
// The controls live in a device block (`gen`: penalty, min_len, the masked EOS ids, the seen-set bitmap), so a captured step reads
// them at replay.  A row kernel is one 1024-thread work-group per logits row: the row's penalised set (seen set + the candidate's
// prefix) is staged in LDS as a bitmap, then one pass of 16-byte loads applies the penalty and the EOS mask in registers and reduces the
// argmax (wave-64 shuffles, then one LDS round over the 16 waves) - optionally also storing the processed fp32 row for sampling.
#include "common.hpp"

namespace lade {

__global__ __launch_bounds__(1024) void gen_ctl_init_kernel(int32_t* gen, int V, float penalty, float inv_penalty, int min_len, EosIds eos,
                                                            const int32_t* prompt, int n_prompt) {
    uint32_t* seen = (uint32_t*)(gen + LADE_GEN_SEEN);
    const int nw = (V + 31) >> 5;
    for (int i = threadIdx.x; i < nw; i += blockDim.x) seen[i] = 0u;
    if (threadIdx.x < LADE_GEN_SEEN) {
        const int w = threadIdx.x;
        int32_t v = 0;
        if (w == LADE_GEN_PENALTY) v = __float_as_int(penalty);
        else if (w == LADE_GEN_INV_PENALTY) v = __float_as_int(inv_penalty);
        else if (w == LADE_GEN_MIN_LEN) v = min_len;
        else if (w == LADE_GEN_N_EOS) v = eos.n;
        else if (w == LADE_GEN_VOCAB) v = V;
        else if (w >= LADE_GEN_EOS) v = w - LADE_GEN_EOS < eos.n ? eos.id[w - LADE_GEN_EOS] : -1;
        gen[w] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_prompt; i += blockDim.x) {
        const int t = prompt[i];
        if (t >= 0 && t < V) atomicOr(&seen[t >> 5], 1u << (t & 31));
    }
}

// the tokens the last post-step accepted (ctl[HITS .. + N_ACCEPT]) join the seen set
__global__ __launch_bounds__(64) void gen_ctl_update_kernel(int32_t* gen, const int32_t* ctl) {
    const int n = min(ctl[LADE_CTL_N_ACCEPT], LADE_MAX_LEVEL);
    const int V = gen[LADE_GEN_VOCAB];
    const int lane = threadIdx.x;
    if (lane < n) {
        const int t = ctl[LADE_CTL_HITS + lane];
        if (t >= 0 && t < V) atomicOr((uint32_t*)(gen + LADE_GEN_SEEN) + (t >> 5), 1u << (t & 31));
    }
}

template <typename T>
__device__ __forceinline__ float ld_one(const void* p, size_t i) {
    if constexpr (__is_same(T, F32)) return ((const float*)p)[i];
    else return to_f32<T>(((const uint16_t*)p)[i]);
}

// One work-group per row of [out | n_inp window rows | candidate rows].  ROWS: also the processed fp32 out row and candidate rows.
template <typename T, bool ROWS>
__global__ __launch_bounds__(1024) void gen_rows_kernel(const void* __restrict__ logits, int64_t ld, int V, int n_inp, int gs,
                                                        const int32_t* __restrict__ gen, const int32_t* __restrict__ ctl,
                                                        const int32_t* __restrict__ guess, const int32_t* __restrict__ pos,
                                                        const int32_t* __restrict__ sel, int32_t* __restrict__ am,
                                                        float* __restrict__ rows_out) {
    extern __shared__ uint32_t bits[];           // the row's penalised set, ceil(V/32) words
    __shared__ float sb[16];
    __shared__ int si[16];
    const int row = blockIdx.x, tid = threadIdx.x;
    int c = -1, j = 0;                          // candidate / position of a candidate row
    if (row > n_inp) {
        const int k = row - 1 - n_inp;
        c = k / gs;
        j = k - c * gs;
    }
    if (c >= 0 && c >= ctl[LADE_CTL_G]) {      // padded candidate slot: never read
        if (tid == 0) am[row] = 0;
        return;
    }
    const float pen = __int_as_float(gen[LADE_GEN_PENALTY]);
    const float inv = __int_as_float(gen[LADE_GEN_INV_PENALTY]);
    const int L = pos[sel ? sel[row] : row] + 1;         // the sequence length at which this row predicts
    EosIds eos;
    eos.n = L < gen[LADE_GEN_MIN_LEN] ? min(max(gen[LADE_GEN_N_EOS], 0), LADE_GEN_MAX_EOS) : 0;
#pragma unroll
    for (int e = 0; e < LADE_GEN_MAX_EOS; ++e) eos.id[e] = gen[LADE_GEN_EOS + e];
    const int nw = (V + 31) >> 5;
    const uint32_t* seen = (const uint32_t*)(gen + LADE_GEN_SEEN);
    for (int i = tid; i < nw; i += 1024) bits[i] = seen[i];
    __syncthreads();
    if (c >= 0 && tid <= j) {                   // the candidate's own prefix guess[c][0..j] (a repeat sets its bit once)
        const int t = guess[c * gs + tid];
        if (t >= 0 && t < V) atomicOr(&bits[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    float* orow = nullptr;
    if (ROWS && (row == 0 || c >= 0)) orow = rows_out + (size_t)(row == 0 ? 0 : 1 + c * gs + j) * V;

    // HF's order: the penalty (gather / where / scatter: once per distinct token), then the min-length mask
    auto proc = [&](float v, int i, uint32_t w) -> float {
        if ((w >> (i & 31)) & 1u) v = v < 0.f ? v * pen : v * inv;
        if (eos.has(i)) v = -INFINITY;
        return v;
    };
    float best = -INFINITY;
    int bi = 0x7fffffff;
    auto upd = [&](float v, int i) {
        if (argmax_better(v, i, best, bi)) { best = v; bi = i; }
    };
    constexpr bool is16 = !__is_same(T, F32);
    constexpr int VEC = is16 ? 8 : 4;           // elements per 16-byte load; VEC divides 32, so a load's bits sit in one word
    const size_t ebytes = is16 ? 2 : 4;
    const size_t base = (size_t)row * ld;
    const bool aligned = (((size_t)logits + base * ebytes) & 15) == 0 && (!orow || ((size_t)orow & 15) == 0);
    int vend = 0;
    if (aligned) {
        vend = (V / VEC) * VEC;
        for (int i0 = tid * VEC; i0 < vend; i0 += 4 * 1024 * VEC) {
            uint4 uu[4];                        // four 16-byte loads in flight
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = min(i0 + k * 1024 * VEC, vend - VEC);
                uu[k] = *reinterpret_cast<const uint4*>((const char*)logits + (base + i) * ebytes);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + k * 1024 * VEC;
                if (i < vend) {
                    const uint32_t w[4] = {uu[k].x, uu[k].y, uu[k].z, uu[k].w};
                    const uint32_t wb = bits[i >> 5];
                    float f[VEC];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (is16) {
                            f[2 * e] = to_f32<T>((uint16_t)(w[e] & 0xffffu));
                            f[2 * e + 1] = to_f32<T>((uint16_t)(w[e] >> 16));
                        } else {
                            f[e] = __uint_as_float(w[e]);
                        }
                    }
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        f[e] = proc(f[e], i + e, wb);
                        upd(f[e], i + e);
                    }
                    if (ROWS && orow) {
#pragma unroll
                        for (int q = 0; q < VEC / 4; ++q)
                            *reinterpret_cast<float4*>(orow + i + 4 * q) = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
                    }
                }
            }
        }
    }
    for (int i = vend + tid; i < V; i += 1024) {
        const float v = proc(ld_one<T>(logits, base + i), i, bits[i >> 5]);
        upd(v, i);
        if (ROWS && orow) orow[i] = v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (oi != 0x7fffffff && argmax_better(ob, oi, best, bi)) { best = ob; bi = oi; }
    }
    if ((tid & 63) == 0) { sb[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (si[w] != 0x7fffffff && argmax_better(sb[w], si[w], best, bi)) { best = sb[w]; bi = si[w]; }
        am[row] = bi;
    }
}

template <bool ROWS>
static int launch_rows(const char* fn, const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, int32_t n_inp, int32_t gs,
                       const int32_t* gen, const int32_t* ctl, const int32_t* guess, const int32_t* pos, const int32_t* sel, int32_t* am,
                       float* rows_out, void* stream) {
    LADE_REQUIRE(logits && gen && ctl && pos && am && (!ROWS || rows_out), LADE_E_ARG, "%s: null pointer", fn);
    LADE_REQUIRE(V > 0 && V <= LADE_GEN_MAX_VOCAB && ld >= V && rows >= 1 && n_inp >= 0 && rows >= 1 + n_inp && gs > 0 && gs < LADE_MAX_LEVEL,
                 LADE_E_ARG, "%s: rows=%d V=%d ld=%lld n_inp=%d gs=%d (V <= %d)", fn, rows, V, (long long)ld, n_inp, gs, LADE_GEN_MAX_VOCAB);
    const int cand_rows = rows - 1 - n_inp;
    LADE_REQUIRE(cand_rows % gs == 0 && cand_rows / gs <= LADE_MAX_GUESS_SET && (cand_rows == 0 || guess), LADE_E_ARG,
                 "%s: %d candidate rows are not whole candidates of gs=%d (<= %d), or no guess buffer", fn, cand_rows, gs, LADE_MAX_GUESS_SET);
    const size_t lds = (size_t)((V + 31) / 32) * 4;
    hipStream_t st = (hipStream_t)stream;
    const bool known = dispatch_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL((gen_rows_kernel<decltype(t), ROWS>), dim3(rows), dim3(1024), lds, st, logits, ld, V, n_inp, gs, gen, ctl, guess, pos, sel, am, rows_out);
    });
    LADE_REQUIRE(known, LADE_E_DTYPE, "%s: dtype=%d", fn, dtype);
    return check_launch(fn);
}

}  // namespace lade

using namespace lade;

extern "C" int lade_gen_ctl_init(int32_t* gen, int32_t V, double penalty, int32_t min_len, const int32_t* eos_ids, int32_t n_eos,
                                 const int32_t* prompt, int32_t n_prompt, void* stream) {
    LADE_REQUIRE(gen && V > 0 && V <= LADE_GEN_MAX_VOCAB, LADE_E_ARG, "lade_gen_ctl_init: gen=%p V=%d (V <= %d)", (void*)gen, V, LADE_GEN_MAX_VOCAB);
    LADE_REQUIRE(penalty > 0.0 && penalty < 1e30 && min_len >= 0, LADE_E_ARG, "lade_gen_ctl_init: penalty=%g min_len=%d", penalty, min_len);
    LADE_REQUIRE(n_eos >= 0 && n_eos <= LADE_GEN_MAX_EOS && (n_eos == 0 || eos_ids), LADE_E_ARG, "lade_gen_ctl_init: n_eos=%d (0..%d)", n_eos,
                 LADE_GEN_MAX_EOS);
    LADE_REQUIRE(n_prompt >= 0 && (n_prompt == 0 || prompt), LADE_E_ARG, "lade_gen_ctl_init: n_prompt=%d without prompt tokens", n_prompt);
    EosIds eos = {};
    eos.n = n_eos;
    for (int e = 0; e < n_eos; ++e) {
        LADE_REQUIRE(eos_ids[e] >= 0, LADE_E_ARG, "lade_gen_ctl_init: eos_ids[%d]=%d is negative", e, eos_ids[e]);
        eos.id[e] = eos_ids[e];
    }
    // torch on the device: `scores * penalty` multiplies by (float)penalty; `scores / penalty` multiplies by the reciprocal, taken in double
    // and then rounded to fp32 (measured: 1.0 / 1.05 rounds differently from 1.0f / 1.05f, and true division matches neither)
    const float pen = (float)penalty, inv = (float)(1.0 / penalty);
    hipLaunchKernelGGL(gen_ctl_init_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, gen, V, pen, inv, min_len, eos, prompt, n_prompt);
    return check_launch("lade_gen_ctl_init");
}

extern "C" int lade_gen_ctl_update(int32_t* gen, const int32_t* ctl, void* stream) {
    LADE_REQUIRE(gen && ctl, LADE_E_ARG, "lade_gen_ctl_update: null pointer");
    hipLaunchKernelGGL(gen_ctl_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, gen, ctl);
    return check_launch("lade_gen_ctl_update");
}

extern "C" int lade_gen_argmax(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, int32_t n_inp, int32_t gs,
                               const int32_t* gen, const int32_t* ctl, const int32_t* guess, const int32_t* pos, const int32_t* sel,
                               int32_t* am, void* stream) {
    return launch_rows<false>("lade_gen_argmax", logits, ld, rows, V, dtype, n_inp, gs, gen, ctl, guess, pos, sel, am, nullptr, stream);
}

extern "C" int lade_gen_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, int32_t n_inp, int32_t gs,
                             const int32_t* gen, const int32_t* ctl, const int32_t* guess, const int32_t* pos, const int32_t* sel,
                             int32_t* am, float* rows_out, void* stream) {
    return launch_rows<true>("lade_gen_rows", logits, ld, rows, V, dtype, n_inp, gs, gen, ctl, guess, pos, sel, am, rows_out, stream);
}
