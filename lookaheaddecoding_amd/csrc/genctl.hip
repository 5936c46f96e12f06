// Generation controls of a lookahead step on the device: HF's repetition penalty and min-length family applied to the logits rows
// of one step, each row with the input_ids it would have in plain decoding (include/lade_hip.h, "generation controls").
//
// The controls live in a device block (`gen`: penalty, min_len, the masked EOS ids, the seen-set bitmap), so a captured step reads
// them at replay.  A row kernel is one 1024-thread work-group per logits row: the row's penalised set (seen set + the candidate's
// prefix) is staged in LDS as a bitmap, then one pass of 16-byte loads applies the penalty and the EOS mask in registers and reduces the
// argmax (wave-64 shuffles, then one LDS round over the 16 waves) - optionally also storing the processed fp32 row for sampling.
//
// Token constraints (HF's suppress_tokens / begin_suppress_tokens / sequence_bias / bad_words_ids) live in a second block whose address
// `gen` holds (include/lade_hip.h, "token constraints").  With a block attached, a row first resolves which sequence entries fire on its
// input_ids - one thread per entry over the block's tail and the candidate's prefix - into a (token, summed bias) list in LDS, and stages
// a second bitmap of the tokens that need more than the common path (banned, begin-banned at this length, biased); the pass itself stays
// one pass of 16-byte loads.  Without a block the row runs the instructions it ran before the block existed.
#include <cmath>
#include <type_traits>
#include <vector>

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

constexpr int CONS_TAIL_SLOTS = LADE_GEN_MAX_SEQ_LEN - 1;       // a sequence entry's prefix is at most this long

// the constraint block attached to `gen` (null: none)
__device__ __forceinline__ const int32_t* cons_of(const int32_t* gen) {
    return (const int32_t*)(((uint64_t)(uint32_t)gen[LADE_GEN_CONS + 1] << 32) | (uint64_t)(uint32_t)gen[LADE_GEN_CONS]);
}

// the tail = the last prompt tokens (right-aligned), and the block's address into gen
__global__ __launch_bounds__(64) void gen_cons_attach_kernel(int32_t* gen, int32_t* cons, const int32_t* prompt, int n_prompt) {
    const int lane = threadIdx.x;
    if (lane < CONS_TAIL_SLOTS) {
        const int src = n_prompt - CONS_TAIL_SLOTS + lane;
        cons[LADE_CONS_TAIL + lane] = src >= 0 ? prompt[src] : -1;
    }
    if (lane == 0) {
        cons[LADE_CONS_TAIL_N] = min(n_prompt, CONS_TAIL_SLOTS);
        gen[LADE_GEN_CONS] = (int32_t)(uint32_t)((uint64_t)cons & 0xffffffffull);
        gen[LADE_GEN_CONS + 1] = (int32_t)(uint32_t)((uint64_t)cons >> 32);
    }
}

// the tokens the last post-step accepted (ctl[HITS .. + N_ACCEPT]) join the seen set and shift into an attached constraint block's tail
__global__ __launch_bounds__(64) void gen_ctl_update_kernel(int32_t* gen, const int32_t* ctl) {
    const int n = max(min(ctl[LADE_CTL_N_ACCEPT], LADE_MAX_LEVEL), 0);
    const int V = gen[LADE_GEN_VOCAB];
    const int lane = threadIdx.x;
    if (lane < n) {
        const int t = ctl[LADE_CTL_HITS + lane];
        if (t >= 0 && t < V) atomicOr((uint32_t*)(gen + LADE_GEN_SEEN) + (t >> 5), 1u << (t & 31));
    }
    int32_t* cons = const_cast<int32_t*>(cons_of(gen));
    if (!cons) return;
    int32_t moved = 0;
    if (lane < CONS_TAIL_SLOTS) {
        const int src = lane + n;                   // < CONS_TAIL_SLOTS + LADE_MAX_LEVEL
        moved = src < CONS_TAIL_SLOTS ? cons[LADE_CONS_TAIL + src] : ctl[LADE_CTL_HITS + src - CONS_TAIL_SLOTS];
    }
    __syncthreads();
    if (lane < CONS_TAIL_SLOTS) cons[LADE_CONS_TAIL + lane] = moved;
    if (lane == 0) cons[LADE_CONS_TAIL_N] = min(max(cons[LADE_CONS_TAIL_N], 0) + n, CONS_TAIL_SLOTS);
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
    extern __shared__ uint32_t bits[];           // the row's penalised set, ceil(V/32) words; with room for constraints (launch_rows) behind
                                                 // it: the special-token bitmap, the same size, and the fired entries' tokens and biases
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

    // ---- token constraints: which entries fire on this row's input_ids, summed per end token in table order ----
    const int32_t* cons = V <= LADE_GEN_CONS_MAX_VOCAB && V == gen[LADE_GEN_VOCAB] ? cons_of(gen) : nullptr;      // (the block's bitmaps are sized by the V it was written for)
    uint32_t* spec = bits + nw;                 // bit t: token t is banned on this row, or a fired entry ends in it
    int32_t* f_tok = (int32_t*)(spec + nw);     // per entry: the end token whose sum the entry holds, or -1
    float* f_bias = (float*)(f_tok + LADE_GEN_MAX_SEQ);
    const uint32_t* ban = nullptr;
    const uint32_t* begin_ban = nullptr;        // set on a row at the begin index only
    int n_eval = 0;
    float zero_bias = -0.0f;                    // x + -0.0f is x for every x; HF's `scores + bias` adds +0.0f where nothing fires
    if (cons) {
        const bool window_row = row > 0 && c < 0;       // window rows: the bans and the length-1 entries only
        const int n_seq = min(max(cons[LADE_CONS_N_SEQ], 0), LADE_GEN_MAX_SEQ);
        n_eval = window_row ? min(max(cons[LADE_CONS_N_ONE], 0), n_seq) : n_seq;
        ban = (const uint32_t*)(cons + LADE_CONS_BAN);
        if (!window_row && cons[LADE_CONS_BEGIN_INDEX] >= 0 && L == cons[LADE_CONS_BEGIN_INDEX]) begin_ban = ban + nw;
        if (cons[LADE_CONS_FLAGS] & LADE_CONS_F_ADD) zero_bias = 0.0f;
        for (int i = tid; i < nw; i += 1024) spec[i] = ban[i] | (begin_ban ? begin_ban[i] : 0u);
        int my_tok = -1;
        float my_bias = 0.f;
        if (tid < n_eval) {
            const int32_t* off = cons + LADE_CONS_OFF;
            const int32_t* tok = cons + LADE_CONS_TOK;
            const int32_t* tail = cons + LADE_CONS_TAIL;
            const int o0 = off[tid], n = off[tid + 1] - o0;
            bool fire = o0 >= 0 && n >= 1 && n <= LADE_GEN_MAX_SEQ_LEN && o0 + n <= LADE_GEN_MAX_SEQ * LADE_GEN_MAX_SEQ_LEN;
            if (fire && n > 1) {
                const int tail_n = min(max(cons[LADE_CONS_TAIL_N], 0), CONS_TAIL_SLOTS);
                const int len = tail_n + (c >= 0 ? j + 1 : 0);          // the context at hand: the tail, then guess[c][0..j]
                fire = L >= n && n - 1 <= len;
                for (int m = 0; fire && m < n - 1; ++m) {
                    const int p = len - (n - 1) + m;
                    const int t = p < tail_n ? tail[CONS_TAIL_SLOTS - tail_n + p] : guess[c * gs + p - tail_n];
                    fire = t == tok[o0 + m];
                }
            }
            if (fire) {
                const int t = tok[o0 + n - 1];
                if (t >= 0 && t < V) { my_tok = t; my_bias = __int_as_float(cons[LADE_CONS_BIAS + tid]); }
            }
        }
        f_tok[tid] = my_tok;
        f_bias[tid] = my_bias;
        __syncthreads();
        bool first = my_tok >= 0;               // the first fired entry of its end token sums all of them, in table order
        for (int e = 0; first && e < tid; ++e) first = f_tok[e] != my_tok;
        float sum = 0.f;
        if (first) {
            for (int e = tid; e < n_eval; ++e)
                if (f_tok[e] == my_tok) sum += f_bias[e];
            atomicOr(&spec[my_tok >> 5], 1u << (my_tok & 31));
        }
        __syncthreads();
        if (my_tok >= 0) {
            if (first) f_bias[tid] = sum;
            else f_tok[tid] = -1;
        }
        __syncthreads();
    }
    // a token of the special bitmap: banned (the result is -inf whatever else applies), or the end of fired entries (their sum)
    auto special = [&](int i, float& b) -> bool {
        const uint32_t m = 1u << (i & 31);
        if ((ban[i >> 5] | (begin_ban ? begin_ban[i >> 5] : 0u)) & m) return true;
        for (int e = 0; e < n_eval; ++e)
            if (f_tok[e] == i) { b = f_bias[e]; break; }
        return false;
    };

    // HF's order: the sequence-bias sum, the penalty (gather / where / scatter: once per distinct token), then the -inf masks (bans, min length)
    auto proc = [&](auto has_cons, float v, int i, uint32_t w, uint32_t ws) -> float {
        bool banned = false;
        if constexpr (decltype(has_cons)::value) {
            float b = zero_bias;
            if ((ws >> (i & 31)) & 1u) banned = special(i, b);
            v += b;
        }
        if ((w >> (i & 31)) & 1u) v = v < 0.f ? v * pen : v * inv;
        if (eos.has(i) || banned) v = -INFINITY;
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
    auto pass = [&](auto has_cons) {        // the one pass over the row; has_cons: with the constraint stages compiled in
        constexpr bool CONS = decltype(has_cons)::value;
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
                        const uint32_t ws = CONS ? spec[i >> 5] : 0u;
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
                            f[e] = proc(has_cons, f[e], i + e, wb, ws);
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
            const float v = proc(has_cons, ld_one<T>(logits, base + i), i, bits[i >> 5], CONS ? spec[i >> 5] : 0u);
            upd(v, i);
            if (ROWS && orow) orow[i] = v;
        }
    };
    if (cons) pass(std::true_type{});
    else pass(std::false_type{});
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
    // room for a constraint block that may be attached at replay: the second bitmap and the fired-entry list (lade_gen_constraints_init
    // refuses a vocabulary for which they would not fit)
    const size_t lds = (size_t)((V + 31) / 32) * 4 * (V <= LADE_GEN_CONS_MAX_VOCAB ? 2 : 1) + (V <= LADE_GEN_CONS_MAX_VOCAB ? LADE_GEN_MAX_SEQ * 8 : 0);
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

extern "C" int lade_gen_constraints_init(int32_t* gen, int32_t* cons, int32_t V, const int32_t* ban_ids, int32_t n_ban, const int32_t* begin_ids,
                                         int32_t n_begin, int32_t begin_index, const int32_t* seq_off, const int32_t* seq_tok,
                                         const float* seq_bias, int32_t n_seq, int32_t add_bias, const int32_t* prompt, int32_t n_prompt,
                                         void* stream) {
    const char* fn = "lade_gen_constraints_init";
    LADE_REQUIRE(gen && cons, LADE_E_ARG, "%s: null pointer (gen=%p cons=%p)", fn, (void*)gen, (void*)cons);
    LADE_REQUIRE(V > 0 && V <= LADE_GEN_CONS_MAX_VOCAB, LADE_E_ARG, "%s: V=%d (constraints take V <= LADE_GEN_CONS_MAX_VOCAB = %d)", fn, V,
                 LADE_GEN_CONS_MAX_VOCAB);
    LADE_REQUIRE(n_ban >= 0 && (n_ban == 0 || ban_ids) && n_begin >= 0 && (n_begin == 0 || (begin_ids && begin_index >= 0)), LADE_E_ARG,
                 "%s: n_ban=%d n_begin=%d begin_index=%d, or an id array is null", fn, n_ban, n_begin, begin_index);
    LADE_REQUIRE(n_seq >= 0 && n_seq <= LADE_GEN_MAX_SEQ, LADE_E_ARG, "%s: %d sequence entries (at most LADE_GEN_MAX_SEQ = %d)", fn, n_seq,
                 LADE_GEN_MAX_SEQ);
    LADE_REQUIRE(n_seq == 0 || (seq_off && seq_tok && seq_bias), LADE_E_ARG, "%s: n_seq=%d without the entry arrays", fn, n_seq);
    LADE_REQUIRE(n_prompt >= 0 && (n_prompt == 0 || prompt), LADE_E_ARG, "%s: n_prompt=%d without prompt tokens", fn, n_prompt);
    for (int e = 0; e < n_seq; ++e) {
        const int n = seq_off[e + 1] - seq_off[e];
        LADE_REQUIRE(seq_off[e] >= 0 && n >= 1, LADE_E_ARG, "%s: entry %d is empty or its offsets run backwards", fn, e);
        LADE_REQUIRE(n <= LADE_GEN_MAX_SEQ_LEN, LADE_E_ARG, "%s: entry %d has %d tokens (at most LADE_GEN_MAX_SEQ_LEN = %d)", fn, e, n,
                     LADE_GEN_MAX_SEQ_LEN);
        for (int m = 0; m < n; ++m) {
            const int t = seq_tok[seq_off[e] + m];
            LADE_REQUIRE(t >= 0 && t < V, LADE_E_ARG, "%s: entry %d holds token %d outside the vocabulary of %d", fn, e, t, V);
        }
        const float b = seq_bias[e];
        LADE_REQUIRE(!std::isnan(b) && !(std::isinf(b) && b > 0.f), LADE_E_ARG, "%s: entry %d has bias %g (finite or -inf only)", fn, e, (double)b);
    }
    for (int i = 0; i < n_ban; ++i) LADE_REQUIRE(ban_ids[i] >= 0, LADE_E_ARG, "%s: ban_ids[%d]=%d is negative", fn, i, ban_ids[i]);
    for (int i = 0; i < n_begin; ++i) LADE_REQUIRE(begin_ids[i] >= 0, LADE_E_ARG, "%s: begin_ids[%d]=%d is negative", fn, i, begin_ids[i]);

    // the block is put together on the host and copied in one piece: the length-1 entries first, then the longer ones, each in the caller's order
    const int nw = (V + 31) / 32;
    std::vector<int32_t> blk((size_t)LADE_GEN_CONS_WORDS(V), 0);
    int n_out = 0, n_tok = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int e = 0; e < n_seq; ++e) {
            const int n = seq_off[e + 1] - seq_off[e];
            if ((n == 1) != (pass == 0)) continue;
            blk[LADE_CONS_OFF + n_out] = n_tok;
            for (int m = 0; m < n; ++m) blk[LADE_CONS_TOK + n_tok++] = seq_tok[seq_off[e] + m];
            uint32_t bits;
            __builtin_memcpy(&bits, &seq_bias[e], 4);
            blk[LADE_CONS_BIAS + n_out++] = (int32_t)bits;
        }
        if (pass == 0) blk[LADE_CONS_N_ONE] = n_out;
    }
    blk[LADE_CONS_OFF + n_out] = n_tok;
    blk[LADE_CONS_N_SEQ] = n_out;
    blk[LADE_CONS_BEGIN_INDEX] = n_begin > 0 ? begin_index : -1;
    blk[LADE_CONS_FLAGS] = add_bias ? LADE_CONS_F_ADD : 0;
    for (int i = 0; i < n_ban; ++i)
        if (ban_ids[i] < V) blk[LADE_CONS_BAN + (ban_ids[i] >> 5)] |= (int32_t)(1u << (ban_ids[i] & 31));
    for (int i = 0; i < n_begin; ++i)
        if (begin_ids[i] < V) blk[LADE_CONS_BAN + nw + (begin_ids[i] >> 5)] |= (int32_t)(1u << (begin_ids[i] & 31));
    hipStream_t st = (hipStream_t)stream;
    hipError_t err = hipMemcpyAsync(cons, blk.data(), blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    LADE_REQUIRE(err == hipSuccess, LADE_E_LAUNCH, "%s: copying the block: %s", fn, hipGetErrorString(err));
    hipLaunchKernelGGL(gen_cons_attach_kernel, dim3(1), dim3(64), 0, st, gen, cons, prompt, n_prompt);
    const int rc = check_launch(fn);
    err = hipStreamSynchronize(st);             // `blk` is the copy's source until the stream has passed it
    LADE_REQUIRE(err == hipSuccess, LADE_E_LAUNCH, "%s: %s", fn, hipGetErrorString(err));
    return rc;
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
