// The attention core that attn.hip (decode: lade_attn_fwd) and attn_prefill.hip (lade_attn_prefill) share - included by these two only.
//
// Both kernels compute "transposed" (S^T = K Q^T, O^T = V^T P^T on v_mfma_f32_32x32x16, one query row per lane) and keep one online-softmax
// state per 32-key half of a 64-key tile; lade_attn_prefill is specified to return the bits lade_attn_fwd returns with n_splits = 1.  What
// decides those bits has ONE definition here, and both kernels call it: the scaling of the scores, the online-softmax update with its lazy
// rescale, the packing of P, and the merge of the two key halves.  The LDS tile layout, the LDS-DMA stream of K / V^T tiles and the zeroing
// of a chunk's stale V^T tail are here for the same reason.  Where a multiply is rounded on its own and where it is fused is part of the
// result: the arithmetic is spelled with explicit rounding (__fmul_rn, __fsub_rn, __builtin_fmaf) and compiled with contraction off (the
// pragma at the top of each function - with this toolchain __fmul_rn(x, y) is x * y, which the default -ffp-contract may still fuse).
// What stays in each kernel: the mask source, the fragment addressing, rings / barriers / waits and every sched_barrier.
#pragma once
#include "common.hpp"

namespace lade {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int KT = 64;        // keys per tile
constexpr float NEG_BIG = -1.0e30f;     // initial running max
constexpr float MASKED = -3.0e30f;      // masked score: 2^(MASKED - m) == 0 even while m is still NEG_BIG
constexpr float RESCALE_THR = 8.0f;    // log2 units: the running max is only raised when it grows by more

// ---- LDS tiles ------------------------------------------------------------------------------
// K tile [KT keys][D] and V^T tile [D][KT keys] are filled by LDS-DMA (global_load_lds, 16 B per
// lane, no VGPR staging).  The DMA writes LDS linearly (wave-uniform base + lane*16), so the XOR
// swizzle that keeps the ds_read_b128 fragment reads conflict-free is applied to the per-lane
// SOURCE address and to the read address (never to the destination).
template <int ROW_BYTES>
__device__ __forceinline__ int swz16(int row) {          // 16-B chunk swizzle of a row-major tile
    constexpr int CPR = ROW_BYTES / 16;                  // chunks per row
    constexpr int RPB = 256 / ROW_BYTES > 0 ? 256 / ROW_BYTES : 1;   // rows per 256-B bank row
    return (row / RPB) & (CPR - 1);
}
template <int ROW_BYTES>
__device__ __forceinline__ int tile_off(int row, int c16) { return row * ROW_BYTES + ((c16 ^ swz16<ROW_BYTES>(row)) << 4); }

// MFMA row index rho (0..31) of an S^T sub-tile <-> key kappa within the sub-tile.  With
// kappa = (rho&3) | ((rho>>3)&3)<<2 | ((rho>>2)&1)<<4 the 16 S^T values a lane holds are the 16
// CONTIGUOUS keys 16*hi .. 16*hi+15, so each PV k-step needs 8 contiguous keys of V^T = one 16-B read.
__device__ __forceinline__ int kappa(int rho) { return (rho & 3) | (((rho >> 3) & 3) << 2) | (((rho >> 2) & 1) << 4); }

template <typename T> struct Mfma;
template <> struct Mfma<BF16> {
    __device__ static __forceinline__ f32x16 run(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mfma<F16> {
    __device__ static __forceinline__ f32x16 run(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};

// Work-group barrier that the compiler cannot move memory operations across.  The raw
// __builtin_amdgcn_s_barrier() is IntrNoMem: LDS reads that follow it in the source may be scheduled
// BEFORE it (observed: Q fragments read ahead of the barrier that publishes other waves' LDS-DMA).
__device__ __forceinline__ void wg_barrier() { asm volatile("s_barrier" ::: "memory"); }

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ---- K / V^T stream ---------------------------------------------------------------------------
// One wave's share of a tile's LDS-DMA in a work-group of NW waves: the per-lane byte offsets of its 1-KiB pieces inside a K tile / a V^T
// tile, resolved ONCE: a piece of a tile is then (wave-uniform tile base) + (32-bit lane offset) - one scalar add per piece instead of a
// 64-bit multiply-add per lane.  Which tile goes to which stage, and when, is the kernel's ring logic.
template <int D, int NW>
struct KvStream {
    static constexpr int KPW = KT * D * 2 / 1024 / NW;       // 1-KiB DMA pieces per wave per tile
    static constexpr int VPW = D * KT * 2 / 1024 / NW;
    static constexpr int K_CPR = D / 8;                      // 16-B chunks per K row
    static_assert(KPW >= 1 && VPW >= 1, "every wave moves at least one piece of every tile");
    int wave;
    uint32_t k_off[KPW], v_off[VPW];

    __device__ __forceinline__ KvStream(int wave_, int lane, int S_max) : wave(wave_) {
#pragma unroll
        for (int i = 0; i < KPW; ++i) {
            const int piece = wave * KPW + i;
            const int row = piece * (64 / K_CPR) + lane / K_CPR;
            const int c = (lane % K_CPR) ^ swz16<2 * D>(row);
            k_off[i] = (uint32_t)(row * D + c * 8) * 2u;
        }
#pragma unroll
        for (int i = 0; i < VPW; ++i) {
            const int piece = wave * VPW + i;
            const int row = piece * 8 + (lane >> 3);
            const int c = (lane & 7) ^ swz16<2 * KT>(row);
            v_off[i] = ((uint32_t)row * (uint32_t)S_max + (uint32_t)(c * 8)) * 2u;      // < 2^32 while S_max < 2^24 (lade_attn_prefill's host check caps it at 2^22; lade_attn_fwd's does not cap it)
        }
    }
    // kt / vt: the tile's first K row / first V^T column of the KV head (wave uniform); ks / vs: its LDS tiles.
    // AUX: cache-policy bits of the loads (1 = sc0, 2 = nt, 16 = sc1)
    template <int AUX>
    __device__ __forceinline__ void issue(const unsigned char* kt, const unsigned char* vt, unsigned char* ks, unsigned char* vs) const {
#pragma unroll
        for (int i = 0; i < KPW; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kt + k_off[i]),
                                             (__attribute__((address_space(3))) void*)(ks + (wave * KPW + i) * 1024), 16, 0, AUX);
#pragma unroll
        for (int i = 0; i < VPW; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vt + v_off[i]),
                                             (__attribute__((address_space(3))) void*)(vs + (wave * VPW + i) * 1024), 16, 0, AUX);
    }
};

// The chunk's last tile: V^T columns of keys >= P+T (`first` = the first such key within the tile) hold stale bytes; zero them
// (0 * NaN would poison O).  Every thread of the work-group calls it; the caller waits and passes a barrier afterwards.
template <int D>
__device__ __forceinline__ void zero_stale_vt(unsigned char* vs, int first, int tid, int n_threads) {
    for (int idx = tid; idx < D * (KT - first); idx += n_threads) {
        const int row = idx / (KT - first), key = first + idx % (KT - first);
        *reinterpret_cast<uint16_t*>(vs + tile_off<2 * KT>(row, key >> 3) + (key & 7) * 2) = 0;
    }
}

// ---- arithmetic of one 32-key sub-tile ----------------------------------------------------------
// A lane's 16 scores into the log2 domain: a separately rounded multiply (the mask is a select applied after it, in the kernel)
__device__ __forceinline__ void scale_scores(f32x16& s, float scale_log2) {
#pragma clang fp contract(off)      // here and below: __fmul_rn is plain x * y in this HIP, so only this keeps the product out of an fma
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = __fmul_rn(s[e], scale_log2);
}

// Online softmax in the log2 domain on the scaled and masked scores of lane (q, hi): s becomes p = 2^(s - m), and (m, l, O^T) of the row's state
// move on.  The running max is raised only when it grows by more than RESCALE_THR for some row of the wave (a wave-uniform decision, in
// which every lane votes - padding lanes too): p stays <= 2^THR, harmless in the fp32 accumulators, and the O^T rescale is skipped on most tiles.
template <int DBLK>
__device__ __forceinline__ void softmax_update(f32x16& s, float& m_run, float& l_run, f32x16 (&oacc)[DBLK]) {
#pragma clang fp contract(off)
    float tmax = NEG_BIG;
#pragma unroll
    for (int e = 0; e < 16; ++e) tmax = fmaxf(tmax, s[e]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    if (__builtin_amdgcn_ballot_w64(tmax > m_run + RESCALE_THR) != 0ull) {
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f(__fsub_rn(m_run, m_new));
        m_run = m_new;
        l_run = __fmul_rn(l_run, alpha);
#pragma unroll
        for (int ii = 0; ii < DBLK; ++ii)
#pragma unroll
            for (int e = 0; e < 16; ++e) oacc[ii][e] = __fmul_rn(oacc[ii][e], alpha);
    }
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const float p = __builtin_amdgcn_exp2f(__fsub_rn(s[e], m_run));   // masked: 2^(-3e30 - m) = 0
        s[e] = p;
        psum += p;
    }
    l_run += psum;
}

// P^T B-operand fragments of the two PV k-steps, straight from the S^T accumulator layout: k-step jj = the lane's keys 8jj .. 8jj+7
template <typename T>
__device__ __forceinline__ void pack_p(f32x16 p, u32x4& pf0, u32x4& pf1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        pf0[e] = pack2<T>(p[2 * e], p[2 * e + 1]);
        pf1[e] = pack2<T>(p[8 + 2 * e], p[8 + 2 * e + 1]);
    }
}

// ---- merge of a row's two key halves ----------------------------------------------------------------
// Always in key-half order (half 0, half 1), whoever calls: identical mm and lsum on both sides.  lsum includes the lane ^ 32 add (the
// two lanes of a row); s0 / s1 carry the normalisation (rcp: 1 ulp; the result is rounded to 16 bits).
struct PairMerge { float mm, lsum, s0, s1; };
__device__ __forceinline__ PairMerge pair_merge(float m0, float l0, float m1, float l1) {
#pragma clang fp contract(off)
    PairMerge r;
    r.mm = fmaxf(m0, m1);
    const float a0 = __builtin_amdgcn_exp2f(__fsub_rn(m0, r.mm)), a1 = __builtin_amdgcn_exp2f(__fsub_rn(m1, r.mm));
    r.lsum = __builtin_fmaf(l0, a0, __fmul_rn(l1, a1));
    r.lsum += __shfl_xor(r.lsum, 32);
    const float inv = r.lsum > 0.f ? __builtin_amdgcn_rcpf(r.lsum) : 0.f;
    r.s0 = __fmul_rn(a0, inv);
    r.s1 = __fmul_rn(a1, inv);
    return r;
}
// one merged element: `own` is the half whose wave (decode) or d-block range (prefill) finishes this column
__device__ __forceinline__ float merged_elem(float o_own, float s_own, float o_oth, float s_oth) {
#pragma clang fp contract(off)
    return __builtin_fmaf(o_own, s_own, __fmul_rn(o_oth, s_oth));
}

}  // namespace lade
