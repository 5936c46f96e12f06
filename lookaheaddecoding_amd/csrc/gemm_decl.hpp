// Shared between the C entry points (gemm.hip) and the per-dtype translation units of the skinny GEMM (gemm_bf16.hip, gemm_f16.hip).
#pragma once
#include "common.hpp"

namespace lade {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int G_BK = 64;          // K depth of one LDS tile (128-byte rows)

struct GemmK {
    const uint16_t* A;     // [M][lda]
    const uint16_t* W;     // [N][ldw], or [K/64][N][64] (w_ts != 0)
    uint16_t* C;           // [M][ldc] model dtype (n_split == 1)
    float* Cpart;          // [n_split][M][N] fp32 (n_split > 1)
    int64_t lda, ldw, ldc;
    int64_t w_ts;          // 0: W is row-major [N][ldw];  64 N: W is K-tile-major [K/64][N][64] (elements between the K tiles of a row)
    int M, N, K, n_split;
    int n_stage;           // LDS ring depth of this launch (0: the shape's default)
    int dbg;               // ablation switches for tools/gemm_ablate.py (LADE_DEBUG=gemm_dbg=<bits>): 1 = no output stores, 4 = no LDS reads / MFMA
    int epi;               // n_split == 1 only: 0 = C = A.W^T;  1 = SwiGLU over interleaved gate / up rows, C is [M][N/2];
                           // 2 = row argmax: no C, Cpart holds one (value, column) pair per row and column block
};

// What the qkv GEMM's fused tail needs beside GemmK (gemm_qkv_rope.hip): the arguments of lade_rope_kv_append on partials, plus the ticket
// counters of the pair hand-off.  The two work-groups that share an (n-block, m-block) each leave their fp32 tile in Cpart (in accumulator
// order: a private hand-off layout, not [split][M][N]); the second to arrive sums both in split order, rounds once, rotates q and k and writes
// q_out / the K cache / the V^T cache.
struct RopeK {
    const int32_t* positions;      // [M] gathered position ids
    const uint16_t* cos_tab;       // [max_pos][d]
    const uint16_t* sin_tab;
    uint16_t* q_out;               // [M][H*d]
    uint16_t* k_cache;             // [Hkv][S_max][d]
    uint16_t* vt_cache;            // [Hkv][d][S_max]
    const int32_t* dyn_P;          // nullable: the cache length read from the device
    int32_t* tickets;              // [n-blocks x m-blocks], zero between launches (the second arriver leaves its counter at zero)
    int P, H, Hkv, d, S_max, max_pos;
};

// Weight row that the fused qkv kernel streams into row n of its tile order.  A rotation pair is (i, i + d/2) of a q or k head; in tile order every
// 32-row MFMA block of such a head is [16 rows i = 16 b .. 16 b + 15 | their partners i + d/2] (the interleave of the fused gate/up weight), so a
// lane's accumulators e and e + 8 are one pair and a work-group's tile - any multiple of 32 rows - holds whole pairs.  V rows stay in place.  The
// map is applied where the weight DMA forms its addresses (16 consecutive rows stay consecutive: every 1-KiB piece is still one contiguous KiB of
// the K-tile-major weight), so no second weight layout exists and every other kernel reads wqkv as it always did.  d % 32 == 0.
__host__ __device__ inline int qkv_pair_row(int n, int H, int Hkv, int d) {
    const int h = n / d, r = n - h * d;
    if (h >= H + Hkv) return n;
    const int b = r >> 5, q = r & 31;
    return h * d + (q < 16 ? 16 * b + q : (d >> 1) + 16 * b + (q - 16));
}

// what a group of the shape table answers when the wave grid is not one of its shapes: outside the LADE_E_* range (<= 0), so that a real
// failure of the launch (LADE_E_ARG: the ring does not fit the LDS; LADE_E_LAUNCH) is never taken for it
constexpr int GEMM_NOT_IN_TABLE = 1;

// launch the kernel built for this wave grid (mw x ng waves compute, mt x nt MFMA tiles each); GEMM_NOT_IN_TABLE when it is not in the shape table
int gemm_dispatch_bf16(const GemmK& g, hipStream_t st, int mw, int mt, int ng, int nt);
int gemm_dispatch_f16(const GemmK& g, hipStream_t st, int mw, int mt, int ng, int nt);
// the same for the fused qkv + RoPE + KV append kernel (n_split == 2; dtype LADE_BF16 | LADE_F16): built for the 96-row weight blocks of the 32 .. 128-row classes
int gemm_rope_dispatch(int dtype, const GemmK& g, const RopeK& r, hipStream_t st, int mw, int mt, int ng, int nt);

}  // namespace lade
