// The fused qkv GEMM + RoPE + KV append kernel (gemm_kernel.hpp: gemm_qkv_rope_kernel) for both 16-bit dtypes: a translation unit of its own, so
// that the plain GEMM's shape table compiles exactly as it did.  Built for the wave grids the tuner picks for wqkv with two splits and 96-row
// weight blocks in the 32 .. 128-row classes; another grid is "not in the table" and the caller keeps the two-launch path.
#include "gemm_kernel.hpp"

namespace lade {

#define ROPE_SHAPE(MWv, MTv, NGv, NTv)                                                       \
    if (mw == MWv && mt == MTv && ng == NGv && nt == NTv)                                    \
        return dtype == LADE_BF16 ? launch_gemm_rope<BF16, MWv, MTv, NGv, NTv>(g, r, st) : launch_gemm_rope<F16, MWv, MTv, NGv, NTv>(g, r, st);

int gemm_rope_dispatch(int dtype, const GemmK& g, const RopeK& r, hipStream_t st, int mw, int mt, int ng, int nt) {
    /* 32 rows */  ROPE_SHAPE(1, 1, 3, 1)
    /* 64 rows */  ROPE_SHAPE(2, 1, 3, 1)
    /* 96 rows */  ROPE_SHAPE(1, 3, 3, 1)
    /* 128 rows */ ROPE_SHAPE(2, 2, 3, 1)
    return GEMM_NOT_IN_TABLE;
}
#undef ROPE_SHAPE

}  // namespace lade
