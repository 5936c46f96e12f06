// Skinny weight-streaming GEMM for the decode step:  C[M,N] = A[M,K] . W[N,K]^T,  M <= 256 per row block (a work-group holds every
// activation row of the step, so the weights are streamed once whatever M is).
//
// Reference: the nn.Linear projections of the step (q/k/v/o, gate/up/down, lm_head;
// lade/models/modeling_llama.py:360-380, 492-494, 558, 1541) - SURVEY.md 8(f) rank 2.  With M = T <= 240 rows
// the GEMM is a stream of the weight matrix: bound by HBM (and, per CU, by the ~55-68 GB/s one CU can ingest from HBM), so
// the weight bytes must be spread over all 256 CUs.  Work-group = (BN weight rows) x (one K slice) x (one row
// block); the weight tile and the activation tile of each 64-deep K step arrive by LDS-DMA into a 3-stage ring,
// eight waves hold the C^T tile in MFMA accumulators (lane = one activation row, like the attention kernel),
// split-K partials are fp32 and are summed in a fixed order (deterministic) by lade_splitk_reduce or by the
// consumer kernel.
#include "common.hpp"
#include <cstdlib>

#include "gemm_decl.hpp"

namespace lade {

template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* part, uint16_t* C, int64_t ldc, int M, int N, int n_split) {
    const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int m = blockIdx.y;
    if (i >= N) return;
    float4 a = *reinterpret_cast<const float4*>(part + (size_t)m * N + i);
    for (int s = 1; s < n_split; ++s) {
        const float4 b = *reinterpret_cast<const float4*>(part + ((size_t)s * M + m) * N + i);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    u32x2 w;
    w[0] = pack2<T>(a.x, a.y);
    w[1] = pack2<T>(a.z, a.w);
    *reinterpret_cast<u32x2*>(C + (size_t)m * ldc + i) = w;
}

// output chunk c (16 bytes) of the K-tile-major weight: c = (kt * N + n) * 8 + j  <-  W[n][64 kt + 8 j ..]
__global__ __launch_bounds__(256) void weight_to_ktile_kernel(const uint16_t* W, int64_t ldw, uint16_t* Wkt, int N, int K) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (int64_t)N * (K / 8)) return;
    const int j = (int)(c & 7);
    const int64_t row = c >> 3;                     // kt * N + n
    const int kt = (int)(row / N), n = (int)(row - (int64_t)kt * N);
    *reinterpret_cast<u32x4*>(Wkt + c * 8) = *reinterpret_cast<const u32x4*>(W + (size_t)n * ldw + (size_t)kt * G_BK + j * 8);
}

// the inverse: row-major chunk c = n * (K/8) + kc  <-  Wkt[(kc/8) * N + n][8 (kc % 8) ..]
__global__ __launch_bounds__(256) void weight_from_ktile_kernel(const uint16_t* Wkt, uint16_t* W, int64_t ldw, int N, int K) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cpr = K / 8;
    if (c >= (int64_t)N * cpr) return;
    const int n = (int)(c / cpr), kc = (int)(c - (int64_t)n * cpr);
    *reinterpret_cast<u32x4*>(W + (size_t)n * ldw + (size_t)kc * 8) =
        *reinterpret_cast<const u32x4*>(Wkt + ((size_t)(kc >> 3) * N + n) * G_BK + (kc & 7) * 8);
}

}  // namespace lade

using namespace lade;

// bn: weight rows per work-group (32..256); mb: 32-row activation blocks per work-group (1..4; 0 = by M); mt: m-blocks per
// wave (1 | 2 | 3 | 4, divides mb; 0 = 1); nt: 32-row weight tiles per wave (1..4; 0 = spread the tiles over as many n-groups
// as there are waves).  The waves form an (mb/mt) x (bn/32/nt) grid.  Only the shapes in the table of gemm_kernel.hpp are built.
static int gemm_skinny(const void* A, int64_t lda, const void* W, int64_t ldw, bool ktile, void* C, int64_t ldc, float* Cpart,
                       int32_t M, int32_t N, int32_t K, int32_t n_split, int32_t bn, int32_t mb, int32_t mt, int32_t nt, int32_t ring,
                       int32_t epilogue, int32_t dtype, void* stream) {
    LADE_REQUIRE(ring == 0 || (ring >= 2 && ring <= 6) || ring == 8, LADE_E_ARG, "lade_gemm_skinny: ring=%d (0 = default; loops are compiled for rings of 2, 3, 4, 5, 6 and 8 stages)", ring);
    LADE_REQUIRE(epilogue == 0 || (epilogue == 1 && n_split == 1 && N % 32 == 0 && C != nullptr) || (epilogue == 2 && n_split == 1 && Cpart != nullptr), LADE_E_ARG,
                 "lade_gemm_skinny: epilogue=%d needs n_split == 1 and N %% 32 == 0 + an output matrix (1) or the pair buffer in Cpart (2)", epilogue);
    LADE_REQUIRE(A && W && M > 0 && N > 0 && K > 0 && n_split >= 1, LADE_E_ARG, "lade_gemm_skinny: M=%d N=%d K=%d split=%d", M, N, K, n_split);
    LADE_REQUIRE(K % G_BK == 0 && lda % 8 == 0 && ldw % 8 == 0 && N % 8 == 0, LADE_E_ARG,
                 "lade_gemm_skinny: K=%d must be a multiple of %d, strides / N multiples of 8", K, G_BK);
    LADE_REQUIRE(epilogue == 2 || (n_split == 1 ? (C != nullptr && ldc % (epilogue ? 4 : 8) == 0) : (Cpart != nullptr)), LADE_E_ARG, "lade_gemm_skinny: missing output buffer");
    LADE_REQUIRE(dtype == LADE_BF16 || dtype == LADE_F16, LADE_E_DTYPE, "lade_gemm_skinny: dtype=%d", dtype);
    if (mb == 0) mb = M <= 32 ? 1 : (M <= 64 ? 2 : (M <= 96 ? 3 : (M <= 128 ? 4 : (M <= 160 ? 5 : (M <= 192 ? 6 : 8)))));
    if (mt == 0) mt = mb <= 4 ? 1 : (mb == 5 ? 5 : mb / 2);
    if (mb > 4 && nt == 0) nt = 1;
    LADE_REQUIRE(mb >= 1 && mb <= 8 && mt >= 1 && mt <= 5 && mb % mt == 0, LADE_E_ARG, "lade_gemm_skinny: mb=%d mt=%d", mb, mt);
    // 192 / 256-row work-groups: the activation tile leaves room for <= 128 weight rows per stage of a 3-stage ring; the wider
    // shapes are the double-buffered 256 x 256 tile (mb = 8, bn = 256, nt = 2 | 4) and the 160-row class (mb = 5: one wave holds all five
    // m-blocks, the eight waves - or four with two n-tiles each - lie along N: 256 weight rows + 160 activation rows = 52 KB per stage, three stages)
    if (mb > 5 && bn > 128 && !(mb == 8 && bn == 256 && (nt == 2 || nt == 4))) {
        // (the argmax epilogue's pair buffer is indexed by the CALLER's ceil(N / bn): a silently narrower block would shift every row's pairs)
        LADE_REQUIRE(epilogue != 2, LADE_E_ARG, "lade_gemm_skinny: epilogue 2 with mb=%d needs bn <= 128 (got %d): the pair buffer's stride is ceil(N / bn)", mb, bn);
        bn = 128;
    }
    const int mw = mb / mt;
    const int tiles = bn <= 32 ? 1 : (bn <= 64 ? 2 : (bn <= 96 ? 3 : (bn <= 128 ? 4 : (bn <= 192 ? 6 : (bn <= 224 ? 7 : 8)))));      // 32-row weight tiles per work-group
    if (nt == 0) {                                     // default: as many n-groups as waves allow
        const int ng_max = 8 / mw > 0 ? 8 / mw : 1;
        nt = 1;
        while (tiles / nt > ng_max || tiles % nt != 0) ++nt;
    }
    LADE_REQUIRE(nt >= 1 && nt <= 4 && tiles % nt == 0, LADE_E_ARG, "lade_gemm_skinny: bn=%d (%d tiles) nt=%d", bn, tiles, nt);
    const int ng = tiles / nt;
    GemmK g;
    g.A = (const uint16_t*)A; g.W = (const uint16_t*)W; g.C = (uint16_t*)C; g.Cpart = Cpart;
    g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.n_split = n_split;
    g.w_ts = ktile ? (int64_t)N * G_BK : 0;
    { static int dbg = -1; if (dbg < 0) dbg = debug_int("gemm_dbg"); g.dbg = dbg; }
    g.epi = epilogue;
    g.n_stage = ring;
    hipStream_t st = (hipStream_t)stream;
    const int rc = dtype == LADE_BF16 ? gemm_dispatch_bf16(g, st, mw, mt, ng, nt) : gemm_dispatch_f16(g, st, mw, mt, ng, nt);
    if (rc != GEMM_NOT_IN_TABLE) return rc;          // launched, or failed with its own code and message (launch_gemm, check_launch)
    LADE_REQUIRE(false, LADE_E_ARG, "lade_gemm_skinny: no kernel for mb=%d mt=%d bn=%d nt=%d (wave grid %d x %d)", mb, mt, bn, nt, mw, ng);
}

extern "C" int lade_gemm_skinny(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, float* Cpart,
                                int32_t M, int32_t N, int32_t K, int32_t n_split, int32_t bn, int32_t mb, int32_t mt, int32_t nt,
                                int32_t ring, int32_t epilogue, int32_t dtype, void* stream) {
    return gemm_skinny(A, lda, W, ldw, false, C, ldc, Cpart, M, N, K, n_split, bn, mb, mt, nt, ring, epilogue, dtype, stream);
}

// The same GEMM on a weight stored K-tile-major: Wkt[K/64][N][64] (lade_weight_to_ktile).  Same arithmetic in the same order, so the
// results are bit-identical to lade_gemm_skinny on the row-major weight; only the addresses the weight DMA reads differ.
extern "C" int lade_gemm_skinny_kt(const void* A, int64_t lda, const void* Wkt, void* C, int64_t ldc, float* Cpart,
                                   int32_t M, int32_t N, int32_t K, int32_t n_split, int32_t bn, int32_t mb, int32_t mt, int32_t nt,
                                   int32_t ring, int32_t epilogue, int32_t dtype, void* stream) {
    return gemm_skinny(A, lda, Wkt, 8, true, C, ldc, Cpart, M, N, K, n_split, bn, mb, mt, nt, ring, epilogue, dtype, stream);
}

// The qkv projection with two K splits, finished in its own launch: the two work-groups of an (n-block, m-block) hand their fp32 tiles to each
// other through Cpart and the second to arrive sums, rounds, rotates q and k and appends K / V^T (gemm_kernel.hpp: gemm_rope_epilogue) - what
// lade_gemm_skinny(_kt) with n_split = 2 followed by lade_rope_kv_append on the partials computes, bit for bit.  Explicit launch shape only
// (mb, mt, nt >= 1, bn a multiple of 32); a shape the fused kernel is not built for is LADE_E_ARG, and the caller keeps the two launches.
extern "C" int lade_gemm_qkv_rope(const void* A, int64_t lda, const void* W, int64_t ldw, int32_t ktile, float* Cpart, int64_t cpart_elems,
                                  int32_t* tickets, int32_t n_tickets, int32_t M, int32_t N, int32_t K, int32_t bn, int32_t mb, int32_t mt, int32_t nt,
                                  int32_t ring, const lade_qkv_rope_args* rope, int32_t dtype, void* stream) {
    LADE_REQUIRE(ring == 0 || (ring >= 2 && ring <= 6) || ring == 8, LADE_E_ARG, "lade_gemm_qkv_rope: ring=%d", ring);
    LADE_REQUIRE(A && W && Cpart && tickets && rope && M > 0 && N > 0 && K > 0, LADE_E_ARG, "lade_gemm_qkv_rope: null pointer or M=%d N=%d K=%d", M, N, K);
    LADE_REQUIRE(K % G_BK == 0 && K / G_BK >= 2 && lda % 8 == 0 && ldw % 8 == 0, LADE_E_ARG,
                 "lade_gemm_qkv_rope: K=%d must be a multiple of %d with a K tile per split, strides multiples of 8", K, G_BK);
    LADE_REQUIRE(dtype == LADE_BF16 || dtype == LADE_F16, LADE_E_DTYPE, "lade_gemm_qkv_rope: dtype=%d", dtype);
    LADE_REQUIRE(bn >= 32 && bn <= 256 && bn % 32 == 0 && mb >= 1 && mb <= 4 && mt >= 1 && mb % mt == 0 && nt >= 1 && (bn / 32) % nt == 0, LADE_E_ARG,
                 "lade_gemm_qkv_rope: bn=%d mb=%d mt=%d nt=%d", bn, mb, mt, nt);
    const lade_qkv_rope_args& a = *rope;
    LADE_REQUIRE(a.q_out && a.positions && a.cos_tab && a.sin_tab && a.k_cache && a.vt_cache, LADE_E_ARG, "lade_gemm_qkv_rope: null pointer in the RoPE arguments");
    // a rotation pair must sit in one 32-row MFMA block: heads of whole blocks
    LADE_REQUIRE(a.H > 0 && a.Hkv > 0 && a.d > 0 && a.d % 32 == 0 && a.d <= 256 && (int64_t)(a.H + 2 * a.Hkv) * a.d == N, LADE_E_ARG,
                 "lade_gemm_qkv_rope: H=%d Hkv=%d d=%d do not make N=%d rows of whole 32-row blocks", a.H, a.Hkv, a.d, N);
    LADE_REQUIRE(a.P >= 0 && a.S_max > 0 && a.max_pos > 0 && (int64_t)a.P + M <= a.S_max, LADE_E_ARG, "lade_gemm_qkv_rope: T=%d P=%d S_max=%d max_pos=%d", M, a.P,
                 a.S_max, a.max_pos);
    const int bm = 32 * mb;
    const int64_t n_tiles = (int64_t)cdiv(N, bn) * cdiv(M, bm);
    LADE_REQUIRE(n_tiles <= n_tickets && n_tiles * 2 * bm * bn <= cpart_elems, LADE_E_ARG,
                 "lade_gemm_qkv_rope: %lld tiles of %d x %d need %lld fp32 of hand-off space and as many tickets as tiles (got %lld, %d)", (long long)n_tiles, bm, bn,
                 (long long)(n_tiles * 2 * bm * bn), (long long)cpart_elems, n_tickets);
    GemmK g;
    g.A = (const uint16_t*)A; g.W = (const uint16_t*)W; g.C = nullptr; g.Cpart = Cpart;
    g.lda = lda; g.ldw = ktile ? 8 : ldw; g.ldc = 0; g.M = M; g.N = N; g.K = K; g.n_split = 2;
    g.w_ts = ktile ? (int64_t)N * G_BK : 0;
    g.dbg = 0;
    g.epi = 0;
    g.n_stage = ring;
    RopeK r;
    r.positions = a.positions; r.cos_tab = (const uint16_t*)a.cos_tab; r.sin_tab = (const uint16_t*)a.sin_tab; r.q_out = (uint16_t*)a.q_out;
    r.k_cache = (uint16_t*)a.k_cache; r.vt_cache = (uint16_t*)a.vt_cache; r.dyn_P = a.dyn_P; r.tickets = tickets;
    r.P = a.P; r.H = a.H; r.Hkv = a.Hkv; r.d = a.d; r.S_max = a.S_max; r.max_pos = a.max_pos;
    const int rc = gemm_rope_dispatch(dtype, g, r, (hipStream_t)stream, mb / mt, mt, bn / 32 / nt, nt);
    if (rc != GEMM_NOT_IN_TABLE) return rc;
    LADE_REQUIRE(false, LADE_E_ARG, "lade_gemm_qkv_rope: no fused kernel for mb=%d mt=%d bn=%d nt=%d", mb, mt, bn, nt);
}

// tile-order row -> weight row of the fused qkv kernel (gemm_decl.hpp: qkv_pair_row), for callers and tests that want the order itself; -1 = bad arguments
extern "C" int lade_qkv_pair_row(int32_t n, int32_t H, int32_t Hkv, int32_t d) {
    if (H <= 0 || Hkv <= 0 || d <= 0 || d % 32 != 0 || n < 0 || n >= (H + 2 * Hkv) * d) return -1;
    return qkv_pair_row(n, H, Hkv, d);
}

// Wkt[kt][n][0..63] = W[n][64 kt .. 64 kt + 63]: one 16-byte chunk per thread, a wave writes 1 KiB contiguous
extern "C" int lade_weight_to_ktile(const void* W, int64_t ldw, void* Wkt, int32_t N, int32_t K, int32_t dtype, void* stream) {
    LADE_REQUIRE(W && Wkt && W != Wkt && N > 0 && K > 0 && K % G_BK == 0 && ldw >= K && ldw % 8 == 0, LADE_E_ARG,
                 "lade_weight_to_ktile: N=%d K=%d ldw=%lld (K must be a multiple of %d, out of place)", N, K, (long long)ldw, G_BK);
    LADE_REQUIRE(dtype == LADE_BF16 || dtype == LADE_F16, LADE_E_DTYPE, "lade_weight_to_ktile: dtype=%d", dtype);
    const int64_t chunks = (int64_t)N * (K / 8);
    LADE_REQUIRE(chunks / 256 + 1 < (int64_t)1 << 31, LADE_E_LIMIT, "lade_weight_to_ktile: N=%d K=%d too large", N, K);
    hipLaunchKernelGGL(weight_to_ktile_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)W, ldw, (uint16_t*)Wkt, N, K);
    return check_launch("lade_weight_to_ktile");
}

// W[n][64 kt + j] = Wkt[kt][n][j]: the row-major matrix a library GEMM needs (prefill chunks of a model whose weights are held
// K-tile-major only), written into a caller-provided scratch
extern "C" int lade_weight_from_ktile(const void* Wkt, void* W, int64_t ldw, int32_t N, int32_t K, int32_t dtype, void* stream) {
    LADE_REQUIRE(W && Wkt && W != Wkt && N > 0 && K > 0 && K % G_BK == 0 && ldw >= K && ldw % 8 == 0, LADE_E_ARG,
                 "lade_weight_from_ktile: N=%d K=%d ldw=%lld (K must be a multiple of %d, out of place)", N, K, (long long)ldw, G_BK);
    LADE_REQUIRE(dtype == LADE_BF16 || dtype == LADE_F16, LADE_E_DTYPE, "lade_weight_from_ktile: dtype=%d", dtype);
    const int64_t chunks = (int64_t)N * (K / 8);
    LADE_REQUIRE(chunks / 256 + 1 < (int64_t)1 << 31, LADE_E_LIMIT, "lade_weight_from_ktile: N=%d K=%d too large", N, K);
    hipLaunchKernelGGL(weight_from_ktile_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)Wkt, (uint16_t*)W, ldw, N, K);
    return check_launch("lade_weight_from_ktile");
}

extern "C" int lade_splitk_reduce(const float* part, void* C, int64_t ldc, int32_t M, int32_t N, int32_t n_split, int32_t dtype, void* stream) {
    LADE_REQUIRE(part && C && M > 0 && N > 0 && N % 4 == 0 && n_split >= 1, LADE_E_ARG, "lade_splitk_reduce: bad args");
    dim3 grid(cdiv(N / 4, 256), M);
    if (dtype == LADE_BF16) hipLaunchKernelGGL(splitk_reduce_kernel<BF16>, grid, dim3(256), 0, (hipStream_t)stream, part, (uint16_t*)C, ldc, M, N, n_split);
    else if (dtype == LADE_F16) hipLaunchKernelGGL(splitk_reduce_kernel<F16>, grid, dim3(256), 0, (hipStream_t)stream, part, (uint16_t*)C, ldc, M, N, n_split);
    else LADE_REQUIRE(false, LADE_E_DTYPE, "lade_splitk_reduce: dtype=%d", dtype);
    return check_launch("lade_splitk_reduce");
}
