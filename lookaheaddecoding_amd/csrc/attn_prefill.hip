// One-pass causal attention for prefill chunks on gfx950 (MI355X): lade_attn_prefill.
//
// Replaces the reference's eager attention under the plain causal mask of a prompt (lade/models/modeling_llama.py:124-130 builds the mask,
// :520-541 apply it) for chunks of more than 256 rows.  attn.hip's kernel is built for the decode step - 60-240 query rows against a long
// cache, HBM bound, split over the KV axis and merged by a second launch.  A prefill chunk is the other regime: thousands of rows per head,
// arithmetic intensity far above the ridge, MFMA / VALU bound.  So the decomposition changes while the formulation stays:
//
//   * the transposed formulation of attn.hip: S^T = K Q^T, O^T = V^T P^T on v_mfma_f32_32x32x16, one query row per lane (the row statistics
//     are lane-local), kappa() key order, XOR-swizzled ds_read_b128 fragments, LDS-DMA ring - the shared formulation, and every piece of
//     arithmetic that decides an output bit, is attn_core.hpp's, which both kernels call;
//   * a work-group of 8 waves owns 256 rows of the (head-in-group, token) row space; wave w owns rows 32w .. 32w+31 and ALL 64 keys of every
//     tile: a K / V^T tile is filled and read once per 256 rows, and there is no key-part exchange at the end;
//   * no KV split and no partial buffers: row block rb of KV head kvh walks the tiles 0 .. (P + its last token) / 64 and writes `out`;
//   * Q never touches LDS: a lane's B-operand fragments are 16-byte global loads of its own row (D / 8 x 16 bytes per row, read once);
//   * ring of 3 stages, prefetch distance 2, ONE barrier per tile: the barrier that publishes tile i also says that every wave is done with
//     tile i - 1, whose stage the request of tile i + 2 then overwrites;
//   * two online-softmax states per row, one per 32-key half of a tile, merged at the end exactly as the decode kernel's two waves of a row
//     group merge theirs: the output equals lade_attn_fwd's single-launch form (n_splits = 1) bit for bit;
//   * tiles wholly below a wave's diagonal take the unmasked path, tiles wholly above it are skipped by that wave, tiles above the whole
//     block's diagonal are never requested;
//   * blocks are issued longest first (the latest rows of a chunk see the most keys), so the tail of the launch is short blocks.
#include <stdlib.h>

#include <type_traits>

#include "attn_core.hpp"

namespace lade {
namespace pf {

constexpr int NW = 8;                   // waves per work-group
constexpr int NTHR = 64 * NW;
constexpr int ROWS = 32 * NW;           // query rows per work-group
constexpr int NSTG = 3;                 // ring depth
// cache policy of the K / V stream (bits 1 = sc0, 2 = nt, 16 = sc1): the DEFAULT policy here, unlike the decode kernel's non-temporal stream -
// the row blocks of a KV head re-read the same tiles, and the L2 of their XCD is where they should find them
constexpr int KV_AUX = 0;

struct PrefillK {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* vt;
    uint16_t* out;
    int64_t q_row_stride, out_row_stride;
    int H, Hkv, S_max, n_rep, T, P, n_rb;
    float scale_log2;                   // scale * log2(e)
};

template <typename T, int D>
__global__ __launch_bounds__(NTHR) void attn_prefill_kernel(PrefillK a) {
    constexpr int KSTEPS = D / 16;                 // MFMA k-steps of S^T
    constexpr int DBLK = D / 32;                   // 32-row blocks of O^T
    constexpr int K_BYTES = KT * D * 2, V_BYTES = D * KT * 2, STAGE_BYTES = K_BYTES + V_BYTES;
    using Stream = KvStream<D, NW>;                // this wave's share of a tile's DMA
    constexpr int PIECES = Stream::KPW + Stream::VPW;      // per wave per tile

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // ring of NSTG x (K tile | V^T tile); reused for the store staging

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hi = lane >> 5;
    // longest blocks first: work-group g is row block n_rb - 1 - g / Hkv of KV head g % Hkv (consecutive ids go round the 8 XCDs: with Hkv a
    // multiple of 8 every row block of a KV head lands on one XCD and shares one L2 copy of its K / V stream, as in attn.hip)
    const int rbi = (int)blockIdx.x / a.Hkv;
    const int kvh = (int)blockIdx.x - rbi * a.Hkv;
    const int rb = a.n_rb - 1 - rbi;
    const int n_rep = a.n_rep, Tn = a.T, P = a.P;
    const int n_rows = n_rep * Tn;
    const int S_tot = P + Tn;

    // ---- this lane's query row.  Rows past the end (the chunk's last wave) are never stored, but they vote in the wave-uniform rescale
    // decision below: they behave exactly as in attn_fwd_kernel - row 0's q, every key of the tiles wholly inside the cache visible, every
    // other key masked - so that a launch equals lade_attn_fwd's single-launch form bit for bit in its partial wave too
    const int r = rb * ROWS + wave * 32 + ql;
    const bool valid = r < n_rows;
    const int rc = valid ? r : 0;
    const int hg = rc / Tn, t = rc - hg * Tn;
    const int qh = kvh * n_rep + hg;
    const int kmax = valid ? P + t : (P / KT) * KT - 1;       // last key this lane sees
    u32x4 qf[KSTEPS];                              // Q^T B-operand fragments: Q[row][kk*16 + hi*8 .. +8]
    {
        const uint16_t* qrow = a.q + (size_t)t * a.q_row_stride + (size_t)qh * D + hi * 8;
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) qf[kk] = *reinterpret_cast<const u32x4*>(qrow + kk * 16);
    }

    // ---- key range of the block and of this wave (all scalar)
    int n_tiles;
    {
        const int r0 = rb * ROWS, r1 = min(r0 + ROWS, n_rows) - 1;
        const int h0 = r0 / Tn, h1 = r1 / Tn;
        const int tmax = h0 != h1 ? Tn - 1 : r1 - h1 * Tn;
        n_tiles = (P + tmax + 1 + KT - 1) / KT;
    }
    const int w0 = rb * ROWS + wave * 32;
    const bool wave_live = w0 < n_rows;
    int w_subs = 0, w_full = 0;                    // 32-key sub-tiles this wave computes; the first w_full of them hold no masked key for any of its rows
    if (wave_live) {
        const int w1 = min(w0 + 31, n_rows - 1);
        const int h0 = w0 / Tn, h1 = w1 / Tn;
        const int tlo = h0 != h1 ? 0 : w0 - h0 * Tn, thi = h0 != h1 ? Tn - 1 : w1 - h1 * Tn;
        w_subs = min(2 * n_tiles, (P + thi + 1 + 31) / 32);
        w_full = (P + tlo + 1) / 32;
        if (w0 + 31 >= n_rows) w_full = min(w_full, (P / KT) * 2);      // a wave with padding lanes: they see the cache's whole tiles only
    }

    // ---- LDS-DMA stream of this KV head's K / V^T tiles
    const unsigned char* kbytes = reinterpret_cast<const unsigned char*>(a.k + (size_t)kvh * a.S_max * D);
    const unsigned char* vbytes = reinterpret_cast<const unsigned char*>(a.vt + (size_t)kvh * D * a.S_max);
    const Stream kv(wave, lane, a.S_max);
    auto issue_tile = [&](int tile, int stage) {
        unsigned char* ks = smem + stage * STAGE_BYTES;
        kv.template issue<KV_AUX>(kbytes + (size_t)tile * KT * D * 2, vbytes + (size_t)tile * KT * 2, ks, ks + K_BYTES);
    };
    issue_tile(0, 0);
    issue_tile(min(1, a.S_max / KT - 1), 1);       // unconditional (a one-tile block re-reads tile 0 or reads a tile it never computes): the wait below stays counted
    // the Q loads are complete, as far as the compiler is concerned, HERE (a counted wait that leaves the tiles in flight): a use of qf that it still
    // has to wait for inside the loop becomes s_waitcnt vmcnt(0) in front of every tile's first MFMA - which drains the ring's prefetch
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) asm volatile("" : "+v"(qf[kk]));

    // Two online-softmax states per row, one per 32-key half kh of every tile, merged at the end: the state of attn_fwd_kernel's 128-row
    // shape (there the two halves live in two waves), moved on by the same attn_core.hpp calls - lade_attn_prefill returns the bits
    // lade_attn_fwd returns with n_splits = 1 (tests/test_gpu_attn_prefill.py), so routing a chunk to this kernel changes no token.  The two
    // states are also two independent dependency chains for the scheduler.
    f32x16 oacc[2][DBLK];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < DBLK; ++i)
#pragma unroll
            for (int j = 0; j < 16; ++j) oacc[h][i][j] = 0.f;
    float m_run[2] = {NEG_BIG, NEG_BIG}, l_run[2] = {0.f, 0.f};
    // LDS fragment addresses: a swizzled chunk index is (constant ^ per-lane bits), and every row / stage / sub-tile offset is a multiple of the
    // swizzle's span - so ONE per-lane base per tile kind serves every fragment as (base + stage) ^ constant + constant, computed per tile
    // (left to the compiler, the loop-invariant addresses of every code path are kept live across the loop: > 60 registers)
    const int krow = kappa(ql);                    // LDS row (key within a 32-key sub-tile) of this lane's MFMA row
    const int kb_lane = krow * 2 * D + ((hi ^ swz16<2 * D>(krow)) << 4);
    const int vb_lane = K_BYTES + ql * 2 * KT + (((2 * hi) ^ swz16<2 * KT>(ql)) << 4);
    const float sc = a.scale_log2;

    // one 32-key sub-tile kh of a tile: S^T, online softmax in the log2 domain, O^T += V^T P^T.  The sub-tiles of a tile are independent
    // up to the running (m, l): the S^T MFMAs of the second run beside the softmax VALU work of the first
    // (`masked` is wave uniform and guards only the selects: two whole instantiations under an if / else made the compiler keep two copies of O^T)
    auto compute = [&](int kb, int vb, int k0, auto kh_c, bool masked) {
        constexpr int kh = decltype(kh_c)::value;
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
        {
            u32x4 kf[KSTEPS];
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) kf[kk] = *reinterpret_cast<const u32x4*>(smem + (kb ^ (kk << 5)) + kh * 32 * 2 * D);
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) s = Mfma<T>::run(kf[kk], qf[kk], s);
        }
        __builtin_amdgcn_sched_barrier(0);      // (keeps the next sub-tile's K fragments out of this one's register budget: no scratch)
        // V^T fragments of the first PV k-step are requested before the softmax VALU work
        u32x4 vf0[DBLK];
#pragma unroll
        for (int db = 0; db < DBLK; ++db) vf0[db] = *reinterpret_cast<const u32x4*>(smem + (vb ^ ((4 * kh) << 4)) + db * 32 * 2 * KT);
        // lane (q, hi) holds the scores of keys k0 + 32 kh + 16 hi + e
        scale_scores(s, sc);
        if (masked) {
            const int lim = kmax - k0 - 32 * kh - 16 * hi;           // key offset e is visible iff <= lim
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = (e <= lim) ? s[e] : MASKED;      // a select: NaN of rows that do not exist never gets further
        }
        softmax_update(s, m_run[kh], l_run[kh], oacc[kh]);
        // k-step jj = keys 32 kh + 16 hi + 8 jj + 0..7 = 16-byte chunk 4 kh + 2 hi + jj of a V^T row
        u32x4 vf1[DBLK];
#pragma unroll
        for (int db = 0; db < DBLK; ++db) vf1[db] = *reinterpret_cast<const u32x4*>(smem + (vb ^ ((4 * kh + 1) << 4)) + db * 32 * 2 * KT);
        u32x4 pf0, pf1;
        pack_p<T>(s, pf0, pf1);
#pragma unroll
        for (int db = 0; db < DBLK; ++db) oacc[kh][db] = Mfma<T>::run(vf0[db], pf0, oacc[kh][db]);
#pragma unroll
        for (int db = 0; db < DBLK; ++db) oacc[kh][db] = Mfma<T>::run(vf1[db], pf1, oacc[kh][db]);
    };

    for (int i = 0; i < n_tiles; ++i) {
        const int stage = i % NSTG;
        unsigned char* ks = smem + stage * STAGE_BYTES;
        unsigned char* vs = ks + K_BYTES;
        // tile i has landed (tile i + 1 stays in flight) ...
        if (i + 1 < n_tiles) wait_vm<PIECES>();
        else wait_vm<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wg_barrier();                   // ... for every wave, and every wave is done reading tile i - 1: its stage takes tile i + 2
        if (i + 2 < n_tiles) issue_tile(i + 2, (i + 2) % NSTG);
        const int k0 = i * KT;
        if (k0 + KT > S_tot) {          // work-group uniform, the chunk's last tile only
            zero_stale_vt<D>(vs, S_tot - k0, tid, NTHR);      // the V^T columns of keys >= P + T hold whatever the cache held
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            wg_barrier();
        }
        int kb = kb_lane + stage * STAGE_BYTES, vb = vb_lane + stage * STAGE_BYTES;
        asm volatile("" : "+v"(kb), "+v"(vb));
        // wave uniform: sub-tiles above this wave's diagonal are skipped, sub-tiles wholly below it take the unmasked path
        if (2 * i < w_subs) compute(kb, vb, k0, std::integral_constant<int, 0>{}, 2 * i >= w_full);
        if (2 * i + 1 < w_subs) compute(kb, vb, k0, std::integral_constant<int, 1>{}, 2 * i + 1 >= w_full);
    }

    // ---- normalise, transpose through LDS (32 rows per wave, wave-private), store whole rows
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    wg_barrier();                       // the ring is no longer read: reuse it
    if (!wave_live) return;
    constexpr int RS = 2 * D + 16;      // staging row stride (bytes), 16-B aligned
    static_assert((size_t)ROWS * RS <= (size_t)NSTG * STAGE_BYTES, "staging rows fit in the ring");
    unsigned char* stg = smem + (size_t)wave * 32 * RS;
    // merge of the two key halves, with attn_fwd_kernel's ownership convention: there the wave of half 0 finishes the lower d-blocks
    // (own = half 0) and the wave of half 1 the upper ones (own = half 1)
    const PairMerge pm = pair_merge(m_run[0], l_run[0], m_run[1], l_run[1]);
    auto merged = [&](int db, int e) {
        return db < DBLK / 2 ? merged_elem(oacc[0][db][e], pm.s0, oacc[1][db][e], pm.s1) : merged_elem(oacc[1][db][e], pm.s1, oacc[0][db][e], pm.s0);
    };
#pragma unroll
    for (int db = 0; db < DBLK; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            u32x2 w;
            w[0] = pack2<T>(merged(db, 4 * g4 + 0), merged(db, 4 * g4 + 1));
            w[1] = pack2<T>(merged(db, 4 * g4 + 2), merged(db, 4 * g4 + 3));
            *reinterpret_cast<u32x2*>(stg + ql * RS + (db * 32 + 8 * g4 + 4 * hi) * 2) = w;
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // LDS operations of one wave complete in order: no barrier for a wave-private region
    constexpr int CPR = 2 * D / 16;     // 16-B chunks per output row
    const int n_store = min(32, n_rows - w0) * CPR;
    for (int idx = lane; idx < n_store; idx += 64) {
        const int row = idx / CPR, c = idx % CPR;
        const int r2 = w0 + row, hg2 = r2 / Tn, t2 = r2 - hg2 * Tn;
        const u32x4 v = *reinterpret_cast<const u32x4*>(stg + row * RS + c * 16);
        *reinterpret_cast<u32x4*>(a.out + (size_t)t2 * a.out_row_stride + (size_t)(kvh * n_rep + hg2) * D + c * 8) = v;
    }
}

template <typename T, int D>
static int launch(const lade_attn_args* a, hipStream_t st) {
    PrefillK k;
    k.q = (const uint16_t*)a->q; k.k = (const uint16_t*)a->k_cache; k.vt = (const uint16_t*)a->vt_cache; k.out = (uint16_t*)a->out;
    k.q_row_stride = a->q_row_stride; k.out_row_stride = a->out_row_stride;
    k.H = a->H; k.Hkv = a->Hkv; k.S_max = a->S_max; k.n_rep = a->H / a->Hkv; k.T = a->mask.T; k.P = a->mask.P;
    k.n_rb = (int)(((int64_t)k.n_rep * k.T + ROWS - 1) / ROWS);
    k.scale_log2 = a->scale * 1.4426950408889634f;
    const size_t lds = (size_t)NSTG * KT * D * 2 * 2;
    static bool attr_set = false;          // > 64 KiB of dynamic LDS needs the opt-in once per kernel
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)attn_prefill_kernel<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((attn_prefill_kernel<T, D>), dim3((unsigned)(k.n_rb * a->Hkv)), dim3(NTHR), lds, st, k);
    return check_launch("lade_attn_prefill");
}

}  // namespace pf
}  // namespace lade

using namespace lade;

extern "C" int lade_attn_prefill(const lade_attn_args* a, void* stream) {
    LADE_REQUIRE(a != nullptr, LADE_E_ARG, "lade_attn_prefill: null args");
    LADE_REQUIRE(a->q && a->k_cache && a->vt_cache && a->out, LADE_E_ARG, "lade_attn_prefill: null tensor pointer");
    LADE_REQUIRE(a->dtype == LADE_BF16 || a->dtype == LADE_F16, LADE_E_ARG, "lade_attn_prefill: dtype=%d (bf16 and f16 only; fp32 chunks run on lade_attn_fwd)", a->dtype);
    LADE_REQUIRE(a->d == 128 || a->d == 64, LADE_E_ARG, "lade_attn_prefill: head_dim %d (64 and 128)", a->d);
    LADE_REQUIRE(a->mask.is_prefill == 1, LADE_E_ARG, "lade_attn_prefill: is_prefill=%d (plain causal chunks only; lookahead steps run on lade_attn_fwd)", a->mask.is_prefill);
    LADE_REQUIRE(a->dyn_P == nullptr, LADE_E_ARG, "lade_attn_prefill: dyn_P is not supported (the block lengths are decided on the host)");
    LADE_REQUIRE(a->H > 0 && a->Hkv > 0 && a->H % a->Hkv == 0, LADE_E_ARG, "lade_attn_prefill: H=%d Hkv=%d", a->H, a->Hkv);
    LADE_REQUIRE(a->mask.T > 0 && a->mask.P >= 0, LADE_E_ARG, "lade_attn_prefill: T=%d P=%d", a->mask.T, a->mask.P);
    LADE_REQUIRE(a->S_max % 64 == 0 && a->S_max <= (1 << 22) && (int64_t)a->mask.P + a->mask.T <= a->S_max, LADE_E_ARG,
                 "lade_attn_prefill: S_max=%d must be a multiple of 64, at most 2^22 and >= P+T=%lld", a->S_max, (long long)a->mask.P + a->mask.T);
    LADE_REQUIRE((int64_t)(a->H / a->Hkv) * a->mask.T < (1ll << 30), LADE_E_LIMIT, "lade_attn_prefill: %d x %d rows per KV head", a->H / a->Hkv, a->mask.T);
    LADE_REQUIRE(a->q_row_stride % 8 == 0 && a->out_row_stride % 8 == 0 && ((uintptr_t)a->q & 15) == 0 && ((uintptr_t)a->out & 15) == 0, LADE_E_ARG,
                 "lade_attn_prefill: q / out rows must keep 16-B alignment");
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == LADE_BF16) return a->d == 128 ? pf::launch<BF16, 128>(a, st) : pf::launch<BF16, 64>(a, st);
    return a->d == 128 ? pf::launch<F16, 128>(a, st) : pf::launch<F16, 64>(a, st);
}
