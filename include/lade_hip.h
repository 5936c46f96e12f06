/*
 * lade_hip.h -- C ABI of liblade_hip.so, the MI355X (gfx950) native hot path of lookahead decoding.
 *
 * Boundary contract:
 *   - plain C: pointers + sizes, no torch / C++ types.  Device pointers are raw HBM addresses
 *     (tensor.data_ptr()), `stream` is a hipStream_t passed as void* (torch's current stream).
 *   - the caller owns every buffer; the library allocates nothing persistent.
 *   - every entry point returns 0 on success or a negative LADE_E_* code and never throws;
 *     arguments are validated on the host before any launch; lade_last_error_string() gives the
 *     text of the last failure on the calling thread.  Asynchronous kernel faults surface at the
 *     caller's next synchronisation, as with any HIP launch.
 *   - all entry points are stateless and re-entrant; ordering is only through `stream`.
 *     Everything is hipGraph-capturable (no allocation / sync inside).
 *
 * What each entry point replaces in the reference (paths relative to the reference repo):
 *   lade_attn_fwd            flash_attn_lade.flash_attn_func(q,k,v,...,lookahead=[7 ints])
 *                            lade/models/modeling_llama.py:705-713 (flash) and the eager op
 *                            :520-541 + the dense mask of :115-207 (evaluated in-kernel here)
 *   lade_attn_combine        (second pass of the split-KV attention; no reference counterpart)
 *   lade_attn_prefill        eager attention under the causal prefill mask (modeling_llama.py:124-130, :520-541), chunks > 256 rows
 *   lade_rope_kv_append      apply_rotary_pos_emb + torch.cat KV append
 *                            lade/models/modeling_llama.py:321-346, :510-516
 *   lade_kv_commit           lade/decoding.py:1154-1163 (greedy) / :582-590 (sample)
 *   lade_kv_pack_bshd        (adapter only) K / V as `flash_attn_func` receives them -> this library's cache layout
 *   lade_build_inputs        lade/models/modeling_llama.py:1463-1511 (ids / position_ids assembly)
 *   lade_argmax_rows / lade_argmax_pairs   torch.argmax(outputs.*_logits, dim=-1)  lade/decoding.py:1021,1041,1052,1072,1102
 *                            (pairs: on what the lm_head GEMM's argmax epilogue leaves instead of the logits)
 *   lade_verify_greedy       lade/decoding.py:1071-1084
 *   lade_pool_insert_window  update_token_map             lade/decoding.py:37-63
 *   lade_pool_insert_ngrams  fill_pool_with_prompt / append_new_generated_pool  lade/decoding.py:80-127
 *   lade_pool_lookup         lade/decoding.py:948-954
 *   lade_window_fill_first / lade_window_fill / lade_window_roll   lade/decoding.py:1038-1066, :1119-1124
 *   lade_greedy_post_step    the fused single-rank tail of one steady step: verify + pool insert +
 *                            roll + next lookup + control update   lade/decoding.py:1071-1130,1165
 *   lade_lp_unique_id / lade_lp_comm_create / lade_lp_allgather / lade_lp_comm_count / lade_lp_comm_destroy   RCCL communicator + the step's one
 *                            collective   lade/utils.py:28-33, lade/decoding.py:1024,1057,1090,1096,1106
 *   lade_lp_pack / lade_lp_reduce_apply   the per-step lookahead-parallel exchange record
 *                            lade/decoding.py:1023-1024, 1088-1107 (four pickled object collectives
 *                            -> one fixed int32 all-gather issued by the host through RCCL)
 *   lade_softmax_rows / lade_softmax_gather   probabilities of the sampling verify: one full row (the distribution a token is
 *                            finally drawn from) / the per-candidate draft probabilities of the acceptance loop, gathered on
 *                            the device without materialising guess_probs   lade/decoding.py:484-540
 *   lade_warp_rows           temperature / top-k / top-p warpers in one launch   lade/decoding.py:375-377, :443, :488
 *   lade_warp_rows_ex        the same launch followed by HF's min-p, typical, epsilon and eta warpers (transformers
 *                            generation/logits_process.py; the reference refuses every warper beyond the three, lade/decoding.py:375-377)
 *   lade_rmsnorm / lade_embed_rmsnorm / lade_add_rmsnorm / lade_silu_mul / lade_gather_rows   LlamaRMSNorm (+ residual add), SwiGLU,
 *                            embedding / logits-row gather around the GEMMs
 *                            lade/models/modeling_llama.py:222-227, :360-380, :1164 ("next" row)
 *   lade_gemm_skinny / lade_gemm_skinny_kt / lade_gemm_qkv_rope / lade_qkv_pair_row / lade_weight_to_ktile / lade_weight_from_ktile / lade_splitk_reduce   the nn.Linear projections of the step at M = T <= 128 rows
 *                            lade/models/modeling_llama.py:360-380 (MLP), :492-494, :558 (q/k/v/o)
 *                            lade_rope_kv_append, lade_add_rmsnorm and lade_silu_mul also take that GEMM's fp32 split-K partials as
 *                            their input (the reduction is fused into the consumer); lade_rope_kv_append carries the qkv epilogue of
 *                            Qwen2 (q / k / v bias) and Qwen3 (per-head RMSNorm of q and k before RoPE) - the reference adapts Llama only
 *   lade_gen_ctl_init / lade_gen_ctl_update / lade_gen_argmax / lade_gen_rows   HF's repetition penalty and min-length processors on the
 *                            step's rows; lade_gen_constraints_init adds HF's bad_words_ids / suppress_tokens / begin_suppress_tokens /
 *                            sequence_bias processors to them (the reference refuses every logits processor, lade/decoding.py:968); lade_greedy_post_step takes a set of EOS ids (the reference refuses them, lade/decoding.py:968)
 *   lade_emit_init / lade_emit_rows   the `scores` / `logits` tuples of generate(return_dict_in_generate=True): the reference refuses them
 *                            (lade/decoding.py:967 greedy, the matching assertion at the head of jacobi_sample_multilevel's loop for sampling)
 *   lade_time_attn / lade_time_attn_rot   hipEvent timing helpers for bench.py (no reference counterpart)
 */
#ifndef LADE_HIP_H
#define LADE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LADE_ABI_VERSION 5      /* 2: lade_attn_args grew (wg_rows, fused RoPE), lade_gemm_skinny* take `ring`, lade_greedy_post_step takes record_host;
                                 * 3: + lade_gemm_ra_kt, lade_build_flags; + lade_gen_ctl_init, lade_gen_ctl_update, lade_gen_argmax,
                                 *    lade_gen_rows, lade_greedy_post_step_ex (nothing that existed changed);
                                 * 4: the measured-and-dropped kernels are gone: lade_attn_args ends at wg_rows (n_parts, qkv_parts, part_stride, positions,
                                 *    cos_tab, sin_tab, max_pos, sync_flags removed), lade_gemm_ra_kt and lade_build_flags removed; nothing else changed
                                 *    (+ lade_emit_init, lade_emit_rows);
                                 * 5: one entry point per kernel family, the source and the optional stages chosen by nullable arguments: lade_rope_kv_append
                                 *    (was + _ex, _parts, _parts_ex), lade_greedy_post_step (takes the EOS set; _ex removed), lade_add_rmsnorm (was + _parts,
                                 *    _rows), lade_silu_mul (was + _parts);
                                 *    + lade_gemm_qkv_rope, lade_qkv_pair_row, lade_qkv_rope_args (additions only: no argument list that existed changed, so the
                                 *    number stays - a library without them fails to load by the missing symbol) */

/* error codes */
#define LADE_OK 0
#define LADE_E_ARG (-1)     /* invalid argument (null pointer, unsupported size ...) */
#define LADE_E_DTYPE (-2)   /* unsupported dtype / head_dim for this kernel */
#define LADE_E_LAUNCH (-3)  /* hipLaunch failed (text in lade_last_error_string) */
#define LADE_E_LIMIT (-4)   /* a compiled-in limit exceeded (LADE_MAX_*) */

/* element types of floating-point tensors */
#define LADE_BF16 0
#define LADE_F16 1
#define LADE_F32 2

/* compiled-in limits of the integer kernels */
#define LADE_MAX_LEVEL 16        /* N  (n-gram size) */
#define LADE_MAX_WINDOW 128      /* W + N - 3 */
#define LADE_MAX_GUESS_SET 64    /* G  (candidates per key; one wave lane per slot) */
#define LADE_REC_WORDS (8 + LADE_MAX_LEVEL)      /* int32 words of a step's record */
/* Seal of a step record (its last word), so that a host polling a pinned copy can tell a complete record of step `step_no` from a stale
 * or half-landed one: a multiplicative hash of the step number xor-folded with the other words, each times an odd constant (the
 * definition is seal_words() in csrc/common.hpp, shared by the kernel and this host entry point).  rec: LADE_REC_WORDS words in HOST memory. */
uint32_t lade_record_seal(const uint32_t* rec, uint32_t step_no);

/* ---- control block ------------------------------------------------------------------
 * One int32 array in HBM carries the dynamic state of a sequence between kernels, so a steady
 * step needs no host round trip except reading the small `record` it leaves behind.
 * Layout (indices into int32_t ctl[LADE_CTL_WORDS]): */
#define LADE_CTL_P 0            /* committed KV rows (= past_key_values_length of the coming step) */
#define LADE_CTL_LST_TOKEN 1    /* lst_token: last accepted token = the next input token */
#define LADE_CTL_LST_POS 2      /* position id of that token (= attention_mask length - 1) */
#define LADE_CTL_N_INPUT 3      /* true input tokens fed at the head of the step (1 + guess_skip_dist) */
#define LADE_CTL_G 4            /* candidates to verify in the coming step (0..G) */
#define LADE_CTL_FILL_LEVEL 5   /* fill_level */
#define LADE_CTL_MAX_HIT 6      /* results of the last step */
#define LADE_CTL_MAX_HIT_IDX 7
#define LADE_CTL_N_ACCEPT 8     /* max_hit + 1 */
#define LADE_CTL_STEP 9         /* steps executed */
#define LADE_CTL_KV_SRC 10      /* kv_commit: first source row (step_len - lguess + idx*gs) */
#define LADE_CTL_KV_DST 11      /* kv_commit: first destination row (kvcache_len) */
#define LADE_CTL_KV_CNT 12      /* kv_commit: rows to copy (max_hit, 0 under lookahead parallelism) */
#define LADE_CTL_FIRST_GUESS 13
#define LADE_CTL_HITS 16        /* hits[0..gs) */
#define LADE_CTL_WLEN 32        /* lengths of window levels 0..N-2 */
#define LADE_CTL_WORDS 64

/* ---- attention ----------------------------------------------------------------------- */

/* The lookahead mask in closed form (reference: j_make_causal_mask_multilevel,
 * lade/models/modeling_llama.py:115-207; its flash counterpart gets the same information as
 * lookahead=[window, level, n_guess, kv_cache, fill_offset, guess_offset, 0], :1184-1187).
 * Token order of the T new rows: [n_input inputs | L0 | L1 .. | g*gs candidate tokens] (layout 0, the eager
 * path's order), or with levels >= 1 interleaved column-major [.. | L0 | L1[0] L2[0] .. | L1[1] L2[1] .. | ..]
 * (layout 1: the order the reference feeds its flash kernel, modeling_llama.py:1471-1485); q rows, the new
 * K/V rows and the output rows all follow the chosen order. */
typedef struct lade_mask_params {
    int32_t T;            /* new tokens this step (query rows; keys P..P+T) */
    int32_t P;            /* cached keys, visible to every row */
    int32_t is_prefill;   /* 1: plain causal over the T new tokens (:124-130) */
    int32_t s;            /* level_sizes[-1]                       ("window") */
    int32_t lguess;       /* g*gs candidate rows at the tail */
    int32_t gs;           /* tokens per candidate = N-1 */
    int32_t level_offset; /* n_input-1 = guess_offset */
    int32_t dist_offset;  /* 1 + level_sizes[0] - level_sizes[-1]  (fill_offset = level_offset+dist_offset) */
    int32_t layout;       /* 0 = level-major rows (eager order), 1 = levels >= 1 column-major (flash order) */
} lade_mask_params;

typedef struct lade_attn_args {
    const void* q;          /* [T][H][d] rows, element stride q_row_stride between tokens */
    const void* k_cache;    /* [Hkv][S_max][d]   keys, row-major            */
    const void* vt_cache;   /* [Hkv][d][S_max]   values, TRANSPOSED (key index fastest) */
    void* out;              /* [T][H][d], token stride out_row_stride */
    void* part_o;           /* split-KV partial outputs [n_splits][T][H][d], model dtype (n_splits>1) */
    float* part_ml;         /* [n_splits][H][T][2]  (running max in log2 units, running sum) */
    const int32_t* dyn_P;   /* optional device int32: overrides mask.P at run time (graph replay) */
    int64_t q_row_stride, out_row_stride; /* in elements */
    int32_t H, Hkv, d, S_max;
    int32_t dtype;          /* LADE_BF16 / LADE_F16 (MFMA kernel, d = 64 or 128), LADE_F32 (VALU kernel, d <= 256) */
    int32_t n_splits;       /* >= 1 ; work-groups = ceil(n_rep*T/128) x H/n_rep x n_splits (1-D grid, XCD-aware order) */
    float scale;            /* softmax scale, 1/sqrt(d) */
    lade_mask_params mask;
    /* ---- since LADE_ABI_VERSION 2 ---- */
    int32_t wg_rows;        /* work-group shape: query rows of the (head-in-group, token) row space per work-group - 128 (4 x 2 waves, one 64-key
                             * tile per stage), 64 or 32 (two tiles per stage, every wave computes); 0 = 128.  A launch parameter like the GEMM's
                             * tile shape: the caller's in-step autotune picks it per launch shape together with n_splits */
} lade_attn_args;

int lade_attn_fwd(const lade_attn_args* a, void* stream);
/* merges the n_splits partials of lade_attn_fwd into `out` (call only when n_splits > 1) */
int lade_attn_combine(const lade_attn_args* a, void* stream);
/* One-pass causal attention for a prefill chunk (replaces the reference's eager attention under the plain causal mask of a prompt:
 * lade/models/modeling_llama.py:124-130 build the mask, :520-541 apply it).  lade_attn_fwd is built for the decode step (few rows, long
 * cache, HBM bound: KV splits + lade_attn_combine); this entry point is the compute-bound form for chunks of hundreds to thousands of rows:
 * work-groups of 8 waves x 32 query rows, every K / V^T tile staged once per 256 rows, tiles above a block's diagonal never requested,
 * longest blocks first, ONE launch and no partial buffers.
 * The engine launches it only under LADE_DEBUG=prefill_attn=1.
 * Takes lade_attn_args as it is and requires: mask.is_prefill == 1 (row t of the chunk sees keys 0 .. P + t),
 * dyn_P == NULL, dtype LADE_BF16 or LADE_F16, d = 64 or 128, S_max a multiple of 64 (at most 2^22) and >= P + T, q / out 16-byte aligned with
 * row strides that are multiples of 8 elements (q may be a view into the qkv buffer).  Anything else returns LADE_E_ARG with a message.
 * Reads k_cache [Hkv][S_max][d] and vt_cache [Hkv][d][S_max] (rows P .. P+T already appended), writes out [T][H][d].  n_splits, wg_rows,
 * part_o and part_ml are ignored.  Scores stay fp32, the softmax is online in the log2 domain, P is rounded to the model dtype before PV
 *  - the arithmetic of lade_attn_fwd's 128-row shape, operation for operation: the output equals lade_attn_fwd's with
 * n_splits = 1 bit for bit.  Cache rows at and beyond P + T may hold anything (NaN included): they never reach the output. */
int lade_attn_prefill(const lade_attn_args* a, void* stream);
/* dense 0/1 rendering of the mask predicate, [T][P+T] bytes on the device (test / debug aid) */
int lade_mask_render(const lade_mask_params* m, uint8_t* out, void* stream);

/* ---- RoPE + KV append, KV commit ----------------------------------------------------- */

/* rope_scaling "dynamic" (LlamaDynamicNTKScalingRotaryEmbedding, lade/models/modeling_llama.py:292-318): the cos / sin rows of ONE step.
 * The reference rebuilds its tables with a sequence-dependent base whenever kv_seq_len = P + T (:502-510) exceeds the longest length seen;
 * here state[0] (device int32, initialised to max_position_embeddings, reset with the sequence) carries that length, inv_tab
 * [n_len][d/2] (fp32, host-built like the reference builds inv_freq) holds the inverse frequencies of a rebuild at length
 * max_position_embeddings + i, and the kernel writes cos_rows / sin_rows [T][d] (model dtype) for the step's T positions - the rope
 * entry points below are then called with positions = 0..T-1 and these rows as their tables.  len_hint: a longer length the step
 * belongs to (chunked prefill: the reference sees the whole prompt at once), 0 otherwise.  P from dyn_P when non-null.  g_dev (nullable):
 * the step is a hipGraph step padded to gcap candidates of gs rows of which only *g_dev exist - the length counts the real rows. */
int lade_rope_rows_dynamic(const int32_t* positions, int32_t T, int32_t P, const int32_t* dyn_P, int32_t len_hint, int32_t* state,
                           int32_t max_position_embeddings, const float* inv_tab, int32_t n_len, int32_t d, void* cos_rows, void* sin_rows,
                           int32_t dtype, const int32_t* g_dev, int32_t gcap, int32_t gs, void* stream);

/* RoPE of q and k fused with the KV append: the rotated k and the v of token t go to cache row P+t.  cos/sin: [max_pos][d] tables in the
 * model dtype, built as the reference builds them (fp32 math, then cast; modeling_llama.py:248-256); the rotation reproduces the
 * reference's per-op rounding: round(q*cos) + round(rotate_half(q)*sin), rounded.  positions: device int32[T] (explicit, non-monotone
 * position ids).  P from `dyn_P` if non-null.
 * The source of q / k / v - exactly one of the two, both or neither is LADE_E_ARG:
 *   qkv     [T][(H+2*Hkv)*d], the materialised fused projection; q is rotated in place (n_parts, part_stride, q_out are ignored).  d even;
 *           all three dtypes.
 *   parts   the same projection as n_parts >= 1 fp32 split-K partials [n_parts][T][(H+2*Hkv)*d], part_stride elements apart, summed in
 *           split order and rounded once to the model dtype; the rotated q goes to q_out [T][H*d] (required).  (d/2) % 8 == 0; bf16 / f16
 *           only (LADE_E_DTYPE otherwise).
 * epi (nullable; one whose three pointers are null counts as null: exactly the plain kernel) - the qkv epilogue of Qwen2 / Qwen3, applied
 * per token and head between the projection and RoPE; a null field skips its step:
 *   bias    [(H + 2*Hkv)*d] model dtype, added to q, k and v: to the fp32 sum of the partials before its single rounding (F.linear with a
 *           bias), or to the already rounded qkv with one more rounding;
 *   q_norm, k_norm   [d] model dtype: Qwen3RMSNorm over each q / k head, x -> round(w * round(x * rsqrt(mean(x^2) + eps))), the mean in
 *           fp32, 0 <= eps < 1; RoPE runs on the result.  V gets the bias only.
 * The three pointers 16-byte aligned.  The head norm on `parts` needs d / 16 to be a power of two. */
typedef struct lade_qkv_epilogue {
    const void* bias;
    const void* q_norm;
    const void* k_norm;
    float eps;
} lade_qkv_epilogue;
int lade_rope_kv_append(void* qkv, const float* parts, int32_t n_parts, int64_t part_stride, void* q_out, const int32_t* positions,
                        const void* cos_tab, const void* sin_tab, void* k_cache, void* vt_cache, int32_t T, int32_t P,
                        const int32_t* dyn_P, int32_t H, int32_t Hkv, int32_t d, int32_t S_max, int32_t max_pos, int32_t dtype,
                        const lade_qkv_epilogue* epi, void* stream);

/* Copies `cnt` K/V rows src..src+cnt -> dst..dst+cnt in every layer of a [L][2] cache whose
 * K part is [Hkv][S_max][d] and V part [Hkv][d][S_max]; layer_stride / v_offset in elements.
 * If `ctl` is non-null, (src,dst,cnt) are read from ctl[LADE_CTL_KV_SRC..KV_CNT] on the device.  max_cnt is reserved
 * (pass 0). */
int lade_kv_commit(void* cache, int64_t layer_stride, int64_t v_offset, int32_t L, int32_t Hkv, int32_t d,
                   int32_t S_max, int32_t src, int32_t dst, int32_t cnt, const int32_t* ctl, int32_t max_cnt,
                   int32_t elem_bytes, void* stream);

/* K / V in the layout the reference hands its flash kernel - [S][Hkv][d], token-major: `flash_attn_func(q, k, v, ...)` at
 * lade/models/modeling_llama.py:705-713 after the transposes of :636-638 - re-laid into this library's cache layout: k_cache
 * [Hkv][S_max][d], vt_cache [Hkv][d][S_max] (rows >= S untouched).  k and v share their strides (elements): tok_stride between tokens,
 * head_stride between heads - Hkv*d and d for a contiguous [S][Hkv][d] tensor, d and S*d for the transposed VIEW of [Hkv][S][d] the
 * reference really passes (:636-638 transpose without a copy).  One launch, every byte read and written once: the adapter
 * `lookaheaddecoding_amd/flash_attn_lade.py:flash_attn_func` calls it per attention call, which costs about what the reference's own
 * per-layer torch.cat of the whole cache costs (:626-629); the step engine never does - its cache is resident in this layout. */
int lade_kv_pack_bshd(const void* k, const void* v, int64_t tok_stride, int64_t head_stride, void* k_cache, void* vt_cache, int32_t S,
                      int32_t Hkv, int32_t d, int32_t S_max, int32_t elem_bytes, void* stream);

/* ---- integer path (all bit-exact against the reference's python logic) ---------------- */

/* window: int32 [N-1][wcap] (wcap >= W+N-3), level lengths in ctl[LADE_CTL_WLEN+l].
 * pool_tok: int32 [V][G][gs], pool_cnt: int32 [V]. */

/* ids/pos <- [n_input inputs | L0[0:c1-1] | L1[c0:c1] .. L_fill[c0:c1] | candidates].  The input tokens
 * and their positions are read from in_ids/in_pos (device); when null they come from the control block:
 * ids = lst_token (n_input = 1) or hits[0..n_input) (re-fed accepted tokens under lookahead parallelism),
 * positions = the n_input positions ending at ctl[LADE_CTL_LST_POS].  (c0,c1) = this rank's window columns under lookahead
 * parallelism (lade/decoding.py:973-984), c1 < 0 = all columns.  g < 0 reads ctl[LADE_CTL_G].
 * cand_rows >= 0 emits exactly that many candidate rows (zero tokens beyond g*gs: fixed-shape graph
 * replay), cand_rows < 0 emits g*gs.  out_T[0] = total tokens written (may be null).  lp_world > 1 with g < 0: the candidates
 * emitted are rank lp_rank's share of ctl[LADE_CTL_G] (lade/decoding.py:956-963), decided on the device; otherwise pass 0, 1. */
int lade_build_inputs(const int32_t* in_ids, const int32_t* in_pos, int32_t n_input, const int32_t* window,
                      int32_t wcap, const int32_t* ctl, int32_t fill_level, int32_t c0, int32_t c1,
                      const int32_t* guess, int32_t g, int32_t gs, int32_t cand_rows, int32_t* ids, int32_t* pos,
                      int32_t* out_T, int32_t lp_rank, int32_t lp_world,
                      void* stream);

/* one argmax per row, first index wins ties (torch.argmax semantics); logits [rows][V] with row
 * stride `ld` elements. */
int lade_argmax_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, int32_t* out,
                     void* stream);

/* out[r] = column of the best of row r's n_blocks {value, column} pairs (lade_gemm_skinny, epilogue 2): the same ids lade_argmax_rows
 * returns on the materialised logits (first index wins ties). */
int lade_argmax_pairs(const float* pairs, int32_t rows, int32_t n_blocks, int32_t* out, void* stream);

/* out3 = {max_hit, max_hit_idx}, hits[gs]; g may also come from ctl[LADE_CTL_G] when dyn != 0 */
int lade_verify_greedy(const int32_t* first_guess, const int32_t* guess, const int32_t* guess_argmax, int32_t g,
                       int32_t gs, int32_t* out2, int32_t* hits, void* stream);

int lade_pool_insert_window(int32_t* pool_tok, int32_t* pool_cnt, int32_t V, int32_t G, int32_t gs,
                            const int32_t* lst_token, const int32_t* window, int32_t wcap, const int32_t* new_results,
                            int32_t W, int32_t N, void* stream);
/* n sequential inserts; ngrams [n][N]: key then gs tokens */
int lade_pool_insert_ngrams(int32_t* pool_tok, int32_t* pool_cnt, int32_t V, int32_t G, int32_t gs,
                            const int32_t* ngrams, int32_t n, void* stream);
/* sliding N-grams over tokens[0..len) == fill_pool_with_prompt */
int lade_pool_fill_prompt(int32_t* pool_tok, int32_t* pool_cnt, int32_t V, int32_t G, int32_t gs,
                          const int32_t* tokens, int32_t len, void* stream);
/* guess_out [G*gs], g_out[0] = number of tuples stored under *key (0 if none) */
int lade_pool_lookup(const int32_t* pool_tok, const int32_t* pool_cnt, int32_t V, int32_t G, int32_t gs,
                     const int32_t* key, int32_t* guess_out, int32_t* g_out, void* stream);

int lade_window_fill_first(int32_t* window, int32_t wcap, int32_t* ctl, const int32_t* inp_argmax, int32_t n,
                           void* stream);
int lade_window_fill(int32_t* window, int32_t wcap, int32_t* ctl, int32_t fill_level, const int32_t* inp_argmax,
                     int32_t n, void* stream);
int lade_window_roll(int32_t* window, int32_t wcap, int32_t* ctl, const int32_t* new_results, int32_t W, int32_t N,
                     void* stream);

/* Fused tail of one single-rank greedy step.  am = argmax rows in the order
 * [out row | n_inp inp rows | cand_rows guess rows].  phase 0 = prefill step (L1 <- inp rows),
 * 1 = window-fill step, 2 = steady step.  Does: verify (g = ctl[G], phase 2) -> pool insert (W n-grams)
 * -> window fill / roll -> EOS scan + POOL_FROM_PROMPT appends (`tail` = [len, last <=N tokens of the
 * reference's all_old_tokens]) -> lookup of the next step's candidates into `guess` / ctl[G] -> ctl update
 * (P, lst_token, lst_pos, kv-commit triple, hits, step).
 * record = {max_hit, n_accept, finished_by_eos, g_next, P_next, max_hit_idx, first_guess, step number (ctl[STEP] after this step),
 * hits[gs], 0 ..., seal} - LADE_REC_WORDS words, the last one lade_record_seal() of the others.  record_host (nullable): the same
 * words are ALSO stored to this address - pinned host memory mapped into the device - so that the host can poll for the step's record
 * instead of synchronising the stream (no copy node, no blocking wait in a steady step).  NO fence follows those stores (fine-grained host
 * memory takes them as they are issued, in any order): the seal, computed over all the other words, is the only ordering guarantee - a
 * reader accepts a record only when the step number AND the seal match what it read, and must bound its wait (memory the device's stores do
 * not reach coherently never shows the record).
 * eos_set: HOST array of n_eos end-of-sequence ids (0..LADE_GEN_MAX_EOS, each >= 0; null allowed when n_eos == 0), copied into the
 * launch.  The EOS scan (lade/decoding.py:1167-1177) stops at the first accepted token that is in the set; the tokens accepted after it in
 * the same step are dropped.  n_eos == 0 disables the scan.
 * Sampling (lade/decoding.py:137-692): the rejection-sampling verify runs on the host (it consumes the python
 * and torch RNG streams in the reference's order); its result is passed as forced = {max_hit, max_hit_idx,
 * hits[gs]} (device) and replaces the greedy verify; level_override[W] (device, -1 = keep) carries the
 * filter_window() replacements of EOS tokens in the newest window level.  Both are null for greedy. */
int lade_greedy_post_step(int32_t* ctl, int32_t* window, int32_t wcap, int32_t* pool_tok, int32_t* pool_cnt,
                          int32_t V, int32_t W, int32_t N, int32_t G, const int32_t* am, int32_t n_inp,
                          int32_t* guess, int32_t T_step, int32_t cand_rows, int32_t phase, int32_t pool_from_prompt,
                          int32_t* tail, const int32_t* eos_set, int32_t n_eos, const int32_t* forced,
                          const int32_t* level_override, int32_t* record, int32_t* record_host, void* stream);

/* ---- generation controls (HF's RepetitionPenaltyLogitsProcessor, MinLengthLogitsProcessor / MinNewTokensLengthLogitsProcessor) ----
 * The controls of one sequence live in a device block of int32 words `gen` (LADE_GEN_WORDS(V)), never in kernel arguments: a captured
 * step reads them at replay, so a new prompt (new seen set, new min_len) needs no re-capture.
 *   gen[LADE_GEN_PENALTY]      penalty p as fp32 bits (1.0 = off)
 *   gen[LADE_GEN_INV_PENALTY]  fp32 bits of (float)(1.0 / p), the reciprocal taken in double: torch's device kernel divides by a
 *                              scalar as a multiplication by that reciprocal, so HF's s / p is s * inv here (bit-exact against torch)
 *   gen[LADE_GEN_MIN_LEN]      absolute minimum length (min_length, or prompt length + min_new_tokens; 0 = off)
 *   gen[LADE_GEN_N_EOS], gen[LADE_GEN_EOS + e]   the ids masked to -inf while a row's sequence length L < min_len
 *   gen[LADE_GEN_VOCAB]        V
 *   gen[LADE_GEN_CONS], gen[LADE_GEN_CONS + 1]   address of the token-constraint block (below), low / high 32 bits; 0 = no constraints
 *   gen[LADE_GEN_SEEN ..]      seen-set bitmap, ceil(V/32) words: bit t = token t occurs in prompt + accepted tokens */
#define LADE_GEN_MAX_EOS 8
#define LADE_GEN_PENALTY 0
#define LADE_GEN_INV_PENALTY 1
#define LADE_GEN_MIN_LEN 2
#define LADE_GEN_N_EOS 3
#define LADE_GEN_VOCAB 4
#define LADE_GEN_EOS 8
#define LADE_GEN_SEEN 16
#define LADE_GEN_WORDS(V) (LADE_GEN_SEEN + ((V) + 31) / 32)
#define LADE_GEN_MAX_VOCAB (1 << 18)    /* a row's penalised set is staged in LDS: <= 32 KiB */
#define LADE_GEN_CONS 5                 /* gen[5..6]: device address of the token-constraint block, low / high word (0 = none) */

/* ---- token constraints (HF's SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor, SequenceBiasLogitsProcessor,
 * NoBadWordsLogitsProcessor) ----
 * A second device block of int32 words `cons` (LADE_GEN_CONS_WORDS(V)), attached to `gen` by its address in gen[LADE_GEN_CONS ..+1]:
 * the row kernels read that address at replay, so attaching, detaching or rewriting the block needs no re-capture.  Address 0: the row
 * kernels compute exactly what they compute without this section.
 *   cons[LADE_CONS_N_SEQ]       sequence entries in the table (<= LADE_GEN_MAX_SEQ)
 *   cons[LADE_CONS_N_ONE]       how many of them, at the head of the table, have length 1 (they fire on every row, window rows included)
 *   cons[LADE_CONS_BEGIN_INDEX] the input length at which the begin bans apply (-1 = no begin bans)
 *   cons[LADE_CONS_FLAGS]       LADE_CONS_F_ADD: a sequence-bias class is present, so every score takes HF's `scores + bias` (bias +0.0
 *                               where nothing fires: a -0.0 score becomes +0.0, as in HF)
 *   cons[LADE_CONS_TAIL_N], cons[LADE_CONS_TAIL ..]   the last min(len, LADE_GEN_MAX_SEQ_LEN - 1) tokens of prompt + accepted tokens,
 *                               right-aligned in LADE_GEN_MAX_SEQ_LEN - 1 slots
 *   cons[LADE_CONS_OFF ..]      n_seq + 1 offsets into the token array; entry e = tokens [off[e], off[e+1]) = (t_0 .. t_{n-1}), n <= LADE_GEN_MAX_SEQ_LEN
 *   cons[LADE_CONS_BIAS ..]     fp32 bits of the entries' biases (finite or -inf)
 *   cons[LADE_CONS_TOK ..]      the entries' tokens, packed
 *   cons[LADE_CONS_BAN ..]      ban bitmap, ceil(V/32) words: bit t = token t is -inf on every row; behind it the begin-ban bitmap, the
 *                               same size: bit t = token t is -inf on a row whose input length L == begin_index
 * Table order: the length-1 entries first, then the longer ones, each group in the order of HF's dict - the order in which HF's
 * SequenceBiasLogitsProcessor sums them (length_1_bias, then the dict's longer entries). */
#define LADE_GEN_MAX_SEQ_LEN 16         /* tokens of one sequence entry */
#define LADE_GEN_MAX_SEQ 1024           /* sequence entries (length-1 -inf entries live in the ban bitmap and do not count) */
#define LADE_GEN_CONS_MAX_VOCAB (3 << 16)   /* with constraints a row stages a second bitmap and the fired entries in LDS: <= 64 KiB */
#define LADE_CONS_N_SEQ 0
#define LADE_CONS_N_ONE 1
#define LADE_CONS_BEGIN_INDEX 2
#define LADE_CONS_FLAGS 3
#define LADE_CONS_TAIL_N 4
#define LADE_CONS_TAIL 8
#define LADE_CONS_OFF (LADE_CONS_TAIL + LADE_GEN_MAX_SEQ_LEN)
#define LADE_CONS_BIAS (LADE_CONS_OFF + LADE_GEN_MAX_SEQ + 8)
#define LADE_CONS_TOK (LADE_CONS_BIAS + LADE_GEN_MAX_SEQ)
#define LADE_CONS_BAN (LADE_CONS_TOK + LADE_GEN_MAX_SEQ * LADE_GEN_MAX_SEQ_LEN)
#define LADE_GEN_CONS_WORDS(V) (LADE_CONS_BAN + 2 * (((V) + 31) / 32))
#define LADE_CONS_F_ADD 1

/* Writes the block: penalty (> 0, double: the value HF holds) / min_len (>= 0) / the min-length EOS ids (host array, n_eos <= LADE_GEN_MAX_EOS), and the seen set =
 * the n_prompt prompt tokens (device).  Once per sequence, before its first step.  Detaches a constraint block (gen[LADE_GEN_CONS ..] = 0). */
int lade_gen_ctl_init(int32_t* gen, int32_t V, double penalty, int32_t min_len, const int32_t* eos_ids, int32_t n_eos,
                      const int32_t* prompt, int32_t n_prompt, void* stream);
/* Writes the constraint block `cons` and attaches it to `gen`: once per sequence, after lade_gen_ctl_init, in place (no re-capture).
 * Host arrays: ban_ids[n_ban] (-inf on every row; no cap; ids >= V are ignored, as HF's isin does), begin_ids[n_begin] with begin_index
 * (-inf on a row of input length L == begin_index), and the sequence entries in HF's dict order: seq_off[n_seq + 1] offsets into seq_tok,
 * seq_bias[n_seq] (finite or -inf; NaN and +inf are refused).  add_bias != 0: a SequenceBias / NoBadWords class is present
 * (LADE_CONS_F_ADD).  prompt (device, n_prompt tokens) seeds the tail.  LADE_E_ARG with the cap in the message for n_seq >
 * LADE_GEN_MAX_SEQ, an entry longer than LADE_GEN_MAX_SEQ_LEN tokens or V > LADE_GEN_CONS_MAX_VOCAB.  Synchronises the stream (the host
 * arrays are staged and copied). */
int lade_gen_constraints_init(int32_t* gen, int32_t* cons, int32_t V, const int32_t* ban_ids, int32_t n_ban, const int32_t* begin_ids,
                              int32_t n_begin, int32_t begin_index, const int32_t* seq_off, const int32_t* seq_tok, const float* seq_bias,
                              int32_t n_seq, int32_t add_bias, const int32_t* prompt, int32_t n_prompt, void* stream);
/* Adds the tokens the last post-step accepted (ctl[LADE_CTL_HITS ..], ctl[LADE_CTL_N_ACCEPT] of them) to the seen set, and shifts them
 * into the tail of an attached constraint block: after every post-step, inside a captured step too (no host round trip). */
int lade_gen_ctl_update(int32_t* gen, const int32_t* ctl, void* stream);
/* Row argmax of one step under the controls.  logits [rows][ld] (model dtype), rows = [out row | n_inp window rows | candidate rows, gs
 * positions each]; candidate slots c >= ctl[LADE_CTL_G] are padding (am = 0, nothing else written).  Row r predicts the token at sequence
 * length L = pos[sel ? sel[r] : r] + 1 (pos / sel: the step's position ids and row selection, device).  Penalised set: the seen set,
 * plus guess[c][0..j] for position j of candidate c; window rows use the seen set alone (they feed the window and the pool, never an
 * emitted token).  Per row in fp32: s -> s < 0 ? s * p : s * inv once per distinct token of the set, then -inf for the EOS ids when
 * L < min_len; am[r] = the argmax in torch.argmax's order.  One pass over the logits, no fp32 copy.
 * With a constraint block attached, per row: first the sequence-bias sum - an entry (t_0 .. t_{n-1}) -> b fires on a row with L >= n whose
 * last n-1 input_ids (the tail, then guess[c][0..j]) equal t_0 .. t_{n-2}; the fp32 sum per end token starts at 0 and takes the fired
 * entries in table order, and is added to the score in one add - then the penalty, then -inf for the ban bitmap, for the begin-ban bitmap
 * when L == begin_index, and for the min-length EOS ids.  Window rows take the ban bitmap and the length-1 entries only.  One work-group
 * thread per entry resolves the row's fired entries into LDS before the pass. */
int lade_gen_argmax(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, int32_t n_inp, int32_t gs,
                    const int32_t* gen, const int32_t* ctl, const int32_t* guess, const int32_t* pos, const int32_t* sel,
                    int32_t* am, void* stream);
/* The same, plus the processed fp32 rows of the out row and the candidate rows: rows_out[0] = out row, rows_out[1 + c*gs + j] =
 * position j of candidate c (row stride V; padded candidate slots are not written) - what lade_softmax_gather / lade_warp_rows read
 * with dtype LADE_F32 and skip = 0 (sampling). */
int lade_gen_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, int32_t n_inp, int32_t gs,
                  const int32_t* gen, const int32_t* ctl, const int32_t* guess, const int32_t* pos, const int32_t* sel,
                  int32_t* am, float* rows_out, void* stream);

/* ---- emitted rows (generate(return_dict_in_generate=True, output_scores / output_logits)) ---------------------------------------------
 * HF returns, per generated token, the fp32 row that decided it: `logits` = the model's row (`.to(float32)`), `scores` = that row after
 * the logits processors / warpers.  A lookahead step emits 1 .. gs + 1 tokens; which rows decided them:
 *   token 0 of a step      the out row:                       raw row 0,                         processed row 0
 *   token k >= 1           position k-1 of the accepted candidate c:  raw row 1 + n_inp + c*gs + (k-1),   processed row 1 + c*gs + (k-1)
 * (raw = the step's materialised logits [out | n_inp window rows | candidate rows], model dtype; processed = the rows_out layout of
 * lade_gen_rows / lade_warp_rows, fp32, no window rows).
 * The destinations live in a device descriptor of LADE_EMIT_WORDS int64 words, never in kernel arguments, so a captured step appends to
 * whatever buffers the descriptor names at replay:
 *   desc[LADE_EMIT_SCORES], desc[LADE_EMIT_LOGITS]   destination buffers, fp32 [cap_rows][ld] (either may be null: not written)
 *   desc[LADE_EMIT_CAP]    rows the buffers hold        desc[LADE_EMIT_LD]   their row stride in elements (= V)
 *   desc[LADE_EMIT_COUNT]  rows appended so far; it keeps counting beyond cap_rows (rows at or beyond the capacity are not written), so the
 *                          host detects an overflow by reading it */
#define LADE_EMIT_SCORES 0
#define LADE_EMIT_LOGITS 1
#define LADE_EMIT_CAP 2
#define LADE_EMIT_LD 3
#define LADE_EMIT_COUNT 4
#define LADE_EMIT_WORDS 8
/* Writes the descriptor (counter = 0): once per generate() call, in place - no re-capture.  At least one destination must be non-null. */
int lade_emit_init(int64_t* desc, float* scores_buf, float* logits_buf, int64_t cap_rows, int32_t V, void* stream);
/* Appends the rows of the tokens one step emitted, in emission order, at desc[LADE_EMIT_COUNT], then advances the counter (a one-thread
 * launch behind the row kernel).  raw [..][raw_ld] in raw_dtype, widened to fp32 (exact).  proc (nullable) fp32 [..][proc_ld]: the source of
 * `scores`; null = scores are the widened raw rows (greedy without controls: HF's scores and logits hold the same values).
 * Which rows: idx == NULL (greedy, also inside a captured step, behind the post-step): n = ctl[LADE_CTL_N_ACCEPT] tokens of candidate
 * ctl[LADE_CTL_MAX_HIT_IDX], read on the device.  Otherwise idx is a HOST array copied into the launch: n_idx (1 .. gs + 1) tokens, token
 * k >= 1 from candidate idx[k] (idx[0] is not read) - the sampling path, whose verify runs on the host.
 * Grid (gs + 1 token slots) x (column blocks); a slot at or above n exits at once.  16-byte loads and stores where V, the strides and the
 * pointers allow them, a scalar tail otherwise; plain stores only. */
int lade_emit_rows(int64_t* desc, const void* raw, int64_t raw_ld, int32_t raw_dtype, int32_t n_inp, int32_t gs, const float* proc,
                   int64_t proc_ld, const int32_t* ctl, const int32_t* idx, int32_t n_idx, int32_t V, void* stream);

/* lookahead parallelism: record packing, then (after the all-gather of rec_words int32 per rank, lade_lp_allgather
 * or the host's collective) the deterministic reduction every rank applies (same phases as above).
 * rec = [first_guess, n_inp, g_local, 0 | new tokens[split] | argmax ids of the rank's g_local*gs candidate rows];
 * rec_words >= 4 + split + g_local*gs.  The candidates are verified inside lade_lp_reduce_apply, on the gathered rows,
 * against RANK 0's first token - the reference broadcasts `next_tokens` from rank 0 before verifying
 * (lade/decoding.py:1024, :1071-1096) - so every rank takes the same decision even when 16-bit logits round
 * differently from rank to rank.  scratch: int32[R*split + G*gs].  pool_from_prompt / tail: as in
 * lade_greedy_post_step (the EOS scan and the POOL_FROM_PROMPT appends of lade/decoding.py:1167-1177 run identically on
 * every rank; eos: ONE end-of-sequence id, < 0 = no scan); record[1] = n_accept, record[2] = finished, record[5] = winning rank.  lade_lp_pack with ctl != NULL derives g_local
 * from ctl[LADE_CTL_G] and (lp_rank, lp_world) on the device (graph replay; pass g_local = the padded row count's candidates). */
int lade_lp_pack(const int32_t* am_out, const int32_t* am_inp, int32_t n_inp, const int32_t* am_guess, int32_t g_local,
                 int32_t gs, int32_t split, int32_t* rec, int32_t rec_words, const int32_t* ctl, int32_t lp_rank, int32_t lp_world,
                 void* stream);
int lade_lp_reduce_apply(const int32_t* all_rec, int32_t R, int32_t rec_words, int32_t split, int32_t* ctl,
                         int32_t* window, int32_t wcap, int32_t* pool_tok, int32_t* pool_cnt, int32_t V, int32_t W,
                         int32_t N, int32_t G, int32_t phase, int32_t* guess_all, int32_t* scratch, int32_t* record,
                         int32_t pool_from_prompt, int32_t* tail, int32_t eos, void* stream);

/* The step's one collective and its communicator: RCCL over xGMI, bound at run time by soname (the process
 * keeps the RCCL instance it already carries, e.g. torch's).  Replaces dist.init_process_group (lade/utils.py:28-33) and the
 * per-step object collectives of lade/decoding.py:1024, :1057, :1090, :1096, :1106 for a caller without torch.distributed.
 *   lade_lp_unique_id    rank 0: 128 opaque bytes (ncclUniqueId) to hand to every rank over the host's own channel
 *   lade_lp_comm_create  every rank, after hipSetDevice on its GPU; *comm_out = opaque handle, the only persistent allocation of
 *                        the library; one handle per rank / process
 *   lade_lp_allgather    recv[r*words .. ] = rank r's send[0..words): ordered on `stream` (after lade_lp_pack, before
 *                        lade_lp_reduce_apply), in place allowed when send == recv + rank*words
 *   lade_lp_comm_count   number of ranks the communicator spans (ncclCommCount) - what `dist.get_world_size()` is for a caller of the
 *                        reference (lade/utils.py:33 asserts it against DIST_WORKERS); lade_lp_comm_create already refuses a
 *                        communicator whose span differs from `world`
 *   lade_lp_comm_destroy explicit release (the handle is freed even when RCCL reports an error)
 * Without an RCCL library in the process they return LADE_E_LIMIT. */
int lade_lp_unique_id(void* id128);
int lade_lp_comm_create(const void* id128, int32_t rank, int32_t world, void** comm_out);
int lade_lp_allgather(void* comm, const int32_t* send, int32_t* recv, int32_t words_per_rank, void* stream);
int lade_lp_comm_count(void* comm, int32_t* ranks_out);
int lade_lp_comm_destroy(void* comm);

/* ---- sampling helpers ------------------------------------------------------------------ */
/* probs[r][:] = softmax(logits[r][:] / temperature) in fp32 */
int lade_softmax_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, float temperature,
                      float* probs, void* stream);
/* Device side of the sampling verify (lade/decoding.py:484-540; K11 of SURVEY 8b).  logits: [..][ld] with logical row 0 = the
 * out row (physical row 0) and logical row 1 + c*gs + j = position j of candidate c (physical row 1 + c*gs + j + skip: the step's
 * logits hold the `skip` window rows between the out row and the candidate rows); padded candidate slots are ignored.  Per row the
 * softmax statistics of logits/temperature go to stats[row] = {max, sum of exponentials}; the probabilities the acceptance
 * loop consults are gathered into scal[row][g_cap]: row 0 -> P(first token of candidate c), row 1 + c'*gs + j (j < gs-1) ->
 * P(token j+1 of candidate c | the prefix candidate c' shares up to j).  guess: the candidates' tokens [g][gs] (device);
 * g is read from *g_dev when that is not null (hipGraph steps), capped by g_cap.  Nothing of size [rows][V] is written. */
int lade_softmax_gather(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, float temperature, int32_t skip,
                        const int32_t* guess, const int32_t* g_dev, int32_t g, int32_t gs, int32_t g_cap, float* scal,
                        float* stats, void* stream);

/* Logits warpers of the sampling path in one launch (lade/decoding.py:375-377: the reference admits exactly HF's Temperature, TopK and
 * TopP warpers, applied in that order through LogitsProcessorList at :443 / :488):  out[r][:] = top_p(top_k(logits[r'][:] / temperature))
 * in fp32 with removed tokens set to -inf, r' = r for r = 0 and r + skip behind it (the same row addressing as lade_softmax_gather).
 * top_k = 0 and top_p >= 1 switch the respective filter off.  Tie rules of the HF warpers: values equal to the k-th largest stay; the
 * nucleus cut walks the ascending order with ties in token order and always keeps the last token.  Up to V = 32768 one work-group holds a
 * row in registers; a larger vocabulary (Llama-3 class) keeps the row's keys in the output row and settles two bits of a cut-off per pass
 * (same results; 0.4 ms for 31 rows of 128256 against 0.8 ms of torch topk / sort).  V <= 2^24. */
int lade_warp_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, float temperature, int32_t top_k,
                   float top_p, int32_t skip, float* out, void* stream);
/* The same launch with the rest of the truncation warpers generate() builds behind top-p (transformers generation/utils.py
 * _get_logits_processor: MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper of generation/logits_process.py, in
 * that order; the reference refuses them, lade/decoding.py:375-377).  Each stage acts on the survivors of the one before, with masses
 * E = round(exp(x - max) * 2^40), Z = sum E and entropy H = log(Z / 2^40) + sum E (max - x) / Z all in 64-bit fixed point, so no cut depends
 * on the order of a summation and both kernel forms place the same ones:
 *   min_p            remove p < min_p * p_max                                  (E < min_p * 2^40; 0 = off)
 *   typical_p        keep the tokens whose |-log p - H| (fp32) is at most D, the smallest distance with mass(d <= D) >= typical_p; a tie
 *                    group in d stays or goes whole; the largest token may go      (>= 1 = off)
 *   epsilon_cutoff   remove p < epsilon unless x equals the maximum              (0 = off)
 *   eta_cutoff       the same with eta = min(epsilon, sqrt(epsilon) * exp(-H))   (0 = off)
 * (filter_value = -inf and min_tokens_to_keep = 1 of the HF classes.)  With all four off this is lade_warp_rows: the same kernels.  With one
 * of them on, the output-row form of the kernel runs at every V (the register form has no registers left for the stages).
 * LADE_E_ARG, before any launch, for params == NULL, min_p outside [0, 1], typical_p outside (0, 1], a cutoff outside [0, 1). */
typedef struct lade_warp_params {
    float temperature;
    int32_t top_k;
    float top_p;
    float min_p;
    float typical_p;
    float epsilon_cutoff;
    float eta_cutoff;
} lade_warp_params;
int lade_warp_rows_ex(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t dtype, const lade_warp_params* params, int32_t skip,
                      float* out, void* stream);

/* ---- glue around the GEMMs -------------------------------------------------------------- */
/* y = weight * (x * rsqrt(mean(x^2) + eps)) with the reference's rounding (fp32 norm, cast, then * weight) */
int lade_rmsnorm(const void* x, const void* weight, void* y, int32_t rows, int32_t hidden, float eps, int32_t dtype,
                 void* stream);
/* the embedding lookup of a step (lade/models/modeling_llama.py:1413 `embed_tokens(input_ids)`) fused with the first layer's input norm
 * (:857): x[r] = table[ids[r]] (ids clamped to the table), y[r] = rmsnorm(x[r]) - one launch instead of a row gather and a norm */
int lade_embed_rmsnorm(const void* table, int32_t table_rows, const int32_t* ids, void* x, const void* weight, void* y, int32_t rows,
                       int32_t hidden, float eps, int32_t dtype, void* stream);
/* Residual add fused with the norm of the sum: y = rmsnorm(x + res).
 * The residual - exactly one of the two, both or neither is LADE_E_ARG:
 *   r       the residual rows in the model dtype;
 *   parts   a GEMM output as n_parts >= 1 fp32 split-K partials [n_parts][rows of x][hidden], part_stride elements apart, summed in split
 *           order and rounded once to the model dtype - the split-K GEMM needs no reduce pass.  bf16 / f16 only (LADE_E_DTYPE otherwise).
 * sel (nullable) selects the rows:
 *   null    every row r < rows: x[r] <- x[r] + res[r] in place, y[r] = rmsnorm(x[r]); src_rows is ignored;
 *   sel     device int32[rows], the row-pruned tail of a step (the reference norms and projects all T rows, lade/models/modeling_llama.py:
 *           1541-1544; only the out row, the last level's rows and the candidate rows are ever read): y[j] = rmsnorm(x[sel[j]] + res[sel[j]])
 *           for j < rows, x [src_rows][hidden] is read only.  One launch instead of a partial fold, two row gathers and a norm. */
int lade_add_rmsnorm(void* x, const void* r, const float* parts, int32_t n_parts, int64_t part_stride, const int32_t* sel, int32_t src_rows,
                     const void* weight, void* y, int32_t rows, int32_t hidden, float eps, int32_t dtype, void* stream);
/* SwiGLU of LlamaMLP (lade/models/modeling_llama.py:360-380) on the output of the fused gate/up GEMM, rounded like the separate torch ops.
 * layout 0: gu rows are [gate (inter) | up (inter)]: out[r][i] = silu(gu[r][i]) * gu[r][inter + i].
 * layout 1: groups of 16 - [16 gate | their 16 up] per 32 columns: out[r][i] = silu(gu[r][32*(i/16) + i%16]) * gu[r][32*(i/16) + 16 + i%16]
 *           (the row order in which the step engine fuses the two weights, so that lade_gemm_skinny's SwiGLU epilogue is lane-local).
 * The input - exactly one of the two, both or neither is LADE_E_ARG: gu [rows][2*inter] in the model dtype, or that GEMM output as n_parts >= 1
 * fp32 split-K partials [n_parts][rows][2*inter], part_stride elements apart, summed in split order and rounded once to the model dtype
 * (bf16 / f16 only: LADE_E_DTYPE otherwise). */
int lade_silu_mul(const void* gu, const float* parts, int32_t n_parts, int64_t part_stride, void* out, int32_t rows, int32_t inter, int32_t layout,
                  int32_t dtype, void* stream);
/* dst[r][:] = src[idx[r]][:]  (row gather: embedding lookup, logits-row selection) */
int lade_gather_rows(const void* src, const int32_t* idx, void* dst, int32_t rows, int32_t width, int32_t elem_bytes,
                     int32_t src_rows, void* stream);

/* ---- skinny weight-streaming GEMM -------------------------------------
 * C[M,N] = A[M,K] . W[N,K]^T for the projections of a decode step (M = T <= ~256 rows), bf16 / f16, fp32 accumulate.
 * n_split == 1: writes C (model dtype).  n_split > 1: writes fp32 partials Cpart[n_split][M][N] (summed in split
 * order - deterministic - by lade_splitk_reduce).  bn = weight rows per work-group (32..256), mb = 32-row activation
 * blocks per work-group (1: 32 rows, 2: 64, 3: 96, 4: 128, 0: by M; larger M runs as several row blocks).  mt = 32-row activation blocks per WAVE (0 | 1..4, divides
 * mb) and nt = 32-row weight tiles per wave (0 = fewest): the waves form an (mb/mt) x (bn/32/nt) grid; larger wave tiles
 * re-read less from LDS per weight byte.  ring = stages of the LDS ring the tiles arrive in (0 = default: 4 where they fit; 2, 3, 4, 5, 6, 8): a
 * deeper ring keeps more bytes in flight per work-group and leaves room for fewer co-resident work-groups - chosen per projection by the
 * caller's autotune.  Unsupported shapes return LADE_E_ARG.  K % 64 == 0.  M > 256 runs as several 256-row blocks per launch (bn = 256,
 * mb = 8, nt = 2 | 4 is a compute-shaped 256 x 256 tile on a double buffer).
 * epilogue (n_split == 1 only): 0 = none; 1 = SwiGLU - W is the fused gate/up weight in the 16-row interleaved order of
 * lade_silu_mul's layout 1 and C is [M][N/2] = silu(gate) * up (the SwiGLU kernel and the fp32 partials of a split-K
 * gate/up GEMM disappear from the step); 2 = row argmax (the lm_head of a greedy step, lade/models/modeling_llama.py:1541-1544 +
 * torch.argmax at lade/decoding.py:1021): C is not written (may be null), Cpart receives one {float value, int32 column} pair per row
 * and column block - Cpart[(m * ceil(N / bn) + block) * 2] - the value rounded to the model dtype, the lowest column among equal
 * values; lade_argmax_pairs merges a row's pairs.  The [rows, V] logits never reach HBM. */
int lade_gemm_skinny(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, float* Cpart,
                     int32_t M, int32_t N, int32_t K, int32_t n_split, int32_t bn, int32_t mb, int32_t mt, int32_t nt,
                     int32_t ring, int32_t epilogue, int32_t dtype, void* stream);
/* The same GEMM on a weight stored K-TILE-MAJOR: Wkt[K/64][N][64], i.e. Wkt[kt][n][j] = W[n][64 kt + j] - the 128-byte segments of all N
 * rows of one 64-deep K tile are contiguous.  Row-major nn.Linear weights (lade/models/modeling_llama.py:360-380, 492-494, 558) make a
 * work-group's K tile BN separate 128-byte reads K elements apart; K-tile-major makes it ONE contiguous BN x 128 bytes, and the
 * work-groups of a split sweep memory linearly as they walk along K.  Same arithmetic in the same order: results are bit-identical to
 * lade_gemm_skinny.  lade_weight_to_ktile builds the copy once at load time (out of place; K % 64 == 0). */
int lade_gemm_skinny_kt(const void* A, int64_t lda, const void* Wkt, void* C, int64_t ldc, float* Cpart,
                        int32_t M, int32_t N, int32_t K, int32_t n_split, int32_t bn, int32_t mb, int32_t mt, int32_t nt,
                        int32_t ring, int32_t epilogue, int32_t dtype, void* stream);
/* The qkv projection of a decode step finished in ONE launch: the split-K GEMM with two K slices (the grid, slices and ring of lade_gemm_skinny(_kt) with
 * n_split = 2), whose two work-groups per (n-block, m-block) reduce their pair themselves - each leaves its fp32 tile in Cpart with write-through stores and draws
 * a ticket; the second to arrive reads the other tile, forms (0 + split 0) + split 1, rounds once to the model dtype and does what lade_rope_kv_append does
 * with that value: q rotated to q_out [M][H*d], rotated k to K cache rows P .. P+M-1, v to the V^T cache.  Bit-identical to the two launches it replaces; no
 * epilogue (bias / head norm) and no fp32.  Nothing spins and no co-residency is assumed.  The kernel streams the weight rows of a q or k head in PAIR ORDER
 * (lade_qkv_pair_row) so that a rotation pair meets in one lane; W itself is the plain fused [q | k | v] weight, row-major (ktile = 0) or K-tile-major.
 * Cpart: hand-off space of cpart_elems floats, >= ceil(N/bn) * ceil(M/(32 mb)) * 2 * 32 mb * bn (its contents afterwards are private to the kernel).
 * tickets: n_tickets >= ceil(N/bn) * ceil(M/(32 mb)) int32, ZERO before the first launch; every launch leaves them zero (graph replays need no memset).
 * bn a multiple of 32, mb, mt, nt explicit (>= 1); built for bn = 96, nt = 1 and (mb, mt) = (1,1), (2,1), (3,3), (4,2): anything else is LADE_E_ARG.
 * d % 32 == 0, N == (H + 2 Hkv) d, K >= 128. */
typedef struct lade_qkv_rope_args {
    void* q_out;
    const int32_t* positions;     /* [M] */
    const void* cos_tab;          /* [max_pos][d], model dtype */
    const void* sin_tab;
    void* k_cache;                /* [Hkv][S_max][d] */
    void* vt_cache;               /* [Hkv][d][S_max] */
    const int32_t* dyn_P;         /* nullable: P read from the device (hipGraph steps); a step that would pass S_max writes nothing */
    int32_t P, H, Hkv, d, S_max, max_pos;
} lade_qkv_rope_args;
int lade_gemm_qkv_rope(const void* A, int64_t lda, const void* W, int64_t ldw, int32_t ktile, float* Cpart, int64_t cpart_elems, int32_t* tickets,
                       int32_t n_tickets, int32_t M, int32_t N, int32_t K, int32_t bn, int32_t mb, int32_t mt, int32_t nt, int32_t ring,
                       const lade_qkv_rope_args* rope, int32_t dtype, void* stream);
/* weight row that lands in row n of the fused kernel's tile order: per 32-row block of a q / k head [rows 16 b .. 16 b + 15 | rows d/2 + 16 b .. d/2 + 16 b + 15],
 * v rows in place; -1 for arguments out of range (d % 32 != 0, n outside the fused weight).  Host only, no GPU needed. */
int lade_qkv_pair_row(int32_t n, int32_t H, int32_t Hkv, int32_t d);
int lade_weight_to_ktile(const void* W, int64_t ldw, void* Wkt, int32_t N, int32_t K, int32_t dtype, void* stream);
/* the inverse, into a caller-provided row-major scratch W[N][ldw]: what a library GEMM needs (prefill chunks wider than 256 rows) when a
 * model too large to be held twice keeps its projection weights K-tile-major only */
int lade_weight_from_ktile(const void* Wkt, void* W, int64_t ldw, int32_t N, int32_t K, int32_t dtype, void* stream);
/* the reduce pass of a split-K GEMM whose consumer does not take the partials itself (lade_rope_kv_append, lade_add_rmsnorm and
 * lade_silu_mul do): C = the n_split partials summed in split order, rounded once to the model dtype */
int lade_splitk_reduce(const float* part, void* C, int64_t ldc, int32_t M, int32_t N, int32_t n_split, int32_t dtype,
                       void* stream);

/* ---- misc ------------------------------------------------------------------------------- */
int lade_version(void);
const char* lade_last_error_string(void);
/* kernel timing helper for bench.py: runs `reps` launches of lade_attn_fwd (+combine) on `stream`
 * bracketed by hipEvents and returns the mean duration of one launch pair in microseconds. */
int lade_time_attn(const lade_attn_args* a, int32_t reps, float* mean_us, void* stream);
/* the same over n argument sets used round-robin (a[i % n] in repetition i): n K/V caches larger than the Infinity
 * Cache in total make every launch stream from HBM, as consecutive layers of a decode step do */
int lade_time_attn_rot(const lade_attn_args* a, int32_t n, int32_t reps, float* mean_us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LADE_HIP_H */
