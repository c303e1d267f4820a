/*
 * fa_mi355x.h -- C ABI of the MI355X (gfx950) flash-attention forward library
 * (libfa_mi355x.so, built from exploring_flash_attention_amd/csrc/).
 *
 * Computes the exact attention forward O = softmax(Q K^T / sqrt(d)) V over contiguous
 * row-major [B, H, L, d] tensors held in device memory (HBM): non-causal (every query row
 * attends to every key) in all entry points but fa_fwd_v1_causal, which masks row i to keys
 * 0..i (the reference has no causal mode).
 * All entry points are asynchronous on the caller's HIP stream (pass NULL for the
 * null stream), never allocate, never synchronise the device, and return an
 * fa_status_t.  On failure fa_last_error() returns a thread-local message.
 *
 * Each entry point replaces one host launcher of the reference
 * (tyler-utah/exploring_flash_attention, paths relative to its root):
 *
 *   fa_fwd_v1          <- flash_attention_v1(Q,K,V,O,B,H,L,d)
 *                           flash_attention_v1/CUDA/flash_attention_v1.h:251
 *                         flash_attention_v1_opt1(Q,K,V,O,B,H,L,d)
 *                           flash_attention_v1/CUDA/flash_attention_v1_opt1.h:354
 *   fa_fwd_v1_tiled_d  <- flash_attention_v1(Q,K,V,O,B,H,L,d,d_tile_qk,d_tile_v)
 *                           flash_attention_v1_tiled_d/CUDA/flash_attention_v1.h:312
 *                         flash_attention_v1_opt(...)
 *                           flash_attention_v1_tiled_d/CUDA/flash_attention_v1_opt.h:448
 *   fa_fwd_v2_workspace_size + fa_fwd_v2
 *                      <- flash_attention_v2(Q,K,V,O,B,H,L,d,d_tile_qk,d_tile_v,kv_tiles_per_block)
 *                           flash_attention_v2/CUDA/flash_attention_v2.h:438 (opt: _opt.h:559)
 *                         The reference cudaMallocs/frees its workspace inside every call
 *                         (flash_attention_v2.h:461-463, :506-508); here the caller owns it.
 *   fa_fwd_partial     <- partial_attention_kernel  flash_attention_v2/CUDA/flash_attention_v2.h:243
 *   fa_combine         <- reduction_kernel          flash_attention_v2/CUDA/flash_attention_v2.h:356
 *                         (exposed separately so a multi-GPU caller can put an RCCL exchange
 *                         between the two kernels; the reference has no multi-GPU path)
 *
 * Differences from the reference contract, all deliberate:
 *   - the reference launchers return void, assert() on bad arguments and end with
 *     cudaDeviceSynchronize(); these return a status and never synchronise;
 *   - the reference element type is __half (or double under USE_FP64); here the
 *     element type is a runtime argument (FA_DTYPE_BF16, FA_DTYPE_FP16 or FA_DTYPE_FP64);
 *   - the reference fixes the head dim at compile time (assert(d == D),
 *     flash_attention_v1/CUDA/flash_attention_v1.h:264); here d is dispatched at run
 *     time to kernels for d in {32, 64, 128, 256} and, through fa_fwd_v1 / fa_fwd_v1_tiled_d
 *     and the unsplit fa_fwd_v2, the d-tiled kernels for d in {384, 512}; any other d returns
 *     FA_ERR_UNSUPPORTED (the *_scaled entry points let a caller zero-pad any d <= 512);
 *   - sizes are int64_t and every offset is 64-bit (the reference overflows int32 in
 *     its workspace index at L=4096, flash_attention_v2/CUDA/flash_attention_v2.h:324).
 */
#ifndef FA_MI355X_H
#define FA_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum fa_status {
    FA_OK = 0,
    FA_ERR_INVALID_ARG = 1,  /* null pointer, non-positive size, bad tile argument */
    FA_ERR_UNSUPPORTED = 2,  /* head dim / dtype without a kernel */
    FA_ERR_HIP = 3,          /* a HIP runtime call failed (launch, attribute) */
    FA_ERR_WORKSPACE = 4     /* workspace missing or smaller than fa_fwd_v2_workspace_size */
} fa_status_t;

typedef enum fa_dtype {
    FA_DTYPE_FP16 = 0,       /* IEEE binary16 storage, fp32 accumulate */
    FA_DTYPE_BF16 = 1,       /* bfloat16 storage, fp32 accumulate */
    FA_DTYPE_FP32 = 2,       /* only valid as the split-KV partial-output type */
    FA_DTYPE_FP16_SCALED = 4, /* only as a partial-output type (fa_fwd_v2, fa_fwd_partial,
                                 fa_combine): fp16 partials scaled per row by a power of two
                                 (the row's largest |value| below 1), the exponent kept beside
                                 the lse -- half the traffic of FA_DTYPE_FP32, 11 significant
                                 bits relative to each row's maximum, no fp16 range limit */
    FA_DTYPE_FP64 = 3        /* IEEE binary64 throughout (the reference's USE_FP64 build,
                                flash_attention_v1/CUDA/flash_attention_v1.h:29-41): fp64
                                MFMA, fp64 softmax, fp64 partials and lse */
} fa_dtype_t;

/* ABI version.  Callers built against one minor version must rebuild for another:
 *   0.2 -- fa_fwd_v2_ex and fa_fwd_v2_split_plan gained the int blocks_per_workgroup argument
 *          (inserted before workspace / dtype), fa_fwd_v2_workspace_size_ex was added;
 *   0.3 -- head dims 384 and 512 (the d-tiled kernels: fa_fwd_v1, fa_fwd_v1_tiled_d, and
 *          fa_fwd_v2 unsplit), fa_fwd_v1_tiled_d_scaled added;
 *   0.4 -- fa_last_kernels and fa_fwd_v2_ex2 (FA_V2_COUNTERS_ZERO) added (no signature changed);
 *          fa_fwd_v1_causal added later under the same number (an addition only: callers built
 *          against 0.4 stay valid; a library without it fails to resolve the symbol);
 *          fa_fwd_v1_gqa and FA_FWD_CAUSAL added the same way; then fa_fwd_decode_plan and
 *          fa_fwd_decode (KV-cache decode), again additions only; then fa_fwd_decode_paged (the
 *          same forward through a block table), an addition only; then fa_fwd_varlen (token-packed
 *          ragged batches through a device-side cu_seqlens), an addition only; then
 *          fa_fwd_varlen_kv (the same with key lengths of their own), an addition only; then
 *          fa_fwd_varlen_paged (those keys in a paged pool) and fa_kv_append_paged, additions only.
 * fa_version() returns the library's (major << 16) | (minor << 8) | patch; check it against
 * these macros at load time. */
#define FA_MI355X_VERSION_MAJOR 0
#define FA_MI355X_VERSION_MINOR 4
int fa_version(void);

/* Thread-local message describing the last non-FA_OK status on this thread. */
const char* fa_last_error(void);

/* Thread-local description of the kernels the last launching call on this thread enqueued
 * (fa_fwd_v1*, fa_fwd_v1_tiled_d*, fa_fwd_v2*, fa_fwd_partial*, fa_combine), each with its
 * grid, joined by " + ", e.g. "fa_fwd16_chain_kernel<final> [grid 512]".  Valid after an FA_OK
 * return; the reference's launchers have no equivalent (a profiling aid: which of the
 * library's kernels and grids served the call, as the launcher chose them).  The grids of the
 * d = 128 persistent kernels are sized from the compute units of the device that owns
 * `stream`; the split-KV plan (fa_fwd_v2_split_plan, the workspace size) from the current
 * device's -- call them with the stream's device current. */
const char* fa_last_kernels(void);

/* Geometry the library uses for (d, dtype): query rows per workgroup (*bq),
 * keys per KV tile (*bk), threads per workgroup (*threads), LDS bytes per workgroup
 * (*lds_bytes).  Any output pointer may be NULL. */
int fa_kernel_geometry(int64_t d, int dtype, int* bq, int* bk, int* threads,
                       int* lds_bytes);

/* FA-v1 fused forward.  q, k, v, o: [B, H, L, d] contiguous, element type dtype.
 * d = 384 / 512 run the d-tiled kernel with 128-column tiles (fa_fwd_v1_tiled_d). */
int fa_fwd_v1(const void* q, const void* k, const void* v, void* o,
              int64_t B, int64_t H, int64_t L, int64_t d,
              int dtype, void* stream);

/* fa_fwd_v1 with an explicit softmax scale: O = softmax(softmax_scale * Q K^T) V.
 * softmax_scale > 0 and finite (else FA_ERR_INVALID_ARG); fa_fwd_v1 passes 1/sqrt(d).
 * Lets a caller run a head dim without its own kernel by zero-padding Q, K and V to a
 * supported d (zero columns add nothing to Q K^T; the padded O columns come out zero)
 * while keeping the scale of the true head dim -- the reference's Python functions take any
 * d (e.g. flash_attention_v1/numpy_gpu_like_opt2.py:198 with d = 16); the Python layer
 * (exploring_flash_attention_amd/ops.py) does exactly this. */
int fa_fwd_v1_scaled(const void* q, const void* k, const void* v, void* o,
                     int64_t B, int64_t H, int64_t L, int64_t d, double softmax_scale,
                     int dtype, void* stream);
/* fa_fwd_v1_scaled with a causal mask: row i attends to keys 0..i (top-left aligned; query
 * and key length are both L), O[i] = softmax(softmax_scale * Q[i] K[0..i]^T) V[0..i].  Every
 * row sees key 0, so no row is empty.  Contiguous [B, H, L, d], FA_DTYPE_BF16 or FA_DTYPE_FP16,
 * d in {32, 64, 128, 256}; d = 384 / 512 and FA_DTYPE_FP64 return FA_ERR_UNSUPPORTED (the
 * message names "causal").  Pointer, size and scale checks as fa_fwd_v1_scaled.  A query tile
 * of 128 rows walks only the keys up to its last row, so a long sequence does about half the
 * work of fa_fwd_v1.  fa_last_kernels: "fa_fwd_kernel<final, causal>".  The split-KV, d-tiled,
 * strided and multi-GPU entry points have no causal form. */
int fa_fwd_v1_causal(const void* q, const void* k, const void* v, void* o,
                     int64_t B, int64_t H, int64_t L, int64_t d, double softmax_scale,
                     int dtype, void* stream);
/* Grouped-query attention (GQA; H_kv = 1: MQA): q and o are [B, H, L, d], k and v
 * [B, H_kv, L, d] with H a multiple of H_kv, all contiguous, and query head h reads K/V head
 * h / (H / H_kv) -- what fa_fwd_v1_scaled computes on k, v with every head repeated H / H_kv
 * times in place (repeat_interleave along the head axis), bit for bit, without the copy.
 * flags: 0, or FA_FWD_CAUSAL for the mask of fa_fwd_v1_causal; any other bit returns
 * FA_ERR_INVALID_ARG (the message names "flags").  H_kv <= 0, H_kv > H or H % H_kv != 0 return
 * FA_ERR_INVALID_ARG (the message names "H_kv").  FA_DTYPE_BF16 or FA_DTYPE_FP16, d in
 * {32, 64, 128, 256}; d = 384 / 512 and FA_DTYPE_FP64 return FA_ERR_UNSUPPORTED (the message
 * names "gqa"); pointer, size, scale and alignment checks as fa_fwd_v1_scaled.  H_kv == H
 * forwards to fa_fwd_v1_scaled / fa_fwd_v1_causal (the same kernels, labels and bits).
 * Otherwise the call runs the kernel family fa_fwd_v1 / fa_fwd_v1_causal pick for the same
 * B, H, L, d, its fa_last_kernels label ending in ", gqa": "fa_fwd16_chain_kernel<final, gqa>",
 * "fa_fwd16_kernel<final, gqa>", "fa_fwd_kernel<final, gqa>", "fa_fwd_kernel<final, causal, gqa>".
 * The split-KV, d-tiled, strided and multi-GPU entry points take H_kv == H only. */
#define FA_FWD_CAUSAL 1u
int fa_fwd_v1_gqa(const void* q, const void* k, const void* v, void* o,
                  int64_t B, int64_t H, int64_t H_kv, int64_t L, int64_t d,
                  double softmax_scale, unsigned flags, int dtype, void* stream);
/* Variable-length (token-packed) self-attention: one launch for a ragged batch, no padding.
 * q and o are [total_tokens, H, d], k and v [total_tokens, H_kv, d] (H a multiple of H_kv, query
 * head h reads K/V head h / (H / H_kv)); cu_seqlens is an int32 [B + 1] array ON THE DEVICE and
 * sequence b owns token rows [cu_seqlens[b], cu_seqlens[b+1]) of all four tensors.  For token i
 * of sequence b at position p = i - cu_seqlens[b],
 *   O[i, h] = softmax(softmax_scale * Q[i, h] K[cu[b] .. cu[b] + n, h / G]^T) V[cu[b] .. cu[b] + n, h / G]
 * with n = the sequence's length, or p + 1 with FA_FWD_CAUSAL; sequences never see each other's
 * keys.  The lengths are read on the device only (no host read, no synchronisation), clamped:
 *   start_b = clamp(cu[b], 0, total_tokens),
 *   len_b   = clamp(cu[b+1] - start_b, 0, min(max_seqlen, total_tokens - start_b)),
 * so a corrupt or non-monotonic cu_seqlens gives a wrong result, never an access outside q, k, v
 * or o.  Rows of o that belong to no sequence (past cu[B], or past max_seqlen inside a sequence)
 * are never written; a zero-length sequence costs workgroups that exit at once.
 *   q_strides, kv_strides (shared by k and v), o_strides: two element strides {token, head} each,
 *     d contiguous, or NULL for contiguous [total_tokens, H, d] -- a slice of a fused
 *     [total_tokens, (H + 2 H_kv) d] QKV projection is {(H + 2 H_kv) d, d}, read in place.
 *     Positive multiples of 8 elements, token stride >= d and <= 2^20; bases 16-byte aligned.
 *   flags: 0 or FA_FWD_CAUSAL (other bits: FA_ERR_INVALID_ARG, the message names "flags").
 *   max_seqlen: an upper bound of the lengths (longer sequences are truncated to it); the grid
 *     is B * H * ceil(max_seqlen / 128) workgroups and must stay below 2^31 (FA_ERR_UNSUPPORTED,
 *     "grid").
 * FA_ERR_INVALID_ARG: a null pointer (cu_seqlens included) or misaligned one, H_kv not dividing
 * H, B <= 0, max_seqlen <= 0, total_tokens < 0, a scale that is not positive and finite, bad
 * strides.  FA_ERR_UNSUPPORTED: d outside {32, 64, 128, 256}, FA_DTYPE_FP64 (the message names
 * "varlen"), total_tokens > 2^31 - 1.  total_tokens == 0 returns FA_OK without a launch.
 * fa_last_kernels: "fa_fwd_kernel<final, varlen[, causal][, gqa]>" with its grid. */
int fa_fwd_varlen(const void* q, const void* k, const void* v, void* o, const int32_t* cu_seqlens,
                  int64_t B, int64_t total_tokens, int64_t max_seqlen, int64_t H, int64_t H_kv, int64_t d,
                  const int64_t* q_strides, const int64_t* kv_strides, const int64_t* o_strides,
                  double softmax_scale, unsigned flags, int dtype, void* stream);
/* fa_fwd_varlen with key lengths of their own: chunked prefill against a prefix, prefix caching,
 * verification of a long draft, ragged cross-attention.  q and o are [total_tokens, H, d] and
 * cu_seqlens / max_seqlen describe them as above; k and v are [total_tokens_k, H_kv, d] and
 * cu_seqlens_k (int32 [B + 1] on the device) says which of their rows are sequence b's keys, at
 * most max_seqlen_k of them (longer ranges are truncated).  seqused_k, int32 [B] on the device or
 * NULL, cuts sequence b's keys to the first seqused_k[b] rows of its range -- a padded
 * [B, Lmax, H_kv, d] cache is read in place as [B * Lmax, H_kv, d] with cu_seqlens_k[b] = b * Lmax.
 * Clamped on the device like the query side, in 64-bit arithmetic:
 *   start_k = clamp(cu_k[b], 0, total_tokens_k),
 *   len_k   = clamp(cu_k[b+1] - start_k, 0, min(max_seqlen_k, total_tokens_k - start_k)),
 *   len_k   = min(len_k, max(seqused_k[b], 0))   where seqused_k is given,
 * so start_k + len_k <= total_tokens_k whatever the arrays hold, and every K / V read lies in rows
 * [start_k, start_k + len_k).  With len_q the query length and s = len_k - len_q, query position
 * i sees every key, or with FA_FWD_CAUSAL keys j <= i + s: the diagonal is aligned bottom-right,
 * as in fa_fwd_decode.  A row that sees no key (len_k = 0; causal with s < 0 and i < -s) is
 * written as zeros.  Rows of o that belong to no sequence are never written.  The grid is the
 * query side's, B * H * ceil(max_seqlen / 128).  kv_strides address k and v as in fa_fwd_varlen.
 * Errors as fa_fwd_varlen, and FA_ERR_INVALID_ARG for a null or misaligned cu_seqlens_k, a
 * misaligned seqused_k, max_seqlen_k <= 0, total_tokens_k < 0; FA_ERR_UNSUPPORTED for
 * total_tokens_k > 2^31 - 1.  k and v must be non-null even when total_tokens_k == 0 (they are not
 * read then).  With cu_seqlens_k = cu_seqlens on the same tokens the result is fa_fwd_varlen's,
 * bit for bit.  fa_last_kernels: "fa_fwd_kernel<final, varlen, kv[, causal][, gqa]>". */
int fa_fwd_varlen_kv(const void* q, const void* k, const void* v, void* o, const int32_t* cu_seqlens,
                     const int32_t* cu_seqlens_k, const int32_t* seqused_k, int64_t B, int64_t total_tokens,
                     int64_t total_tokens_k, int64_t max_seqlen, int64_t max_seqlen_k, int64_t H, int64_t H_kv,
                     int64_t d, const int64_t* q_strides, const int64_t* kv_strides, const int64_t* o_strides,
                     double softmax_scale, unsigned flags, int dtype, void* stream);
/* fa_fwd_varlen_kv with the keys in a PAGED pool, read in place through a block table: chunked and
 * prefix-cached prefill against the cache fa_fwd_decode_paged reads.  q and o are [total_tokens, H,
 * d] and cu_seqlens / max_seqlen describe them as in fa_fwd_varlen.  k_cache and v_cache are pools
 * of num_blocks blocks of page_size keys; a sequence's keys start at logical key 0 (there is no
 * cu_seqlens_k), key j of sequence b is row j % page_size of block
 *   clamp(block_table[b * table_stride + j / page_size], 0, num_blocks - 1),
 * and it has len_k = clamp(seqused_k[b], 0, max_seqlen_k) of them.  block_table (int32, table_stride
 * entries per sequence) and seqused_k (int32 [B], REQUIRED here) live on the device and are read
 * there only.  Only the table entries of pages that hold a key the call reads are loaded -- the
 * rest may be -1 or anything -- and every entry is clamped into the pool before it enters an
 * address: a corrupt table or length gives a wrong result, never an access outside the pool.
 *   cache_strides (shared by the pools): three element strides {block, head, row}, d contiguous,
 *     or NULL for contiguous [num_blocks, page_size, H_kv, d]; a [num_blocks, H_kv, page_size, d]
 *     pool is {H_kv * page_size * d, page_size * d, d}.  Positive multiples of 8 elements, row
 *     stride >= d and <= 2^20; bases 16-byte aligned.  One block must hold page_size rows of every
 *     head at these strides.
 *   page_size: a positive multiple of 64 keys, so that a KV tile (64 keys, 32 at d = 256) lies
 *     inside one page (other sizes: FA_ERR_UNSUPPORTED, the message names "page_size").
 *   max_seqlen_k: an upper bound of the key counts; table_stride >= ceil(max_seqlen_k / page_size).
 * Causal alignment (bottom-right), zero rows for rows that see no key, unwritten rows of no
 * sequence, q_strides / o_strides, flags and the grid B * H * ceil(max_seqlen / 128) are
 * fa_fwd_varlen_kv's.  The result is, bit for bit, fa_fwd_varlen_kv's on the cache gathered in
 * table order (the same tiles in the same order; only addresses differ).
 * Errors as fa_fwd_varlen for the shared arguments, and FA_ERR_INVALID_ARG for a null or misaligned
 * block_table or seqused_k, num_blocks <= 0, page_size <= 0, max_seqlen_k <= 0, table_stride below
 * ceil(max_seqlen_k / page_size), bad cache_strides.  total_tokens == 0 returns FA_OK without a
 * launch.  fa_last_kernels: "fa_fwd_kernel<final, varlen, paged[, causal][, gqa]>" with its grid. */
int fa_fwd_varlen_paged(const void* q, const void* k_cache, const void* v_cache, void* o,
                        const int32_t* cu_seqlens, const int32_t* block_table, const int32_t* seqused_k,
                        int64_t B, int64_t total_tokens, int64_t max_seqlen, int64_t max_seqlen_k,
                        int64_t H, int64_t H_kv, int64_t d,
                        int64_t num_blocks, int64_t page_size, int64_t table_stride,
                        const int64_t* q_strides, const int64_t* cache_strides, const int64_t* o_strides,
                        double softmax_scale, unsigned flags, int dtype, void* stream);
/* Appends a chunk's new K / V rows to the paged pool fa_fwd_varlen_paged and fa_fwd_decode_paged
 * read.  k_new and v_new are [total_tokens, H_kv, d] (new_strides: {token, head} shared by both, or
 * NULL for contiguous, under fa_fwd_varlen's kv_strides rules); cu_seqlens / max_seqlen say which
 * rows are sequence b's new tokens, clamped on the device exactly as fa_fwd_varlen clamps them
 * (start_b, len_b above).  seqused_k[b] is the sequence's key count AFTER the append -- the array
 * the attention call then takes -- so new token i of sequence b is logical key
 *   p = seqused_k[b] - len_b + i
 * and is copied to row p % page_size of block clamp(block_table[b * table_stride + p / page_size],
 * 0, num_blocks - 1) of both pools.  A token with p < 0 or p >= max_seqlen_k (the keys the table
 * maps; table_stride >= ceil(max_seqlen_k / page_size)) cannot be placed and is skipped.  Only rows
 * that a token owns are written; nothing is read on the host; the copy runs on `stream`.
 * d: any multiple of 8 up to 256 (else FA_ERR_UNSUPPORTED, "head dim"); FA_DTYPE_BF16 or
 * FA_DTYPE_FP16.  Pool, table, page_size and cache_strides checks as fa_fwd_varlen_paged; the grid is
 * B * ceil(max_seqlen / 32) * H_kv workgroups (those past a sequence's end exit) and must stay
 * below 2^31.  total_tokens == 0 returns FA_OK without a launch.
 * fa_last_kernels: "fa_kv_append_kernel" with its grid. */
int fa_kv_append_paged(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                       const int32_t* cu_seqlens, const int32_t* block_table, const int32_t* seqused_k,
                       int64_t B, int64_t total_tokens, int64_t max_seqlen, int64_t max_seqlen_k,
                       int64_t H_kv, int64_t d,
                       int64_t num_blocks, int64_t page_size, int64_t table_stride,
                       const int64_t* new_strides, const int64_t* cache_strides, int dtype, void* stream);
/* fa_fwd_v1_scaled on strided tensors.  q_strides, kv_strides (shared by k and v) and
 * o_strides each point to three element strides {batch, head, row} of a [B, H, L, d] view
 * whose d is contiguous -- e.g. a [B, L, H, d] tensor is {L*H*d, d, H*d} -- or are NULL for
 * contiguous [B, H, L, d].  Strides must be positive multiples of 8 elements (16-byte row
 * starts), row strides >= d, and one head's rows must span < 2 GiB; bf16 / fp16 only
 * (FA_DTYPE_FP64 with strides: FA_ERR_UNSUPPORTED).  No copy is made. */
int fa_fwd_v1_ex(const void* q, const void* k, const void* v, void* o,
                 int64_t B, int64_t H, int64_t L, int64_t d,
                 const int64_t* q_strides, const int64_t* kv_strides, const int64_t* o_strides,
                 double softmax_scale, int dtype, void* stream);
/* FA-v1 d-tiled forward.  d_tile_qk / d_tile_v must satisfy 0 < d_tile <= d
 * (the reference's asserts, flash_attention_v1_tiled_d/CUDA/flash_attention_v1.h:326-327),
 * otherwise FA_ERR_INVALID_ARG.  d in {32, 64, 128, 256, 384, 512}.
 *   d <= 256: one LDS tile holds a whole row, and the fused kernel runs (its QK^T accumulates
 *   32-column k-steps, its O stays in VGPRs); the tiles are validated and do not change it.
 *   d = 384 / 512 (the head dims the variant exists for): the d-tiled kernel streams each
 *   64-key K tile through LDS in [64][d_tile_qk] column chunks and each V tile in
 *   [64][d_tile_v] chunks, O_acc in VGPRs for all d columns; a tile is honoured at the MFMA's
 *   granularity -- rounded down to 32, 64 or 128 columns (at least 32).  QK^T sums the same
 *   k-steps in the same order whatever the tiles, so the output does not depend on them.
 * FA_DTYPE_FP64 takes the same paths in fp64 (d = 384 / 512: 16-key tiles, Q chunks re-read
 * per tile as the reference does, :159-164). */
int fa_fwd_v1_tiled_d(const void* q, const void* k, const void* v, void* o,
                      int64_t B, int64_t H, int64_t L, int64_t d,
                      int d_tile_qk, int d_tile_v,
                      int dtype, void* stream);
/* fa_fwd_v1_tiled_d with an explicit softmax scale (as fa_fwd_v1_scaled: lets a caller zero-pad
 * a head dim without its own kernel, e.g. 257..511, to 384 or 512; the tiles are checked
 * against the d passed here). */
int fa_fwd_v1_tiled_d_scaled(const void* q, const void* k, const void* v, void* o,
                             int64_t B, int64_t H, int64_t L, int64_t d,
                             int d_tile_qk, int d_tile_v, double softmax_scale,
                             int dtype, void* stream);

/* kv_tiles_per_block value that lets the library choose the split from the device's
 * occupancy: no split when the query tiles alone number at least the device's compute units,
 * otherwise ceil(CUs / query tiles) splits (about one workgroup per CU) -- and, for d = 128
 * with 16-bit inputs, ceil(2 * CUs / query tiles) splits (two workgroups per CU) whenever
 * every split then still keeps at least 4096 keys (e.g. B1 H1 L16384: 128 query tiles on 256
 * CUs -> 4 splits, not 2).  The reference's README presets (flash_attention_v2/README.md:29-32)
 * made automatic. */
#define FA_KV_TILES_AUTO (-1)

/* blocks_per_workgroup value that lets the library group the key blocks of a query tile onto
 * workgroups itself (fa_fwd_v2_split_plan). */
#define FA_BLOCKS_PER_WG_AUTO 0

/* Bytes of device workspace fa_fwd_v2 needs for this problem.  A split (the reference's key
 * block) is kv_tiles_per_block * bk keys (bk from fa_kernel_geometry).  partial_dtype is
 * FA_DTYPE_FP32, the input dtype or FA_DTYPE_FP16_SCALED.  *num_splits (may be NULL)
 * receives the number of key blocks.  The size covers the partials fa_fwd_v2 actually moves
 * through the workspace (fa_fwd_v2_split_plan); it depends on the device's occupancy.
 * FA_ERR_UNSUPPORTED when the grid of (query tile, partial, b*h) workgroups exceeds 2^31 - 1
 * or a query tile would have more than 65535 partials (the in-kernel combine counts arrivals
 * and completions in 16-bit halves of one counter): raise kv_tiles_per_block. */
int fa_fwd_v2_workspace_size(int64_t B, int64_t H, int64_t L, int64_t d,
                             int kv_tiles_per_block, int dtype, int partial_dtype,
                             size_t* bytes, int* num_splits);
/* fa_fwd_v2_workspace_size for fa_fwd_v2_ex's blocks_per_workgroup (FA_BLOCKS_PER_WG_AUTO:
 * the library's grouping, as fa_fwd_v2_workspace_size). */
int fa_fwd_v2_workspace_size_ex(int64_t B, int64_t H, int64_t L, int64_t d,
                                int kv_tiles_per_block, int blocks_per_workgroup,
                                int dtype, int partial_dtype, size_t* bytes, int* num_splits);

/* How fa_fwd_v2 schedules the key blocks of a query tile: *key_blocks = ceil(L / (kv_tiles_per_block
 * * bk)) (the reference's partials), *blocks_per_wg_out consecutive blocks per workgroup
 * (combined on chip: the online softmax carried across them), *partials_per_tile partial
 * workgroups per query tile (combined through the workspace).  With blocks_per_workgroup =
 * FA_BLOCKS_PER_WG_AUTO the library cuts the blocks of a query tile into equal groups: none beyond
 * one when the query tiles alone number at least the device's compute units, otherwise
 * ceil(CUs / query tiles) groups (about one workgroup per CU) -- for d = 128 with 16-bit inputs
 * ceil(2 * CUs / query tiles) groups (two per CU) when each group then keeps >= 4096 keys
 * (B1 H1 L16384 on 256 CUs: 4 partials per tile); d = 384 / 512: always one group;
 * a positive value fixes the group size (1: one key block per group, the reference's layout;
 * clamped to the number of blocks).  *partials_per_tile counts the groups, i.e. the partials
 * of a tile; how they are scheduled: one workgroup per group (the one-shot grid), except at
 * d = 128 with 16-bit inputs and scaled-fp16 partials when the query tiles alone fill a grid
 * of two workgroups per CU (B*H*ceil(L/128) >= 2 * CUs), groups of a multiple of 128 keys (at
 * least 256) and L a multiple of 128 -- then a persistent grid of 2 workgroups per CU WALKS each query tile's
 * groups one after another on one workgroup (the "walk", fa_last_kernels:
 * "fa_fwd16_chain_kernel<fused walk>"), stores the first partials_per_tile - 1 partials and
 * combines them with the last one, still in its registers.  The plan depends only on the
 * arguments and the current device's compute-unit count.  Any output pointer may be NULL. */
int fa_fwd_v2_split_plan(int64_t B, int64_t H, int64_t L, int64_t d, int kv_tiles_per_block,
                         int blocks_per_workgroup, int dtype, int* key_blocks,
                         int* blocks_per_wg_out, int* partials_per_tile);

/* FA-v2 split-KV forward: per (q-tile, group of key blocks, b*h) the keys' normalised partial
 * O and log-sum-exp go into the workspace, and the tile's partials are combined with
 * fa_combine's formula inside the same launch (the reduction kernel's maths without its
 * separate pass over HBM) -- either by the last of the tile's workgroups to finish (one-shot
 * grid: one workgroup per group, an arrival counter per tile), or by the workgroup that walks
 * all of the tile's groups in turn (the persistent walk, see fa_fwd_v2_split_plan: no
 * counters, partials_per_tile - 1 partials through HBM).  One partial per q-tile
 * (fa_fwd_v2_split_plan): the plain FA-v1 kernel.  workspace: device buffer of at least fa_fwd_v2_workspace_size bytes,
 * 256-byte aligned, contents need not be initialised (a hipMemsetAsync of its counters
 * precedes the launch on `stream`).  d_tile_qk / d_tile_v as for fa_fwd_v1_tiled_d. */
int fa_fwd_v2(const void* q, const void* k, const void* v, void* o,
              int64_t B, int64_t H, int64_t L, int64_t d,
              int d_tile_qk, int d_tile_v, int kv_tiles_per_block,
              void* workspace, size_t workspace_bytes,
              int dtype, int partial_dtype, void* stream);

/* fa_fwd_v2 with an explicit softmax scale (as fa_fwd_v1_scaled). */
int fa_fwd_v2_scaled(const void* q, const void* k, const void* v, void* o,
                     int64_t B, int64_t H, int64_t L, int64_t d,
                     int d_tile_qk, int d_tile_v, int kv_tiles_per_block,
                     void* workspace, size_t workspace_bytes, double softmax_scale,
                     int dtype, int partial_dtype, void* stream);
/* fa_fwd_v2_scaled on strided q, k, v, o (strides as for fa_fwd_v1_ex), with an explicit key-block
 * grouping (blocks_per_workgroup as for fa_fwd_v2_split_plan; FA_BLOCKS_PER_WG_AUTO = the
 * library's); the workspace is sized by fa_fwd_v2_workspace_size_ex with the same value. */
int fa_fwd_v2_ex(const void* q, const void* k, const void* v, void* o,
                 int64_t B, int64_t H, int64_t L, int64_t d,
                 int d_tile_qk, int d_tile_v, int kv_tiles_per_block, int blocks_per_workgroup,
                 void* workspace, size_t workspace_bytes,
                 const int64_t* q_strides, const int64_t* kv_strides, const int64_t* o_strides,
                 double softmax_scale, int dtype, int partial_dtype, void* stream);
/* fa_fwd_v2_ex with flags (0, or FA_V2_COUNTERS_ZERO).  FA_V2_COUNTERS_ZERO: the caller
 * guarantees that the workspace's completion counters are zero -- it zeroed the whole
 * workspace once (hipMemset) and only fa_fwd_v2* calls with the same B, H, L, d,
 * kv_tiles_per_block, blocks_per_workgroup, dtype and partial_dtype (the same counter words)
 * have used it since, every one of which leaves its counters zero -- so the per-call counter
 * reset, a dispatch of its own on `stream`, is skipped.  A workspace with non-zero counters under this
 * flag gives wrong outputs or, for key blocks of >= 4096 keys, a kernel that never finishes:
 * pass 0 when in doubt.  The reference reallocates its workspace on every call
 * (flash_attention_v2/CUDA/flash_attention_v2.h:461-508). */
#define FA_V2_COUNTERS_ZERO 1u
int fa_fwd_v2_ex2(const void* q, const void* k, const void* v, void* o,
                  int64_t B, int64_t H, int64_t L, int64_t d,
                  int d_tile_qk, int d_tile_v, int kv_tiles_per_block, int blocks_per_workgroup,
                  void* workspace, size_t workspace_bytes,
                  const int64_t* q_strides, const int64_t* kv_strides, const int64_t* o_strides,
                  double softmax_scale, int dtype, int partial_dtype, unsigned flags, void* stream);
/* Split-KV partial forward over ONE key range (a whole KV shard, e.g. one GPU's
 * slice of the sequence).  q: [B, H, Lq, d]; k, v: [B, H, Lk, d].
 * Writes, for every query row, the normalised partial output and its log-sum-exp
 * (base 2, of the scaled scores: lse = log2(sum_j 2^(s_j * log2(e)/sqrt(d)))):
 *   o_part[(row / chunk_rows)][b*H + h][row % chunk_rows][:]   (partial_dtype)
 *   lse   [(row / chunk_rows)][b*H + h][row % chunk_rows]      (fp32; fp64 for FP64)
 * chunk_rows must divide Lq.  chunk_rows = Lq gives a plain [B,H,Lq,d] layout;
 * chunk_rows = Lq / world gives the all-to-all send layout of the multi-GPU path.
 * partial_dtype FA_DTYPE_FP16_SCALED: o_part holds O_row * 2^-e_row in fp16 and lse holds
 * two floats per row, {lse, e} (lse [...][row % chunk_rows][2]); fa_combine undoes the scale. */
int fa_fwd_partial(const void* q, const void* k, const void* v,
                   void* o_part, void* lse,
                   int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t d,
                   int64_t chunk_rows, int dtype, int partial_dtype, void* stream);

/* fa_fwd_partial with a strided q: q_strides = {batch, head, row} element strides of the
 * [B, H, Lq, d] query view (NULL = contiguous), e.g. rows [c*Lq, (c+1)*Lq) of a longer
 * [B, H, L, d] tensor -- the multi-GPU path computes one destination rank's chunk of the
 * partials per launch this way, so the exchange of one chunk overlaps the next one's
 * compute.  k, v contiguous; bf16 / fp16 only when strided. */
int fa_fwd_partial_ex(const void* q, const void* k, const void* v,
                      void* o_part, void* lse,
                      int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t d,
                      int64_t chunk_rows, const int64_t* q_strides,
                      int dtype, int partial_dtype, void* stream);
/* Combine num_splits partials: o_part [num_splits][B*H][L][d] (partial_dtype),
 * lse [num_splits][B*H][L] (fp32, base 2; fp64 for FA_DTYPE_FP64; [num_splits][B*H][L][2]
 * {lse, e} for FA_DTYPE_FP16_SCALED) -> o [B, H, L, d] (dtype), using
 * O = sum_s 2^(lse_s - M) O_s / sum_s 2^(lse_s - M), M = max_s lse_s
 * (the reference's formula, flash_attention_v2/numpy_gpu_like.py:269-288, on
 * normalised partials). */
int fa_combine(const void* o_part, const void* lse, void* o,
               int64_t num_splits, int64_t B, int64_t H, int64_t L, int64_t d,
               int dtype, int partial_dtype, void* stream);

/* ---- KV-cache decode: few query rows per sequence against a long, possibly padded cache ----
 *
 * q and o are [B, H, Lq, d] contiguous, k and v [B, H_kv, Lk, d] with H a multiple of H_kv
 * (G = H / H_kv; query head h reads K/V head h / G), FA_DTYPE_BF16 or FA_DTYPE_FP16, d = 64 or
 * 128, and G * Lq <= 64: the G * Lq query rows of a K/V head are one work item's query tile, so
 * each K/V row is read once per group.  The keys are cut into `splits` ranges of
 * `keys_per_split` keys that run as separate workgroups (grid B * H_kv * splits) and are
 * combined by a second small kernel of the same call.
 *
 * fa_fwd_decode_plan: the split the launcher will use.  num_splits 0 = auto: as few splits as
 * still give every compute unit a workgroup, 1 when B * H_kv alone does, never fewer than 256
 * keys per split; a positive num_splits is clamped to ceil(Lk / 64).  keys_per_split is a
 * multiple of 64, splits * keys_per_split >= Lk > (splits - 1) * keys_per_split.  cus: the
 * compute units to plan for, 0 = the current device's (fa_fwd_decode plans for the device that
 * owns `stream`).  *workspace_bytes: the fp32 partials [B*H_kv*splits][G*Lq][d] and their base-2
 * lse [B*H_kv*splits][G*Lq], each rounded up to 256 bytes; 0 for one split.  Any output pointer
 * may be NULL.  No device is needed when cus > 0.
 *
 * fa_fwd_decode: O[b, h, i] = softmax(softmax_scale * Q[b, h, i] K[b, h/G, 0..n)^T) V[b, h/G, 0..n).
 *   seqlens_k: int32 [B] in DEVICE memory or NULL; the kernel reads len_b = seqlens_k[b] clamped
 *     to [0, Lk] itself (no host read, no synchronisation); NULL: len_b = Lk.  Keys >= len_b do
 *     not exist: whatever the cache holds there (NaN included) is never read into the result.
 *   flags: 0 or FA_FWD_CAUSAL, the mask aligned bottom-right: row position i sees keys
 *     j <= len_b - Lq + i (a no-op at Lq = 1).  A row without a visible key (len_b = 0, or
 *     len_b - Lq + i < 0) is zero.  A key a causal row may not see contributes nothing to that
 *     row, whatever K and V hold there.
 *   kv_strides: {batch, head, row} element strides shared by k and v (d contiguous), NULL for
 *     contiguous -- e.g. a [B, Lmax, H_kv, d] cache is {Lmax*H_kv*d, d, H_kv*d}; positive
 *     multiples of 8, row stride >= d and <= 2^20.  The cache is read in place.
 *   workspace: at least *workspace_bytes of fa_fwd_decode_plan (same arguments, cus = 0 with the
 *     stream's device current), 16-byte aligned; contents need not be initialised and nothing
 *     has to be reset between calls; may be NULL when the plan needs none.
 * FA_ERR_INVALID_ARG: null or misaligned pointers, non-positive sizes, a bad H_kv, a bad scale,
 * unknown flag bits, negative num_splits, a workspace that is missing or too small.
 * FA_ERR_UNSUPPORTED: d not 64 / 128, G * Lq > 64, FA_DTYPE_FP64.  For a fixed plan repeated
 * calls are bitwise equal (the splits are summed in split order).
 * fa_last_kernels: "fa_decode_kernel<16|32|64 rows> [grid B*H_kv*splits]", then
 * " + fa_decode_combine_kernel [grid ...]" when splits > 1. */
int fa_fwd_decode_plan(int64_t B, int64_t H, int64_t H_kv, int64_t Lq, int64_t Lk, int64_t d,
                       int num_splits, int cus, int dtype,
                       int* splits, int* keys_per_split, size_t* workspace_bytes);
int fa_fwd_decode(const void* q, const void* k, const void* v, void* o, const int32_t* seqlens_k,
                  int64_t B, int64_t H, int64_t H_kv, int64_t Lq, int64_t Lk, int64_t d,
                  const int64_t* kv_strides, double softmax_scale, unsigned flags, int num_splits,
                  void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ---- Paged KV-cache decode: fa_fwd_decode on a cache kept in fixed-size pages of a shared pool ----
 *
 * fa_fwd_decode_paged computes exactly what fa_fwd_decode computes on the cache obtained by
 * gathering each sequence's pages in table order, and reads the pool in place.  Key j of batch b,
 * K/V head hkv lives at (elements, d contiguous; the same rule for k_cache and v_cache)
 *     blk  = block_table[b * table_stride + j / page_size]
 *     addr = cache + blk * stride_block + hkv * stride_head + (j % page_size) * stride_row
 * q, o, seqlens_k, flags, softmax_scale, num_splits, the workspace, the split plan, the combine
 * kernel and the bitwise repeatability are fa_fwd_decode's, unchanged.
 *   Lk: the caller's upper bound on the lengths (max_seqlen_k), len_b = seqlens_k[b] clamped to
 *     [0, Lk]; it need not be a multiple of page_size.  The plan and the workspace are those of
 *     fa_fwd_decode_plan(B, H, H_kv, Lq, Lk, d, ...): a table wider than ceil(Lk / page_size)
 *     does not add splits.
 *   block_table: int32 in DEVICE memory, row b at block_table + b * table_stride, table_stride >=
 *     ceil(Lk / page_size).  The kernel reads it itself (no host read, no synchronisation).
 *   page_size: keys per page, a positive multiple of 64 (128, 192, 256, ...: any multiple), so
 *     that every 64-key tile of the kernel lies inside one page.  Pages of 16 or 32 keys are not
 *     supported.
 *   num_blocks: blocks of the pool.  Every table entry the kernel uses is clamped to
 *     [0, num_blocks - 1] before it enters an address: a corrupt entry gives a wrong result for
 *     that sequence, never an access outside the pool.
 *   cache_strides: {block, head, row} element strides shared by k_cache and v_cache, NULL for a
 *     contiguous [num_blocks, page_size, H_kv, d] pool ({page_size*H_kv*d, d, H_kv*d}); a
 *     [num_blocks, H_kv, page_size, d] pool is {H_kv*page_size*d, page_size*d, d}.  Positive
 *     multiples of 8, row stride >= d and <= 2^20.
 * What is read: of the table, only the entries of pages that hold a key below len_b (entries
 * past that may be -1 or anything else); of the pool, only rows of keys below len_b in the blocks
 * those entries name -- unused blocks, the rest of a last page and pages beyond len_b may hold
 * anything (NaN included).  Keys behind the causal mask contribute nothing, as in fa_fwd_decode.
 * FA_ERR_INVALID_ARG: fa_fwd_decode's, a NULL or misaligned block_table, num_blocks <= 0,
 * page_size <= 0, table_stride < ceil(Lk / page_size), bad strides.  FA_ERR_UNSUPPORTED:
 * fa_fwd_decode's, page_size not a multiple of 64, a row stride above 2^20.
 * fa_last_kernels: "fa_decode_kernel<16|32|64 rows, paged> [grid B*H_kv*splits]", then the
 * combine kernel as above. */
int fa_fwd_decode_paged(const void* q, const void* k_cache, const void* v_cache, void* o,
                        const int32_t* block_table, const int32_t* seqlens_k,
                        int64_t B, int64_t H, int64_t H_kv, int64_t Lq, int64_t Lk, int64_t d,
                        int64_t num_blocks, int64_t page_size, int64_t table_stride,
                        const int64_t* cache_strides, double softmax_scale, unsigned flags, int num_splits,
                        void* workspace, size_t workspace_bytes, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_H */
