/* fluent_mi355.h — C-ABI of libfluent_mi355.so (MI355X / gfx950 native hot path for
 * SGLang-FluentLLM: FP8 MLA decode + FP8 block-scaled grouped GEMM).
 *
 * Every entry point below is what the reference's Python operator API for this path binds to
 * (citations are /root/reference/python/sglang/... file:line of the call site replaced).
 * Conventions: plain pointers to DEVICE memory unless the name says host; sizes in elements;
 * `stream` is a hipStream_t passed as void*; return 0 = ok, non-zero = error (message via
 * fl_last_error()).  Compute entry points neither synchronise the host nor allocate device memory: they
 * are hipGraph-capturable (srt/model_executor/cuda_graph_runner.py:433).  Exceptions, all named: the
 * one-shot communicator's setup / teardown / fl_comm_check (fl_comm_create .. fl_comm_destroy allocate,
 * map and synchronise — called outside the captured region), and the ONE piece of process-global
 * state, fl_gemm_set_num_cus (deep_gemm.set_num_sms is process-global in the reference as well);
 * besides that only a thread-local error string and a cached CU count are kept.
 */
#ifndef FLUENT_MI355_H
#define FLUENT_MI355_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* fl_stream_t;

#define FL_OK 0
#define FL_ERR_INVALID 1
#define FL_ERR_LAUNCH 2
#define FL_ERR_UNSUPPORTED 3

#define FL_MLA_PAGE 64        /* srt/layers/attention/flashmla_backend.py:25 PAGE_SIZE */
#define FL_MLA_META_W 8       /* ints per tile-scheduler row */
#define FL_MLA_ROWS_PER_WG 64 /* query rows (s_q*H) one workgroup owns */

/* KV-cache formats (srt/mem_cache/memory_pool.py:635-658) */
#define FL_KV_FP8_PER_TOKEN 0 /* (u8[.,512], f32[.,1], bf16[.,64]) tuple, quant_method="per_token_head" */
#define FL_KV_FP8_576 1       /* one fp8 [.,576] tensor, descale scalars */
#define FL_KV_BF16_576 2      /* one bf16 [.,576] tensor */

/* ABI version of THIS header.  A binding checks fl_version() == FL_ABI_VERSION once after loading the library: that check covers EVERY
 * argument struct below.  FlMlaDecodeArgs — the one struct that has grown so far — additionally carries its own size (`struct_bytes`, first
 * field): a caller compiled against another layout of it is refused with FL_ERR_INVALID instead of being read past its end.  The other
 * argument structs (FlGroupedGemmArgs, FlRopeArgs, FlMlaAbsorbArgs ...) have no size field and are read as this header lays them out.
 * 101: FlMlaDecodeArgs gained struct_bytes (FIRST field: every later field moved — a C caller built against 100 must be recompiled) and
 *      block_table_cols (last); fl_topk_gate added.
 * 102: additive — fl_fused_add_rmsnorm_offset (GemmaRMSNorm: the 1 added in fp32), fl_mla_set_merge_timeout (+ the in-kernel split merge
 *      reports a timeout through the next fl_mla_decode call); no struct changed.
 *      (still 102, additive: fl_mha_prefill_ragged_bf16 with its own FlPrefillArgs — struct_bytes first, checked — and fl_merge_state;
 *      fl_mla_prefill_paged_bf16 with its own FlMlaPrefillArgs, struct_bytes first, checked;
 *      fl_sampling_softmax / fl_sampling_renorm / fl_sampling_sample with FlSamplingArgs, struct_bytes first, checked;
 *      fl_spec_verify_greedy / fl_spec_verify_sample with FlSpecVerifyArgs, struct_bytes first, checked;
 *      fl_gqa_paged_attention_bf16 with FlGqaPagedArgs, struct_bytes first, checked;
 *      fl_gqa_paged_attention_fp8kv over the UNCHANGED FlGqaPagedArgs, the two scales as plain arguments.) */
#define FL_ABI_VERSION 102
const char* fl_last_error(void);
int fl_version(void);
/* number of compute units of HIP device `device` (host query, cached) */
int fl_device_cu_count(int device, int* cu_count);

/* ---- K3: get_mla_metadata (flashmla_backend.py:261-265,276-280,307-321,335-339,380-384) ----
 * num_parts rows of FL_MLA_META_W int32 + num_splits[bs+1]; shapes static in bs. */
int fl_mla_num_parts(int cu_count, int rows_per_kv_head);
int fl_mla_get_metadata(const int32_t* cache_seqlens, int bs, int num_parts,
                        int32_t* tile_scheduler_metadata, int32_t* num_splits, fl_stream_t stream);

/* ---- K4: quantize_ckv_per_token_head (flashmla_backend.py:125,206) ----
 * q bf16 [rows, d_nope+d_rope] -> q_nope fp8 [rows,d_nope], q_scale f32 [rows], q_rope bf16 [rows,d_rope] */
int fl_mla_quant_q(const void* q, int64_t rows, int d_nope, int d_rope, void* q_nope, float* q_scale,
                   void* q_rope, fl_stream_t stream);

/* ---- K5: quantize_and_cache_k (srt/mem_cache/memory_pool.py:864-871,902-909; fallback :873-880) ----
 * key bf16 [n, d_nope+d_rope]; scatter into the three caches at slot indices[i]. */
int fl_mla_quant_store_k(const void* key, int64_t n, int d_nope, int d_rope, const int32_t* indices,
                         void* k_lora_cache, float* k_scale_cache, void* k_rope_cache, int64_t num_slots,
                         fl_stream_t stream);

/* K5 + K4 in one launch: fl_mla_quant_store_k (rows of `key`, scattered at `indices`) and fl_mla_quant_q (rows of `q`, dense
 * outputs) with the bytes of the two separate calls.  The reference issues them back to back in
 * FlashMLABackend.forward_decode (flashmla_backend.py:188-206: set_kv_buffer -> memory_pool.py:864-871, then
 * quantize_ckv_per_token_head); an integrator who wants one launch fewer per layer calls
 * flash_mla_fp8.quantize_q_and_cache_k.  Either row count may be 0. */
int fl_mla_quant_q_store_k(const void* key, int64_t n_k, const int32_t* indices, void* k_lora_cache, float* k_scale_cache,
                           void* k_rope_cache, int64_t num_slots, const void* q, int64_t q_rows, int d_nope, int d_rope,
                           void* q_nope, float* q_scale, void* q_rope, fl_stream_t stream);

/* ---- A2: the query side of the decode layer before the attention kernel, in ONE launch (an extension, like the entry point
 * above: INTEGRATION.md section 4) — torch.bmm(q_nope.transpose(0,1), w_kc) (srt/models/deepseek_v2.py:840), the rotary embedding of
 * q_pe and k_pe (:842-858), set_kv_buffer / K5 (flashmla_backend.py:188-196) and quantize_ckv_per_token_head / K4 (:198-206).
 * Outputs are K4's and K5's, bit-identical to the four-launch chain; the bf16 absorbed query is never written.
 * q [T, H, 192] bf16 (nope 128 | rope 64; element strides), w_kc [H, 512, 128] bf16 k-contiguous (head stride in elements),
 * cos_sin_cache [max_position, 64] f32 (cos 32 | sin 32), latent [T, 576] bf16 (k_nope | k_pe: k_pe is rotated IN PLACE; NULL = no
 * K rows), cache_loc i32 [T] (rows outside [0, num_slots) are skipped), outputs contiguous [T, H, 512] e4m3 / [T, H] f32 /
 * [T, H, 64] bf16. ---- */
typedef struct FlMlaAbsorbArgs {
  const void* q;
  int64_t q_stride_token, q_stride_head;
  int64_t num_tokens;
  int32_t num_heads;
  int32_t d_nope, d_rope, d_lora;   /* 128, 64, 512 */
  const void* w_kc;
  int64_t w_stride_head;
  const int64_t* positions;
  const float* cos_sin_cache;
  int64_t max_position;
  int32_t is_neox;
  void* latent;
  int64_t latent_stride;
  const int32_t* cache_loc;
  void* k_lora_cache;
  float* k_scale_cache;
  void* k_rope_cache;
  int64_t num_slots;
  void* q_nope_out;
  float* q_scale_out;
  void* q_rope_out;
} FlMlaAbsorbArgs;
int fl_mla_absorb_rope_quant(const FlMlaAbsorbArgs* args, fl_stream_t stream);

/* ---- K6: dequantize_ckv_fused_indexed (memory_pool.py:821-824; fallback :826-831) ---- */
int fl_mla_dequant_gather(const void* k_lora_cache, const void* k_rope_cache, const float* k_scale_cache,
                          const int32_t* indices, int64_t n, int d_nope, int d_rope, int64_t num_slots,
                          void* k_lora_out, void* k_rope_out, fl_stream_t stream);

/* ---- K1/K2: flash_mla_ckv_fp8_per_token / flash_mla_with_kvcache
 * (flashmla_backend.py:208-222,127-142 / :227-254,145-175) ---- */
typedef struct FlMlaDecodeArgs {
  int32_t struct_bytes;     /* = sizeof(FlMlaDecodeArgs) as the CALLER compiled it; anything else is refused */
  int32_t kv_format;        /* FL_KV_* */
  int32_t bs, s_q, h_q;     /* q rows per request = s_q*h_q (one latent KV head) */
  int32_t d_nope, d_rope;   /* 512, 64 */
  int32_t causal;           /* query j sees keys [0, seqlen-(s_q-1-j)) when causal */
  int32_t num_parts;        /* rows of tile_scheduler_metadata */
  float softmax_scale;
  const float* descale_q;   /* FL_KV_FP8_576 only: DEVICE scalars (flashmla_backend.py:237-238), NULL = 1.0 */
  const float* descale_k;
  /* query */
  const void* q_nope;       /* fp8 [bs,s_q,h_q,d_nope] (per-token) | fp8/bf16 [bs,s_q,h_q,576] */
  const void* q_rope;       /* bf16 [bs,s_q,h_q,d_rope] (per-token only) */
  const float* q_scale;     /* f32 [bs,s_q,h_q] (per-token only) */
  /* paged cache */
  const void* k_nope;       /* u8 [pages,64,d_nope] | [pages,64,576] */
  const void* k_rope;       /* bf16 [pages,64,d_rope] (per-token only) */
  const float* k_scale;     /* f32 [pages,64] (per-token only) */
  int64_t num_pages;
  const int32_t* block_table; /* i32 [bs, block_table_stride] page ids (bit-exact, allocator.py:60-102) */
  int64_t block_table_stride;
  const int32_t* cache_seqlens; /* i32 [bs] */
  int32_t* tile_scheduler_metadata; /* from fl_mla_get_metadata.  NOT const: columns 5..7 of every row are scratch counters of
                                      * the in-kernel split merge — zero on entry, WRITTEN by fl_mla_decode, zero again when
                                      * the launch has finished.  Ordering rule: launches that share one metadata tensor must
                                      * be ordered on ONE stream (or by events); two concurrent launches on the same tensor
                                      * would mix their arrival counts.  Give concurrent streams their own copy. */
  const int32_t* num_splits;
  /* outputs */
  void* out;                /* bf16 [bs,s_q,h_q,d_nope] */
  float* lse;               /* f32 [bs,h_q,s_q] natural-log LSE */
  float* o_accum;           /* split-KV workspace of (bs+num_parts)*s_q*h_q*d_nope*4 bytes (caller-owned, opaque:
                               f32 rows, or bf16 rows for the 128-row mapping; only fl_mla_decode reads it) */
  float* lse_accum;         /* f32 [bs+num_parts, s_q*h_q, 2] {weight LSE, exact LSE} workspace */
  const void* q_bf16;       /* optional (FL_KV_FP8_PER_TOKEN, s_q*h_q > 32): the UNQUANTISED query bf16 [bs,s_q,h_q,576]; the decode
                             * kernel then does quantize_ckv_per_token_head (K4, flashmla_backend.py:198-206) in its own prologue — same
                             * bytes, same result, one launch and a write + re-read of Q less; q_nope / q_rope / q_scale are ignored */
  int64_t block_table_cols; /* columns of a block_table row that may be read (block_table.shape[1]); 0 = block_table_stride.  The row
                             * stride is NOT the row width for an expanded (stride 0) or sliced table: the kernels clamp their
                             * unconditional page-id loads against THIS */
} FlMlaDecodeArgs;

int fl_mla_decode(const FlMlaDecodeArgs* args, fl_stream_t stream);
/* Budget of the in-kernel split merge's wait for a request's other pieces (default 2 s; env FLUENT_MLA_MERGE_TIMEOUT_S).  A merger that gives up
 * writes NaN into the request's rows and LSEs AND reports through a host-mapped word: the NEXT fl_mla_decode call returns FL_ERR_LAUNCH
 * (fl_last_error names the workgroup).  Synchronises the device (hipMemcpyToSymbol): call it outside captures. */
int fl_mla_set_merge_timeout(double seconds);
/* Sizes of the two workspaces above for a launch of this shape (the partial rows are bf16 or f32 depending on the
 * mapping the shape dispatches to; allocate exactly this much, e.g. from the graph's memory pool). */
int fl_mla_workspace_bytes(int kv_format, int bs, int s_q, int h_q, int num_parts, int64_t* o_accum_bytes,
                           int64_t* lse_accum_bytes);

/* ---- G1-G4: deep_gemm.m_grouped_gemm_fp8_fp8_bf16_nt_{offset,contiguous,masked} / gemm_fp8_fp8_bf16_nt
 * (srt/layers/moe/gemms/fp8/fire.py:18 -> moe/executors/fp8_eps_executor.py:56,78;
 *  moe/executors/deep_ep_executor.py:583-586,607-613,655-662,681-688; dense/gemms/fp8/deep_geem.py:55) ---- */
#define FL_GEMM_OFFSET 0      /* rows [meta[e], meta[e+1]) use group e; meta = exclusive_sum i32 [E+1] */
#define FL_GEMM_CONTIGUOUS 1  /* row i uses group meta[i] (<0 = skip), groups 128-row aligned; meta = m_indices i32 [M] */
#define FL_GEMM_MASKED 2      /* A [G, rows_per_group, K], first meta[g] rows of group g valid; meta = masked_m i32 [G] */
#define FL_GEMM_DENSE 3       /* one group, meta unused */
typedef struct FlGemmArgs {
  int32_t mode;
  int32_t num_groups;         /* E (1 for dense) */
  int64_t M;                  /* total rows of A/out (masked: G*rows_per_group) */
  int32_t N, K;               /* W is [E, N, K] fp8, K % 128 == 0 */
  int64_t rows_per_group;     /* masked only */
  int64_t expected_m;         /* hint for the token-tile height (0 = derive) */
  const void* A;              /* fp8 [M, K] row-major */
  const float* As;            /* f32 scales of A, element (m, kb) at m*as_stride_m + kb*as_stride_k */
  int64_t as_stride_m, as_stride_k;
  int64_t as_stride_g;        /* masked only: stride between groups of As */
  const void* W;              /* fp8 [E, N, K] */
  const float* Ws;            /* f32 [E, ceil(N/128), K/128] */
  void* out;                  /* bf16 [M, N] */
  const int32_t* group_meta;
  void* workspace;            /* optional scratch (f32 partials) for split-K of problems with few tiles — the dense decode GEMMs of
                               * the MLA projections: [T<=256, K] x [N, K] has N/128 tiles for 256 CUs; NULL = never split */
  int64_t workspace_bytes;
} FlGemmArgs;
int fl_grouped_gemm_fp8(const FlGemmArgs* args, fl_stream_t stream);
int fl_gemm_set_num_cus(int n);   /* deep_gemm.set_num_sms (srt/tbo/tbo_executor.py:129-134) */
int fl_gemm_get_num_cus(void);

/* ---- G5: bf16 grouped GEMM of the unquantised MoE experts — eps.executor.AokGroupedGemm.run
 * (srt/layers/moe/gemms/bf16/aok.py:3,18 -> moe/executors/eps_executor.py:35,48: w13, then silu, then w2 on the rows
 * AllToAll.dispatch grouped by expert).  out[r, n] = sum_k A[r, k] * W[e, n, k] for r in [meta[e], meta[e+1]): bf16 operands
 * contiguous in k, fp32 accumulation, ONE rounding (RNE) to bf16.  Rows of `out` outside [meta[0], meta[E]) are never written;
 * meta[0] may be non-zero; group bounds are clamped into [0, M].  FL_GEMM_DENSE: one group of all M rows, meta unused.
 * K % 64 == 0, K >= 64, N % 64 == 0 — anything else is FL_ERR_UNSUPPORTED.  A, W rows 16-byte aligned, out 8-byte aligned.
 * One launch, no host synchronisation, no allocation, hipGraph-capturable; fl_gemm_set_num_cus caps its grid as well. ---- */
typedef struct FlGemmBf16Args {
  int32_t struct_bytes;       /* = sizeof(FlGemmBf16Args) as the CALLER compiled it; anything else is refused */
  int32_t mode;               /* FL_GEMM_OFFSET or FL_GEMM_DENSE */
  int32_t num_groups;         /* E (1 for dense) */
  int32_t N, K;               /* W is [E, N, K] bf16 */
  int32_t tile_rows;          /* token rows per workgroup: 32 (decode: the weight stream bounds it), 128, or 0 = choose
                               * from M / num_groups (host integers only: a captured call site sees one fixed kernel) */
  int64_t M;                  /* rows of A / out */
  const void* A;              /* bf16 [M, K] */
  const void* W;              /* bf16 [E, N, K] */
  void* out;                  /* bf16 [M, N] */
  const int32_t* group_meta;  /* offset mode: exclusive_sum i32 [E + 1], DEVICE */
} FlGemmBf16Args;
int fl_grouped_gemm_bf16(const FlGemmBf16Args* args, fl_stream_t stream);

/* ---- G6: W8A8 dense GEMM, scales applied once after the product — flashinfer.fp8_scaled_mm
 * (srt/layers/dense/gemms/fp8/fp8_utils.py:434,605 apply_fp8_linear; layouts/w8a8_fp8.py) and flashinfer.int8_scaled_mm
 * (layouts/w8a8_int8.py:203-216; compressed_tensors_w8a8_int8.py:167-169):
 *     out[m, n] = out_type( f32( sum_k A[m, k] * B[n, k] ) * sa[m] * sb[n] + bias[n] )
 * A [M, K] and B [N, K] (the weight as stored) hold one byte per element, k contiguous, rows lda / ldb bytes apart; the int8
 * accumulator is i32 (exact) and becomes f32 only in the epilogue.  sa / sb: f32, one entry per row / column (stride 1) or ONE
 * entry (stride 0).  bias: NULL or [N] in the output type.  out: bf16 / fp16, rows ldc elements apart; rows >= M and columns >= N
 * are never written.  K % 16 == 0, N % 16 == 0, lda % 16 == 0, ldb % 16 == 0, ldc % 4 == 0, A / B 16-byte and out 8-byte
 * aligned; M == 0 returns without a launch; anything else is FL_ERR_INVALID before any launch.  A k tail shorter than the MFMA's
 * k step is zero-filled in LDS (never read past the row).  One launch, no host synchronisation, no allocation,
 * hipGraph-capturable (csrc/gemm_w8a8.hip). ---- */
#define FL_W8A8_FP8_E4M3 0
#define FL_W8A8_INT8 1
#define FL_W8A8_OUT_BF16 0
#define FL_W8A8_OUT_FP16 1
typedef struct FlGemmW8A8Args {
  int32_t struct_bytes;       /* = sizeof(FlGemmW8A8Args) as the CALLER compiled it; anything else is refused */
  int32_t elem_type;          /* FL_W8A8_FP8_E4M3 (OCP e4m3fn) or FL_W8A8_INT8 */
  int32_t out_type;           /* FL_W8A8_OUT_BF16 or FL_W8A8_OUT_FP16 */
  int32_t tile_rows;          /* token rows per workgroup: 32 (decode: a weight stream, 64-column tiles), 128 (128 x 128 tiles),
                               * or 0 = choose from M (host integers only: a captured call site sees one fixed kernel) */
  int32_t N, K;
  int64_t M;
  int64_t lda, ldb;           /* bytes between rows of A / B */
  int64_t ldc;                /* elements between rows of out */
  int64_t sa_stride, sb_stride; /* 1, or 0 for a single broadcast entry */
  const void* A;
  const void* B;
  const float* sa;
  const float* sb;
  const void* bias;
  void* out;
} FlGemmW8A8Args;
int fl_gemm_w8a8(const FlGemmW8A8Args* args, fl_stream_t stream);

/* ---- Q1/Q2: 1x128 per-token-group FP8 quantisation (flashinfer.quantization.quant_1x128,
 * moe/executors/fp8_eps_executor.py:53-55,75-77; flashinfer.sgl_per_token_group_quant_fp8,
 * dense/gemms/fp8/fp8_kernel.py:457-460).  s = max(amax, eps)/448 (fp32), q = x/s -> e4m3 (RNE).
 * x bf16 [M, K]; scale (m, kb) written at m*s_stride_m + kb*s_stride_k. ---- */
int fl_quant_1x128(const void* x, int64_t M, int K, float eps, void* x_q, float* x_s, int64_t s_stride_m,
                   int64_t s_stride_k, fl_stream_t stream);

/* ---- Q3-Q5: the row / tensor quantisers of the W8A8 path.  x is contiguous bf16; one wave per row (or group), 16-byte loads;
 * every scale is computed in f32 and the quotient x / s is the IEEE one.  All capturable, no host synchronisation.
 * fl_quant_per_token_fp8 — flashinfer.sgl_per_token_quant_fp8 (dense/gemms/fp8/fp8_kernel.py:43-47; fp8_utils.py apply_fp8_linear):
 *   s[m] = max(amax_m, 1e-10) / 448, q = e4m3fn(x / s) saturating at +-448; an all-zero row gives zeros and s = 1e-10 / 448.  K % 8 == 0.
 * fl_quant_per_token_group_int8 — flashinfer.sgl_per_token_group_quant_int8 (layouts/w8a8_int8.py:203-216 per_token_quant_int8 with
 *   group_size = K; apply_w8a8_block_int8_linear with group_size = 128): s[m, g] = max(amax, eps) / 127 at x_s[m * (K / group) + g],
 *   q = clamp(round-half-away(x / s), -127, 127).  group_size % 8 == 0, K % group_size == 0.
 * fl_quant_per_tensor_fp8 — flashinfer.sgl_per_tensor_quant_fp8 (fp8_kernel.py:43-47): is_static = 0: x_s[0] = max(amax, 1e-10) / 448
 *   over ALL numel elements (a clear kernel, then a vector atomic max on the non-negative f32 bit pattern of each wave's scale —
 *   division by 448 is monotone, so the maximum of the scales is the scale of the maximum), then the quantise launch: three
 *   launches and no memset node.  is_static != 0: one launch that reads x_s[0].  numel % 8 == 0. ---- */
int fl_quant_per_token_fp8(const void* x, int64_t M, int K, void* x_q, float* x_s, fl_stream_t stream);
int fl_quant_per_token_group_int8(const void* x, int64_t M, int K, int group_size, float eps, void* x_q, float* x_s,
                                  fl_stream_t stream);
int fl_quant_per_tensor_fp8(const void* x, int64_t numel, void* x_q, float* x_s, int is_static, fl_stream_t stream);

/* ---- A1: silu(x[:, :I]) * x[:, I:] (eps.executor.silu, fp8_eps_executor.py:62; flashinfer.silu_and_mul), bf16;
 * with q_out != NULL also emits the 1x128 quantisation of the result
 * (flashinfer.activation.silu_and_mul_fuse_block_quant, deep_ep_executor.py:676, activation.py:73). ---- */
int fl_silu_and_mul(const void* x, int64_t M, int I, void* out_bf16, void* q_out, float* s_out, int64_t s_stride_m,
                    int64_t s_stride_k, fl_stream_t stream);

/* ---- C5/C6/C7: compute half of flashinfer.comm.trtllm_{allreduce,reducescatter,allgather}_fusion
 * (srt/layers/flashinfer_comm_fusion.py:286-401, 404-513, 516-640 <- layernorm.py:114-189, 305-359).  The exchange is one
 * one-shot collective over RCCL (host: torch.distributed); this is everything after it in ONE kernel:
 * v = sum_{w<num_pieces} x[w*piece_stride + (t,h)] (+ add_in) (+ residual_in)  [fp32];  residual_out = bf16(v);
 * norm_out = bf16(v * rsqrt(mean_h v^2 + eps) * gamma)  (RMSNorm.forward_native, layernorm.py:88-112);
 * quant_out/scale_out = 1x128 e4m3 quantisation of norm_out (scale (t,g) at t*s_stride_t + g*s_stride_g).
 * All tensors bf16 [T, H] (gamma [H]); any output may be NULL; with norm_out == quant_out == NULL it is the plain
 * one-shot reduction (gamma may be NULL): eps.communication.TPDPConvertor.reduce_scatter (C3,
 * srt/distributed/decoder_comm_manager.py:42-85, layers/dp_attention.py:62-74). ---- */
int fl_fused_add_rmsnorm(const void* x, int num_pieces, int64_t piece_stride /*elements*/, const void* add_in,
                         const void* residual_in, const void* gamma, float eps, int64_t T, int H, void* residual_out,
                         void* norm_out, void* quant_out, float* scale_out, int64_t s_stride_t, int64_t s_stride_g,
                         fl_stream_t stream);
/* The same with norm_out = bf16(v * rsqrt(..) * (gamma + gamma_offset)), the offset added in fp32: GemmaRMSNorm (layernorm.py:209-233,
 * gamma_offset = 1).  x / residual_in may alias norm_out / residual_out (flashinfer's in-place fused_add_rmsnorm). */
int fl_fused_add_rmsnorm_offset(const void* x, int num_pieces, int64_t piece_stride /*elements*/, const void* add_in,
                                const void* residual_in, const void* gamma, float gamma_offset, float eps, int64_t T, int H,
                                void* residual_out, void* norm_out, fl_stream_t stream);
/* C7 (layernorm.py:305-359 <- models/deepseek_v2.py:799-807): dual RMSNorm over gathered rows ag bf16 [T, D]:
 * cols [0, q_rank) -> x_norm_out [T, q_rank] (+ optional 1x128 fp8 quant), cols [q_rank, q_rank+kv_rank) in place. */
int fl_dual_rmsnorm(void* ag, int64_t T, int D, int q_rank, int kv_rank, const void* gamma_q, const void* gamma_kv,
                    float eps_q, float eps_kv, void* x_norm_out, void* quant_out, float* scale_out, int64_t s_stride_t,
                    int64_t s_stride_g, fl_stream_t stream);

/* ---- C5/C6 one-shot: the exchange AND the fused epilogue in one kernel over peer-mapped (hipIpc) workspaces — replaces
 * flashinfer.comm.trtllm_create_ipc_workspace_for_all_reduce_fusion + trtllm_allreduce_fusion / trtllm_reducescatter_fusion
 * (srt/layers/flashinfer_comm_fusion.py:64-109 workspace, :286-401 C5, :404-513 C6) for token counts up to the workspace's
 * max_tokens.  Every rank writes its rows into each destination's inbox over xGMI, raises per-row flags, and the
 * workgroup owning a row reduces it in rank order (bit-identical on all ranks) + residual + RMSNorm (+ 1x128 fp8 quant).
 * Protocol: csrc/comm_protocol.h.  Setup: create on every rank -> exchange the 64-byte handles (any transport) ->
 * connect.  The epoch lives in device memory: launches may be captured in a hipGraph and replayed. ---- */
int fl_comm_workspace_size(int world, int64_t max_tokens, int hidden, int64_t* bytes_out);
int fl_comm_create(int rank, int world, int64_t max_tokens /*<= 1024*/, int hidden /*<= 8192*/, void** comm_out);
int fl_comm_local_handle(void* comm, void* handle_out /*64 bytes: hipIpcMemHandle_t of this rank's workspace*/);
int fl_comm_connect(void* comm, const void* handles /*world x 64 bytes in rank order; NULL allowed at world 1*/);
int fl_comm_set_timeout(void* comm, double seconds /*budget of one flag wait; default 10 s*/);
/* C5: all ranks pass in bf16 [T, H]; every rank gets sum (+ residual_in [T, H]) -> residual_out, RMSNorm -> norm_out,
 * quant_out/scale_out optional (any may be NULL; gamma NULL = sum only into residual_out). */
int fl_allreduce_fused(void* comm, const void* in, int64_t T, int H, const void* residual_in, const void* gamma, float eps,
                       void* residual_out, void* norm_out, void* quant_out, float* scale_out, int64_t s_stride_t,
                       int64_t s_stride_g, fl_stream_t stream);
/* C6: in bf16 [T, H] on every rank; rank r gets its token slice (get_num_tokens_per_rank: the first T % world ranks own
 * one more) of the sum; add_in / residual_in / outputs are [slice rows, H]. */
int fl_reducescatter_fused(void* comm, const void* in, int64_t T, int H, const void* add_in, const void* residual_in,
                           const void* gamma, float eps, void* residual_out, void* norm_out, void* quant_out, float* scale_out,
                           int64_t s_stride_t, int64_t s_stride_g, fl_stream_t stream);
/* C7 / the all-gather half of C3 as one kernel (flashinfer.comm.trtllm_allgather_fusion, flashinfer_comm_fusion.py:613-638;
 * eps.communication.TPDPConvertor.all_gather, layers/dp_attention.py:62-74): every rank holds `t_cur` =
 * get_num_tokens_per_rank(world, T)[rank] rows `in [t_cur, D]`; out [T, D] receives all rows in rank order.  q_rank > 0: dual
 * RMSNorm of every gathered row — cols [0, q_rank) -> x_norm_out [T, q_rank] (+ optional 1x128 fp8 quant_out / scale_out),
 * cols [q_rank, q_rank + kv_rank) in place in `out`.  T <= 1024, ceil(T / world) <= max_tokens, D <= hidden. */
int fl_allgather_fused(void* comm, const void* in, int64_t t_cur, int64_t T, int D, void* out, int q_rank, int kv_rank,
                       const void* gamma_q, const void* gamma_kv, float eps_q, float eps_kv, void* x_norm_out, void* quant_out,
                       float* scale_out, int64_t s_stride_t, int64_t s_stride_g, fl_stream_t stream);
/* C1 / C2 exchange on the same transport (eps.fast_ep.AllToAll over MSCCL++: srt/layers/moe/dispatcher/fast_ep.py:45-78,
 * distributed/parallel_state.py:965-977): equal-split all-to-all of `world` slabs of `cap` rows x D 2-byte elements — slab p of `send`
 * lands as slab `rank` of rank p's `recv`.  ids_col >= 0: a row's top_k int32 expert ids start at element ids_col of the row; rows whose
 * ids are all negative (nobody routed there) travel and are copied out as their 16-byte-aligned tail only.  cap * world <= 1024,
 * cap <= max_tokens, D <= hidden of the communicator. */
int fl_alltoall_oneshot(void* comm, const void* send, void* recv, int cap, int D, int ids_col, int top_k, fl_stream_t stream);
int fl_comm_check(void* comm /*synchronises; FL_ERR_LAUNCH if a flag wait ever timed out*/);
int fl_comm_destroy(void* comm);
/* The same protocol on plain host memory (shared-memory workspaces of several processes): drives the CPU-side protocol
 * test of the flag / epoch / parity logic.  Test infrastructure — nothing on the product path calls these. */
int fl_comm_host_init(void* ws, int world, int64_t max_tokens, int hidden);
int fl_comm_host_exchange(void* const* ws /*[world] workspaces as mapped in this process*/, int rank, int world, int64_t max_tokens,
                          int hidden, int reduce_scatter, const uint16_t* in /*bf16 [T, H]*/, int64_t T, int H,
                          float* out /*f32 [rows, H]: the sums*/, double timeout_s);

/* ---- C1/C2: device side of eps.fast_ep.AllToAll.dispatch / combine (srt/layers/moe/dispatcher/fast_ep.py:45-51,
 * 73-78).  The exchange is one equal-split all-to-all per direction over RCCL (host: torch.distributed); these do the
 * integer / row work around it, sync-free with static shapes.  Rows are bf16 [*, hidden], hidden % 8 == 0. ---- */
int fl_ep_route(const int32_t* indices /*[num_pairs] global expert ids*/, int64_t num_pairs, int experts_per_rank, int world,
                int cap /*rows per peer slab*/, int32_t* send_slot /*[num_pairs] -> dest*cap+pos or -1*/,
                int32_t* send_eid /*[world*cap] local expert id at the destination, -1 = empty*/, fl_stream_t stream);
/* Token-once-per-peer routing of the same dispatch (fluent_mi355/ep.py): tok_slot [tokens, world] = the token's row in
 * each peer slab (-1: none of its experts lives there), send_eid [world*cap, top_k] = local expert ids per slab row (-1
 * padded), pair_src [world*cap, top_k] = t*top_k + k of the (token, expert) pair behind every slab pair (-1 padded): the
 * layout the combine weights travel in (fl_ep_gather_f32).
 * ROW STRIDES (round 3): the ids (and, when the caller has them at dispatch time, the routing weights) can travel in the TAIL of
 * their slab row — message row = [hidden bf16 | top_k int32 ids | top_k f32 weights] — so that a direction is ONE all-to-all
 * instead of two.  The `*_row_stride` arguments are the distance between consecutive rows of that tensor in ITS OWN element
 * type (int32 / f32 / bf16); 0 = dense ([rows, top_k] resp. [rows, hidden]). */
int fl_ep_route_dedup(const int32_t* indices /*[tokens, top_k] global expert ids*/, int64_t num_tokens, int top_k,
                      int experts_per_rank, int world, int cap, int32_t* tok_slot, int32_t* send_eid, int32_t* pair_src,
                      int64_t eid_row_stride,
                      const float* weights /*optional [tokens, top_k] f32: placed beside the ids (send_w[row, j], 0 = padding)*/,
                      float* send_w, int64_t w_row_stride, fl_stream_t stream);
int fl_ep_gather_f32(const float* vals, int64_t n, const int32_t* src /*[out_n]*/, float* out /*out[j] = vals[src[j]], 0 where src[j] is not in [0, n)*/,
                     int64_t out_n, int per_row /*entries per output row*/, int64_t out_row_stride, fl_stream_t stream);
int fl_ep_gather_rows_div(const void* src, int64_t src_rows, const int32_t* idx, int64_t n, int div /*dst[i] = src[idx[i] / div]*/,
                          int hidden, void* dst, int64_t dst_rows,
                          const int32_t* n_valid /*optional DEVICE scalar: only rows i < *n_valid are copied (the launch is sized for n)*/,
                          int64_t src_row_stride, fl_stream_t stream);
int fl_ep_sort(const int32_t* recv_eid /*[num_slots] = [rows, per_row]*/, int64_t num_slots, int num_local_experts,
               int32_t* order /*[num_slots] slots grouped by expert, invalid last*/, int32_t* exclusive_sum /*[E_l+1]*/,
               int32_t* inverse /*optional [num_slots]: inverse[order[i]] = i*/, int per_row, int64_t eid_row_stride, fl_stream_t stream);
int fl_ep_gather_rows(const void* src, int64_t src_rows, const int32_t* idx, int64_t n, int hidden, void* dst,
                      int64_t dst_rows, fl_stream_t stream);   /* dst[i] = src[idx[i]] */
int fl_ep_scatter_rows(const void* src, int64_t src_rows, const int32_t* idx, int64_t n, int hidden, void* dst,
                       int64_t dst_rows, fl_stream_t stream);  /* dst[idx[i]] = src[i] */
int fl_ep_send_rows(const void* x, int64_t num_tokens, const int32_t* send_slot /*[num_pairs]*/, int64_t num_pairs, int top_k,
                    int hidden, void* send_buf, int64_t send_rows, int64_t send_row_stride, fl_stream_t stream);  /* send_buf[send_slot[p]] = x[p / top_k] */
int fl_ep_combine(const void* ret_rows, int64_t num_ret_rows, const int32_t* send_slot, const float* weights,
                  int64_t num_tokens, int top_k, int hidden, void* out, int64_t weight_row_stride, fl_stream_t stream);

/* A1-masked: silu_and_mul_masked_post_quant_fwd (srt/layers/moe/executors/deep_ep_executor.py:106-170, Triton kernel :31-104)
 * between the two masked grouped GEMMs of the low-latency DeepEP path: x bf16 [G, rows_per_group, 2I] contiguous; only rows
 * < masked_m[g] of group g are read / written: q_out fp8 [G, rows_per_group, I] contiguous, s_out f32 at
 * g*s_stride_g + row*s_stride_m + kb*s_stride_k.  Arithmetic of A1 + Q1 (bit-exact vs their golden vectors). */
int fl_silu_and_mul_masked(const void* x, int num_groups, int64_t rows_per_group, int I, const int32_t* masked_m, void* q_out,
                           float* s_out, int64_t s_stride_g, int64_t s_stride_m, int64_t s_stride_k, fl_stream_t stream);

/* ---- R1: flashinfer.moe_fused_gate as called by biased_grouped_topk_gpu (srt/layers/moe/topk.py:709-733);
 * semantics of its torch statement biased_grouped_topk_impl (topk.py:596-663), renormalize=True, no fused shared
 * experts.  logits f32 [T, E] (E = 64*2^k <= 1024), bias f32 [E]; num_expert_group a power of two <= 64;
 * num_token_non_padded: optional DEVICE int32 scalar (rows at or beyond it get ids -1, topk.py:673-680).
 * Rows of the outputs are ordered by descending (sigmoid + bias); ties -> lower expert id. ---- */
int fl_moe_fused_gate(const float* logits, const float* bias, int64_t num_tokens, int num_experts, int num_expert_group,
                      int topk_group, int topk, float routed_scaling_factor, int apply_routed_scaling_factor_on_output,
                      const int32_t* num_token_non_padded, float* topk_weights /*[T, topk]*/,
                      int32_t* topk_ids /*[T, topk]*/, fl_stream_t stream);

/* ---- R1b: the plain (ungrouped) top-k routers imported beside it — flashinfer.topk_softmax (srt/layers/moe/topk.py:33, called by
 * fused_topk :505-520; torch statement fused_topk_torch_native :463-495), flashinfer.routing_flash (LongCat-Flash router, :836-845;
 * torch statement fused_topk_bias :51-70) and eps.utils.ops._ops.topk_sigmoid (:44-47).  logits f32 [T, E] (1 <= E <= 1024),
 * bias f32 [E] or NULL; score_fn 0 = softmax over the row, 1 = sigmoid; choice = score + bias; top-k by choice (descending, ties ->
 * lower expert id); weight = UNBIASED score, divided by the sum of the chosen scores if `renormalize`, times `scale`. ---- */
int fl_topk_gate(const float* logits, const float* bias, int64_t num_tokens, int num_experts, int topk, int score_fn,
                 int renormalize, float scale, float* topk_weights /*[T, topk]*/, int32_t* topk_ids /*[T, topk]*/,
                 fl_stream_t stream);

/* ---- R2: flashinfer.apply_rope_with_cos_sin_cache_inplace as RotaryEmbedding.forward_cuda calls it
 * (srt/layers/rotary_embedding.py:203-218) on q_pe / k_pe of the MLA path (models/deepseek_v2.py:646-647,695-696).
 * q bf16 [T, Hq, >=rotary_dim] and k bf16 [T, Hk, >=rotary_dim] rotated IN PLACE over their first rotary_dim elements
 * (element strides given, last dim contiguous, rows 16-B aligned); positions int64 [T]; cos_sin_cache f32
 * [max_position, rotary_dim] = cos | sin halves (:141-149,791-802).  fp32 arithmetic of forward_native (:804-846),
 * bit-exact.  is_neox: rotate halves (:50-53), else neighbouring pairs (:56-60, DeepSeek). ---- */
int fl_rope_inplace(const int64_t* positions, int64_t num_tokens, void* q, int64_t q_stride_token, int64_t q_stride_head,
                    int num_q_heads, void* k, int64_t k_stride_token, int64_t k_stride_head, int num_k_heads,
                    const float* cos_sin_cache, int64_t max_position, int rotary_dim, int is_neox, fl_stream_t stream);

/* The same call with what models/deepseek_v2.py:843-861 (forward_absorb_prepare) passes on the decode path:
 * output_q_rope / output_k_rope (rotated rows into a SEPARATE tensor, the source is left untouched; NULL = in place) and
 * FusedSetKVBufferArg (models/utils.py:52-81, bf16 KV cache only — enable_fused_set_kv_buffer() is false for fp8 KV):
 * v_buffer[cache_loc[t]] = value[t], k_buffer[cache_loc[t]] = rotated key[t] (k heads side by side), in the same launch.
 * All strides in bf16 elements; cache_loc int64 or int32 [T], negative = skip the token. */
typedef struct {
  const int64_t* positions; int64_t num_tokens;
  void* q; int64_t q_stride_token, q_stride_head; int num_q_heads;
  void* k; int64_t k_stride_token, k_stride_head; int num_k_heads;
  const float* cos_sin_cache; int64_t max_position; int rotary_dim; int is_neox;
  void* q_out; int64_t qo_stride_token, qo_stride_head;
  void* k_out; int64_t ko_stride_token, ko_stride_head;
  void* k_buffer; int64_t k_buffer_stride;
  void* v_buffer; int64_t v_buffer_stride;
  const void* value; int64_t value_stride; int value_dim;
  const void* cache_loc; int cache_loc_is_i64;
} FlRopeArgs;
int fl_rope(const FlRopeArgs* args, fl_stream_t stream);

/* ---- K7: the work of copy_all_layer_kv_cache_tiled (srt/mem_cache/memory_pool.py:2055-2090) as
 * MLATokenToKVPool.move_kv_cache launches it (:746-777): for every buffer b of the table, rows tgt_loc[i] <- src_loc[i]
 * with the semantics of `buf[tgt] = buf[src]` (:756-763): all sources are read before any target is written (overlapping
 * sets are safe).  data_ptrs / row_bytes: DEVICE tables [num_buffers] (base address, bytes per row; rows multiples of 4 B)
 * like the reference's data_ptrs / data_strides (:330-343); max_row_bytes = host-known maximum of row_bytes; tgt/src int64
 * DEVICE [num_locs], num_locs <= 8192 (more: fl_kv_move_staged); num_slots > 0: rows outside [0, num_slots) are skipped.  Bit-exact byte work. ---- */
int fl_kv_move(const uint64_t* data_ptrs, const int64_t* row_bytes, int num_buffers, int64_t max_row_bytes,
               const int64_t* tgt_loc, const int64_t* src_loc, int64_t num_locs, int64_t num_slots, fl_stream_t stream);
/* The same move for MORE rows than fl_kv_move holds in registers (num_locs up to 4,194,240): two launches through a caller-owned staging
 * area of num_locs x sum_row_bytes bytes (sum over the table's buffers) — every source row is copied out, then every target written: the
 * same "all reads before any write" semantics.  row_prefix: DEVICE [num_buffers], exclusive prefix sums of row_bytes (buffer b's staging
 * area starts at row_prefix[b] x num_locs).  A pair with either index outside [0, num_slots) is skipped. */
int fl_kv_move_staged(const uint64_t* data_ptrs, const int64_t* row_bytes, const int64_t* row_prefix, int num_buffers,
                      const int64_t* tgt_loc, const int64_t* src_loc, int64_t num_locs, int64_t num_slots, void* workspace,
                      int64_t workspace_bytes, int64_t sum_row_bytes, fl_stream_t stream);

/* ---- C8/C9: ep_scatter / ep_gather of the DeepExecutor (srt/layers/moe/executors/deep_ep_executor.py:271-332,
 * 396-430; Triton kernels :173-268, :335-393): between the DeepEP dispatch and the contiguous grouped GEMM, and back.
 * Strides in ELEMENTS of the tensor they belong to; topk / ids int32 or int64 (flag).  num_recv_tokens_per_expert: int32
 * [E], each a multiple of 128; num_rows = rows of output_tensor / m_indices.  Order inside an expert's group: atomic
 * cursors, unspecified as in the reference (:247).  expert_start_loc ends as start + count, like the reference's. ---- */
int fl_ep_scatter(const void* recv_x /*fp8 [T, H]*/, int64_t x_stride, const float* recv_x_scale /*[T, H/128]*/,
                  int64_t xs_stride, const void* recv_topk /*[T, K] local expert id or < 0*/, int topk_is_int64,
                  int64_t topk_stride, int64_t num_tokens, int top_k, int hidden,
                  const int32_t* num_recv_tokens_per_expert, int num_experts, int32_t* expert_start_loc /*[E] out*/,
                  void* output_tensor /*fp8 [M, H]*/, int64_t out_stride, float* output_tensor_scale /*[M, H/128]*/,
                  int64_t outs_stride, int32_t* m_indices /*[M]*/, int64_t num_rows, int32_t* output_index /*[T, K]*/,
                  int64_t oi_stride, fl_stream_t stream);
int fl_ep_gather(const void* input_tensor /*bf16 [M, H]*/, int64_t in_stride, int64_t num_rows,
                 const void* recv_topk_ids /*[T, K]*/, int ids_is_int64, int64_t ids_stride,
                 const float* recv_topk_weight /*[T, K]*/, int64_t w_stride, const int32_t* input_index /*[T, K]*/,
                 int64_t idx_stride, int64_t num_tokens, int top_k, int hidden, void* output_tensor /*bf16 [T, H]*/,
                 int64_t out_stride, fl_stream_t stream);

/* ---- B1: the small dense bf16 GEMMs between the big kernels — weight absorption
 * torch.bmm(q_nope.transpose(0,1), w_kc, out=Q[..., :512].transpose(0,1)) / torch.bmm(attn_output.transpose(0,1), w_vc)
 * (srt/models/deepseek_v2.py:840,886; both weights are stored k-contiguous, :1632-1633) and the router GEMM
 * flashinfer.dsv3_router_gemm(hidden, weight, out_dtype) (:177-179).  C[b,m,n] = sum_k A[b,m,k] * B[b,n,k]: bf16 operands
 * contiguous in k, strides in elements, fp32 accumulation, C bf16 (RNE) or f32; N % 32 == 0, K % 16 == 0. ---- */
int fl_bmm_bf16_nt(const void* A, const void* B, void* C, int batch, int64_t M, int N, int K, int64_t a_stride_b,
                   int64_t a_stride_m, int64_t b_stride_b, int64_t b_stride_n, int64_t c_stride_b, int64_t c_stride_m,
                   int out_is_f32, fl_stream_t stream);

/* The same product (one batch) split over K across workgroups, for few output tiles and a long K — the router GEMM
 * flashinfer.dsv3_router_gemm (srt/models/deepseek_v2.py:177-179: hidden [T, 7168] x gate weight [256, 7168]^T -> f32 logits):
 * f32 partials in `workspace` (at least fl_gemm_bf16_nt_splitk_workspace_bytes(M, N, K) bytes, 16-byte aligned; launches that
 * share it must be ordered), summed in split order by a second launch (deterministic).  N % 64 == 0, K % 64 == 0. */
int64_t fl_gemm_bf16_nt_splitk_workspace_bytes(int64_t M, int N, int K);
int fl_gemm_bf16_nt_splitk(const void* A, const void* B, void* C, int64_t M, int N, int K, int64_t a_stride_m,
                           int64_t b_stride_n, int64_t c_stride_m, int out_is_f32, void* workspace, int64_t workspace_bytes,
                           fl_stream_t stream);

/* ---- P1: ragged bf16 MHA prefill attention — flashinfer.BatchPrefillWithRaggedKVCacheWrapper.forward / forward_return_lse
 * (srt/layers/attention/flashinfer_mla_backend.py:449; layers/attention/chunker.py:304) — and flashinfer.merge_state
 * (srt/models/deepseek_v2.py:1037-1071).  Per request b (query rows qo_indptr[b] .. qo_indptr[b+1], keys kv_indptr[b] .. kv_indptr[b+1])
 * and head: o = softmax(sm_scale * q k^T + mask) v with bf16 operands, fp32 accumulation, bf16 P.  causal: bottom-right aligned — row i
 * of a request sees keys j <= i + (kv_len - qo_len).  lse (optional) is BASE 2: log2 sum_j 2^(sm_scale * log2(e) * q.k_j); the only
 * consumer is fl_merge_state, which reads the same base.  A row without a visible key (kv_len == 0, or above the causal diagonal) gets
 * o = 0, lse = -inf.  MHA only (one KV head per query head); head dims (192, 128) only.  Strides in ELEMENTS, last dimension contiguous,
 * rows 16-byte aligned (pointers, and strides multiples of 8); indptr values are clamped to [0, num_*_tokens].  Rows of `out` that
 * belong to no request are not written. ---- */
typedef struct FlPrefillArgs {
  int32_t struct_bytes;      /* = sizeof(FlPrefillArgs) as the CALLER compiled it; anything else is refused */
  int32_t batch;             /* B: requests */
  int64_t num_q_tokens;      /* Tq: rows of q / out / lse */
  int64_t num_kv_tokens;     /* Tk: rows of k / v */
  int32_t num_heads;         /* H (query heads = KV heads) */
  int32_t head_dim_qk, head_dim_vo;   /* 192, 128 */
  int32_t causal;
  float sm_scale;
  int32_t reserved;          /* 0 */
  const void* q;             /* bf16 [Tq, H, head_dim_qk] */
  int64_t q_stride_token, q_stride_head;
  const void* k;             /* bf16 [Tk, H, head_dim_qk] */
  int64_t k_stride_token, k_stride_head;
  const void* v;             /* bf16 [Tk, H, head_dim_vo] */
  int64_t v_stride_token, v_stride_head;
  const int32_t* qo_indptr;  /* i32 [B + 1], DEVICE */
  const int32_t* kv_indptr;  /* i32 [B + 1], DEVICE */
  void* out;                 /* bf16 [Tq, H, head_dim_vo] contiguous */
  float* lse;                /* f32 [Tq, H] contiguous, base 2; NULL = not wanted */
} FlPrefillArgs;
int fl_mha_prefill_ragged_bf16(const FlPrefillArgs* args, fl_stream_t stream);
/* Two attention states over disjoint key sets -> the state over their union: v_* bf16 [rows, head_dim] contiguous (rows = tokens x heads,
 * head_dim % 8 == 0), s_* f32 [rows] base-2 lse.  m = max(s_a, s_b): v = (v_a 2^(s_a-m) + v_b 2^(s_b-m)) / (2^(s_a-m) + 2^(s_b-m)),
 * s = m + log2(2^(s_a-m) + 2^(s_b-m)), in fp32.  A side with s = -inf returns the other side unchanged; both -inf: v = 0, s = -inf. */
int fl_merge_state(const void* v_a, const float* s_a, const void* v_b, const float* s_b, void* v_out, float* s_out, int64_t rows,
                   int head_dim, fl_stream_t stream);

/* ---- P2: absorbed (MQA) paged MLA attention over token-indexed KV — flashinfer.BatchMLAPagedAttentionWrapper.run with page size 1
 * (srt/layers/attention/flashinfer_mla_backend.py:486-541 forward_absorbed, :472-483 decode / verify of the plain backend).  Per request b
 * (query tokens qo_indptr[b] .. qo_indptr[b+1]; key j lives in slot kv_indices[kv_indptr[b] + j], j < kv_len = max(0, min(kv_len_arr[b],
 * kv_indptr[b+1] - kv_indptr[b]))), token i and head h:  s = sm_scale (q_nope . ckv[slot, :512] + q_pe . kpe[slot, :64]),
 * o = softmax(s + mask) ckv[slot, :512], with bf16 operands, fp32 accumulation, bf16 P.  causal: bottom-right aligned — token i sees keys
 * j <= i + (kv_len - q_len).  lse (optional) is BASE 2, as fl_mha_prefill_ragged_bf16 / fl_merge_state speak it.  A row without a visible
 * key gets o = 0, lse = -inf; rows of `out` that belong to no request are not written.  Head dims (512, 64) only.  Strides in ELEMENTS,
 * last dimension contiguous, rows 16-byte aligned (pointers, and strides multiples of 8); qo_indptr values are clamped to [0, num_q_tokens],
 * kv_indptr values to [0, num_kv_indices], slot indices to [0, num_kv_slots).  No split over the KV. ---- */
typedef struct FlMlaPrefillArgs {
  int32_t struct_bytes;      /* = sizeof(FlMlaPrefillArgs) as the CALLER compiled it; anything else is refused */
  int32_t batch;             /* B: requests */
  int64_t num_q_tokens;      /* T: rows of q_nope / q_pe / out / lse */
  int64_t num_kv_slots;      /* N: rows of ckv / kpe */
  int64_t num_kv_indices;    /* entries of kv_indices */
  int32_t num_heads;         /* H */
  int32_t head_dim_ckv, head_dim_kpe;   /* 512, 64 */
  int32_t causal;
  float sm_scale;
  int32_t reserved;          /* 0 */
  const void* q_nope;        /* bf16 [T, H, 512] */
  int64_t q_nope_stride_token, q_nope_stride_head;
  const void* q_pe;          /* bf16 [T, H, 64] */
  int64_t q_pe_stride_token, q_pe_stride_head;
  const void* ckv;           /* bf16 [N, 512] */
  int64_t ckv_stride_slot;
  const void* kpe;           /* bf16 [N, 64] */
  int64_t kpe_stride_slot;
  const int32_t* qo_indptr;  /* i32 [B + 1], DEVICE */
  const int32_t* kv_indptr;  /* i32 [B + 1], DEVICE */
  const int32_t* kv_indices; /* i32 [num_kv_indices], DEVICE */
  const int32_t* kv_len_arr; /* i32 [B], DEVICE */
  void* out;                 /* bf16 [T, H, 512] contiguous */
  float* lse;                /* f32 [T, H] contiguous, base 2; NULL = not wanted */
} FlMlaPrefillArgs;
int fl_mla_prefill_paged_bf16(const FlMlaPrefillArgs* args, fl_stream_t stream);

/* ---- S1: flashinfer.sampling — softmax, top-k / top-p renormalisation, top-k / top-p / min-p sampling over f32 rows (csrc/sampling.hip).
 * One workgroup per row, sort-free (radix descent on the f32 bit pattern to the row's exact cut value), one launch per call, no host
 * synchronisation, no allocation, hipGraph-capturable.  With p(k) the k-th largest value of a row, S its sum, M(x) = sum{p_j : p_j > x}:
 *   top-k : keep i iff p_i >= p(k) (ties at the k-th value are all kept; k >= V keeps everything; k < 1 is read as 1)
 *   top-p : keep i iff M(p_i) < top_p * S_base (ties at the last value kept; top_p >= 1 keeps everything with p_i > 0)
 *   FL_SAMPLING_JOINT        : the intersection, both on the input row, S_base = S       (filter_apply_order="joint")
 *   FL_SAMPLING_TOP_K_THEN_P : top-p on the top-k survivors, S_base = the mass top-k kept  (flashinfer's default, "top_k_first")
 *   min-p : keep i iff p_i >= min_p * max_j p_j (one f32 multiply)
 * Entries <= 0 (and NaN) are never kept.  Per-row parameters: a nullable DEVICE pointer, indexed by the ROW of probs (as flashinfer does
 * when `indices` maps samples to rows), or the scalar beside it when the pointer is NULL.  vocab <= 4,194,304.
 *   fl_sampling_softmax: out[b, :] = softmax(logits[b, :] / temperature[b]) — flashinfer.sampling.softmax (srt/speculative/eagle_worker.py:308,322);
 *                        a row of -inf gives zeros.  Reads probs (= logits), temperature / temperature_val, writes out f32 [batch, vocab].
 *   fl_sampling_renorm : out[b, i] = p_i / S_kept for kept i, exactly 0 otherwise — top_k_renorm_prob(s) / top_p_renorm_prob(s)
 *                        (srt/layers/sampler.py:96-97, srt/speculative/eagle_utils.py:252-263).  Modes TOP_K .. JOINT.
 *   fl_sampling_sample : out[b] = the smallest kept i of row (indices ? indices[b] : b) whose running kept mass in vocabulary order exceeds
 *                        u[b] * S_kept; the last kept i where f32 rounding leaves the sum below that; 0 for a row that keeps nothing —
 *                        top_k_top_p_sampling_from_probs / min_p_sampling_from_probs (srt/layers/sampler.py:98-110).  out i32 [batch]. ---- */
#define FL_SAMPLING_TOP_K 0
#define FL_SAMPLING_TOP_P 1
#define FL_SAMPLING_TOP_K_THEN_P 2
#define FL_SAMPLING_JOINT 3
#define FL_SAMPLING_MIN_P 4
typedef struct FlSamplingArgs {
  int32_t struct_bytes;      /* = sizeof(FlSamplingArgs) as the CALLER compiled it; anything else is refused */
  int32_t mode;              /* FL_SAMPLING_* (ignored by softmax) */
  int32_t batch;             /* B: rows written (softmax, renorm) / samples drawn */
  int32_t vocab;             /* V */
  int64_t num_rows;          /* rows of probs (>= B unless indices is given) */
  int64_t row_pitch;         /* ELEMENTS between rows of probs (>= V); rows 4-byte aligned, 16-byte loads from the first aligned element */
  const float* probs;        /* f32 [num_rows, V] at row_pitch (softmax: the logits) */
  const int32_t* indices;    /* i32 [B] DEVICE: sample b reads row indices[b] (clamped into the rows); NULL = row b.  sample only */
  const void* top_k;         /* i32 or i64 [num_rows] DEVICE, or NULL -> top_k_val */
  int32_t top_k_is_i64;
  int32_t reserved;          /* 0 */
  int64_t top_k_val;
  const float* top_p;        /* f32 [num_rows] DEVICE, or NULL -> top_p_val */
  const float* min_p;        /* f32 [num_rows] DEVICE, or NULL -> min_p_val */
  const float* temperature;  /* f32 [B] DEVICE, or NULL -> temperature_val.  softmax only */
  const float* u;            /* f32 [B] DEVICE uniforms in [0, 1).  sample only */
  float top_p_val, min_p_val, temperature_val;
  int32_t reserved2;         /* 0 */
  void* out;                 /* f32 [B, V] contiguous (softmax, renorm) / i32 [B] (sample) */
} FlSamplingArgs;
int fl_sampling_softmax(const FlSamplingArgs* args, fl_stream_t stream);
int fl_sampling_renorm(const FlSamplingArgs* args, fl_stream_t stream);
int fl_sampling_sample(const FlSamplingArgs* args, fl_stream_t stream);

/* ---- S2: speculative CHAIN verification — flashinfer.sampling.verify_chain_greedy / chain_speculative_sampling_target_only
 * (srt/speculative/eagle_utils.py:234,273; csrc/spec_verify.hip).  Request b owns D chain positions, flat index b * D + j: candidates[b, 0]
 * is the verified root, candidates[b, 1 .. D-1] the drafted chain.  One launch each, no host synchronisation, no allocation,
 * hipGraph-capturable.  Both write accept_index[b, 0] = b * D, accept_index[b, j] = b * D + j for the n accepted steps j = 1 .. n,
 * accept_token_num[b] = n, and n + 1 entries of predicts; nothing else of predicts / accept_index is written (the caller pre-fills -1).
 *   fl_spec_verify_greedy: step j is accepted iff candidates[b, j] == target_predict[b, j - 1] and every earlier step was;
 *                          predicts[b * D + j] = target_predict[b, j] for j = 0 .. n.
 *   fl_spec_verify_sample: step j is accepted iff every earlier step was and, with pt = target_probs[b, j - 1, candidates[b, j]] and
 *                          coin = uniform_samples[b, j - 1]: coin <= pt / max(threshold_acc, 1e-9) (f32 division) or pt >= threshold_single;
 *                          a candidate outside [0, V) is rejected.  predicts[b * D + j - 1] = candidates[b, j] for j = 1 .. n.  The final token,
 *                          predicts[b * D + n], is drawn from w_i = max(q_i - p_i, 0), q = target_probs[b, n, :], p = draft_probs[b, n, :] if
 *                          n < D - 1 else 0 (draft_probs is then not read), the rejected token candidates[b, n + 1] (n < D - 1, in range) given
 *                          weight 0: the smallest i with w_i > 0 whose running weight in vocabulary order exceeds uniform_final[b] * sum(w);
 *                          the last i with w_i > 0 where f32 rounding leaves the running sum below that; 0 when every weight is zero (the
 *                          conventions of fl_sampling_sample).  DIFFERENCE from upstream flashinfer: upstream zeroes the rejected token's
 *                          entry of draft_probs in place; here draft_probs is READ ONLY and never modified.
 *                          The row is split over num_slices workgroups per request; the last to arrive (a ticket per request) finishes, in
 *                          slice order: the result does not depend on arrival order.  The kernel leaves every ticket at 0. ---- */
typedef struct FlSpecVerifyArgs {
  int32_t struct_bytes;            /* = sizeof(FlSpecVerifyArgs) as the CALLER compiled it; anything else is refused */
  int32_t batch;                   /* B <= 65535 */
  int32_t num_draft;               /* D, 1 .. 32 */
  int32_t vocab;                   /* V <= 4,194,304.  sample only */
  int32_t num_slices;              /* S, 1 .. 512: workgroups per request.  sample only */
  int32_t target_predict_is_i64;   /* greedy only */
  int64_t accept_index_pitch;      /* ELEMENTS between rows of accept_index (>= D) */
  int32_t* predicts;               /* i32 [B * D] */
  int32_t* accept_index;           /* i32 [B, >= D] at accept_index_pitch */
  int32_t* accept_token_num;       /* i32 [B] */
  const int32_t* candidates;       /* i32 [B, D] contiguous */
  const void* target_predict;      /* i32 or i64 [B, D] contiguous.  greedy only */
  const float* uniform_samples;    /* f32 [B, D] contiguous.  sample only (as everything below) */
  const float* uniform_final;      /* f32 [B] */
  const float* target_probs;       /* f32 [B, D, V]: element (b, j, i) at b * target_pitch_b + j * target_pitch_d + i; rows 4-byte aligned */
  const float* draft_probs;        /* f32 [B, D, V] at draft_pitch_b / draft_pitch_d; read only */
  int64_t target_pitch_b, target_pitch_d, draft_pitch_b, draft_pitch_d;   /* ELEMENTS; pitch_d >= V */
  float threshold_single, threshold_acc;
  float* slice_sums;               /* f32 [B, S] workspace, any contents; may be NULL when S = 1 */
  uint32_t* tickets;               /* u32 [B] workspace, ALL ZERO on entry and on exit, not shared with a launch on another stream; NULL when S = 1 */
} FlSpecVerifyArgs;
int fl_spec_verify_greedy(const FlSpecVerifyArgs* args, fl_stream_t stream);
int fl_spec_verify_sample(const FlSpecVerifyArgs* args, fl_stream_t stream);

/* ---- P3: paged GQA attention over token-indexed KV, head dim 128, bf16 — flashinfer.BatchDecodeWithPagedKVCacheWrapper /
 * BatchPrefillWithPagedKVCacheWrapper with page size 1 and BatchPrefillWithRaggedKVCacheWrapper at 128/128
 * (srt/layers/attention/flashinfer_backend.py; csrc/gqa_paged_bf16.hip).  Per request b (query tokens qo_indptr[b] .. qo_indptr[b+1], or
 * the single token b when qo_indptr is NULL; key j lives in slot kv_indices[kv_indptr[b] + j], or in row kv_indptr[b] + j of k / v
 * themselves when kv_indices is NULL; kv_len = kv_indptr[b+1] - kv_indptr[b]), token i and query head h, with KV head h / G,
 * G = num_qo_heads / num_kv_heads:  o = softmax(sm_scale q k^T + mask) v, bf16 operands, fp32 accumulation, bf16 P.  causal: bottom-right
 * aligned — token i sees keys j <= i + (kv_len - q_len).  lse (optional) is BASE 2, as fl_merge_state reads it.  A row without a visible
 * key gets o = 0, lse = -inf; rows of `out` that belong to no request are not written.  Strides in ELEMENTS, last dimension contiguous,
 * rows 16-byte aligned; qo_indptr values are clamped to [0, num_q_tokens], kv_indptr values to [0, num_kv_indices], slot indices to
 * [0, num_kv_slots).  Everything that depends on lengths is read on the device: no host synchronisation, hipGraph-capturable.
 *   decode_form = 0: 128 (token, head-of-group) rows per workgroup, any q_len.
 *   decode_form = 1: the CALLER asserts q_len * G <= 16 for every request (tokens past that are not served: left unwritten); the waves of
 *                    a workgroup split the KV, and the KV of a request is cut into num_splits slices (1 .. 16), one workgroup each, whose
 *                    partial states land in `workspace` and are merged by a second kernel in slice order (deterministic).
 *                    workspace_bytes >= num_splits * num_q_tokens * num_qo_heads * 129 * 4 when num_splits > 1. ---- */
typedef struct FlGqaPagedArgs {
  int32_t struct_bytes;      /* = sizeof(FlGqaPagedArgs) as the CALLER compiled it; anything else is refused */
  int32_t batch;             /* B: requests */
  int64_t num_q_tokens;      /* T: rows of q / out / lse */
  int64_t num_kv_slots;      /* N: rows of k / v */
  int64_t num_kv_indices;    /* entries of kv_indices (kv_indices NULL: = N) */
  int32_t num_qo_heads, num_kv_heads;   /* Hq % Hkv == 0 */
  int32_t head_dim;          /* 128 */
  int32_t causal;
  float sm_scale;
  int32_t decode_form;       /* 0 / 1, see above */
  int32_t num_splits;        /* S, decode form only; row form: 1 */
  int32_t reserved;          /* 0 */
  const void* q;             /* bf16 [T, Hq, 128] */
  int64_t q_stride_token, q_stride_head;
  const void* k;             /* bf16 [N, Hkv, 128] */
  int64_t k_stride_slot, k_stride_head;
  const void* v;             /* bf16 [N, Hkv, 128] */
  int64_t v_stride_slot, v_stride_head;
  const int32_t* qo_indptr;  /* i32 [B + 1], DEVICE; NULL = one query token per request (T == B) */
  const int32_t* kv_indptr;  /* i32 [B + 1], DEVICE */
  const int32_t* kv_indices; /* i32 [num_kv_indices], DEVICE; NULL = identity (the ragged form) */
  void* out;                 /* bf16 [T, Hq, 128] contiguous */
  float* lse;                /* f32 [T, Hq] contiguous, base 2; NULL = not wanted */
  void* workspace;           /* DEVICE, 16-byte aligned, any contents; may be NULL when num_splits == 1 */
  int64_t workspace_bytes;
} FlGqaPagedArgs;
int fl_gqa_paged_attention_bf16(const FlGqaPagedArgs* args, fl_stream_t stream);
/* The same statement over an fp8 KV cache (csrc/gqa_paged_fp8kv.hip): `k` / `v` are OCP e4m3fn BYTES [N, Hkv, 128], their strides are in
 * elements = bytes and must be multiples of 16 with 16-byte aligned base pointers; q / out stay bf16.
 *   o = v_scale softmax(sm_scale k_scale q k8^T + mask) v8,   lse = log2 sum_j 2^(sm_scale k_scale log2e q . k8)   (base 2)
 * The bytes are dequantised exactly into the bf16 MFMAs of the bf16 kernel (fp32 accumulation, bf16 P; neither q nor P is quantised);
 * k_scale enters the logit scale, v_scale the final normaliser in fp32 (split partials carry it).  Both scales are finite and positive
 * (1.0f = none); a NaN byte of a visible token propagates.  Every other field, limit and guarantee is fl_gqa_paged_attention_bf16's. */
int fl_gqa_paged_attention_fp8kv(const FlGqaPagedArgs* args, float k_scale, float v_scale, fl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
