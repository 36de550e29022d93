// What the paged GQA kernels share (gqa_paged_bf16.hip, gqa_paged_fp8kv.hip): the kernel parameters, the lane-swap reductions, the query
// tokens of the decode form and the merge of its split partials.  Included inside each file's anonymous namespace, after fl_common.h.
#pragma once

typedef short v4s __attribute__((ext_vector_type(4)));

constexpr int kGqDecRows = 16;                 // decode form: rows per (request, KV head)
constexpr int kGqMaxSplits = 16;
constexpr float kGqLog2e = 1.4426950408889634f;

struct GqParams {
  const uint16_t* q;
  const uint16_t* k;   // (gqa_paged_fp8kv.hip: e4m3fn bytes, strides in bytes)
  const uint16_t* v;
  uint16_t* o;
  float* lse;        // may be null
  float* part_o;     // decode form, S > 1: f32 [S, T, Hq, 128]
  float* part_lse;   //                     f32 [S, T, Hq]
  const int32_t* qo_indptr;    // null: request b = query token b
  const int32_t* kv_indptr;
  const int32_t* kv_indices;   // null: identity
  long long sqt, sqh, sks, skh, svs, svh;   // element strides
  int B, T, N, NI, Hq, G, S, causal;
  float scale_log2e;
};

__device__ __forceinline__ v8bf gq_as_v8bf(const uint4 u) {
  union { uint4 u; v8bf v; } x;
  x.u = u;
  return x.v;
}
__device__ __forceinline__ int gq_clamp(const int v, const int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float gq_pair_max(const float v) {   // over the lane pair (l, l ^ 32)
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(s[0]), __uint_as_float(s[1]));
}
__device__ __forceinline__ float gq_pair_sum(const float v) {
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}
// max / sum over the four lanes (l & 15) + 16 g: v_permlane16_swap pairs lane groups (0, 1) and (2, 3), v_permlane32_swap the pairs
__device__ __forceinline__ float gq_quad_max(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  return gq_pair_max(v);
}
__device__ __forceinline__ float gq_quad_sum(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  return gq_pair_sum(v);
}
// query tokens [beg, beg + len) of request b; the decode form serves at most 16 / G of them
__device__ __forceinline__ void gq_decode_tokens(const GqParams& p, const int b, int& beg, int& len) {
  beg = p.qo_indptr ? gq_clamp(p.qo_indptr[b], p.T) : gq_clamp(b, p.T);
  const int end = p.qo_indptr ? gq_clamp(p.qo_indptr[b + 1], p.T) : gq_clamp(b + 1, p.T);
  len = end > beg ? end - beg : 0;
  len = len < kGqDecRows / p.G ? len : kGqDecRows / p.G;
}

// ---- merge of the S partial states of the decode form: one workgroup per (request, KV head), thread = (row, 8 dims), slices in order ----
__global__ __launch_bounds__(256) void gqa_split_merge_kernel(const GqParams p) {
  int q_beg, q_len;
  gq_decode_tokens(p, blockIdx.x, q_beg, q_len);
  const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
  if (r >= q_len * p.G) return;
  const int ti = r / p.G;
  const long long orow = (long long)(q_beg + ti) * p.Hq + (int)blockIdx.y * p.G + (r - ti * p.G);
  const long long pitch = (long long)p.T * p.Hq;
  float m = -INFINITY;
  for (int s = 0; s < p.S; ++s) m = fmaxf(m, p.part_lse[s * pitch + orow]);
  float den = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  if (m != -INFINITY) {
    for (int s = 0; s < p.S; ++s) {
      const float ls = p.part_lse[s * pitch + orow];
      if (ls == -INFINITY) continue;   // an empty slice: its o was never meaningful
      const float w = __builtin_amdgcn_exp2f(ls - m);
      den += w;
      const float4* src = reinterpret_cast<const float4*>(p.part_o + (s * pitch + orow) * 128 + 8 * c);
      const float4 a = src[0], b = src[1];
      acc[0] += w * a.x; acc[1] += w * a.y; acc[2] += w * a.z; acc[3] += w * a.w;
      acc[4] += w * b.x; acc[5] += w * b.y; acc[6] += w * b.z; acc[7] += w * b.w;
    }
  }
  const float inv = den > 0.f ? 1.f / den : 0.f;
  *reinterpret_cast<uint4*>(p.o + orow * 128 + 8 * c) =
      make_uint4(fl_pack_bf16(acc[0] * inv, acc[1] * inv), fl_pack_bf16(acc[2] * inv, acc[3] * inv),
                 fl_pack_bf16(acc[4] * inv, acc[5] * inv), fl_pack_bf16(acc[6] * inv, acc[7] * inv));
  if (c == 0 && p.lse != nullptr) p.lse[orow] = den > 0.f ? m + __builtin_amdgcn_logf(den) : -INFINITY;
}
