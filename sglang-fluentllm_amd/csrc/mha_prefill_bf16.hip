// P1 — ragged bf16 MHA prefill attention (flash-attention forward) and merge_state, gfx950 (MI355X) only.
//
// Replaces flashinfer.BatchPrefillWithRaggedKVCacheWrapper.forward / forward_return_lse as the DeepSeek-V3 / LongCat MLA prompt path calls
// them (srt/layers/attention/flashinfer_mla_backend.py:449 forward_normal_extend; layers/attention/chunker.py:304 per prefix chunk) and
// flashinfer.merge_state (models/deepseek_v2.py:1037-1071):
//   per request b and head h:  s[i, j] = sm_scale * q[i, :192] . k[j, :192],  o[i, :] = softmax_j(s[i, :] + mask) . v[:, :128]
//   causal mask bottom-right aligned: row i sees keys j <= i + (kv_len - qo_len);  lse[i] = log2 sum_j 2^(s[i, j] * log2 e)  (BASE 2)
//   a row without a visible key: o = 0, lse = -inf.
// q / k / v are bf16 with a contiguous last dimension and arbitrary (16-byte aligned) token / head strides — the reference passes
// v = kv[..., 128:] and q as a view of [T, H * 192]; nothing is copied.
//
// Mapping.  Workgroup = 4 waves = ONE head x 128 query rows of one request, 32 rows per wave; the KV of the request walks past in tiles
// of 64 tokens.  Grid = (ceil(Tq / 128) + B, H): only Tq, B and H are known on the host, so a workgroup finds its (request, row tile) by
// a scalar scan of qo_indptr — from the LAST row tile of the last request backwards, so that under a causal mask the long row tiles of
// a request are dispatched before its short ones — and surplus workgroups exit.  x runs over the row tiles of one head first: the
// workgroups in flight together read the same K / V rows out of L2.
//   * S^T[64 tok x 32 rows] = K . Q^T on v_mfma_f32_32x32x16_bf16 ("SwapAB"): the wave's Q fragment (12 k-steps, 48 VGPRs) is loaded once
//     and stays in registers; K fragments are conflict-free ds_read_b128 (row pitch 400 B: 16 consecutive rows start 9 chunks apart).  A
//     lane then owns 32 scores of ONE query row (lane & 31): row maximum and sum are in-lane but for one v_permlane32_swap per tile
//     (the partial sums of the two lane halves meet only in the epilogue).
//   * online softmax in base 2, fp32 statistics; P is rounded to bf16 and feeds O^T[128 dims x 32 rows] += V^T . P^T STRAIGHT from the
//     accumulator registers: accumulator registers 8 a .. 8 a + 7 of token sub-tile st are the B operand of k-step 2 st + a under the
//     token permutation  k = 8 lh + e  <->  token 16 ks + (e & 3) + 8 (e >> 2) + 4 lh;  V^T comes from the row-major V tile by
//     ds_read_b64_tr_b16 under the same permutation (a 16-lane group reads 4 consecutive tokens x 16 dims; row pitch 320 B puts the four
//     tokens of a 32-lane group in the four 64-B quarters of the bank period — mla_decode_bf16.hip lost 38 % of its LDS cycles there).
//     P takes no LDS round trip and O's lane owns the same query row as the scores: the rescale is in-lane, and skipped when no row moved.
//   * K / V tiles reach LDS through registers (16-B global loads of tile t + 1 issued in front of the MFMAs of tile t, written after the
//     barrier that retires tile t): one 45-KiB tile buffer, two workgroups per CU (256 VGPRs per wave) cover each other's barriers.
//     Rows past the visible end of the KV are ZERO in LDS (0 x NaN would poison the PV MFMA; nothing is read out of bounds).
//   * causal: KV tiles wholly above the workgroup's diagonal are never loaded, a wave skips the tiles above ITS 32 rows, only tiles that
//     cross a wave's diagonal (or the KV end) take the masking pass.
// No host synchronisation, no allocation: hipGraph-capturable.
#include "fl_common.h"

namespace {

typedef short v4s __attribute__((ext_vector_type(4)));

constexpr int kPfRows = 128;   // query rows per workgroup (32 per wave)
constexpr int kPfTile = 64;    // KV tokens per tile
constexpr float kPfLog2e = 1.4426950408889634f;

template <int DQK, int DVO>
struct PfLay {
  static_assert(DQK % 64 == 0 && DVO % 32 == 0 && DVO == 128, "K rows are staged as 8 lanes x (DQK / 64) chunks, V rows as 16 lanes x 1 chunk");
  static constexpr int kKSteps = DQK / 16;          // MFMA k-steps of S^T (12)
  static constexpr int kDTiles = DVO / 32;          // 32-dim tiles of O^T (4)
  static constexpr int kKPitch = DQK * 2 + 16;      // 400 B
  static constexpr int kVPitch = DVO * 2 + 64;      // 320 B
  static constexpr int kOffV = kPfTile * kKPitch;
  static constexpr int kLds = kOffV + kPfTile * kVPitch;   // 46,080 B
  static constexpr int kKJ = DQK / 64;              // 16-B chunks per staging lane and K row (3)
};

struct PfParams {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  uint16_t* o;
  float* lse;                 // may be null
  const int32_t* qo_indptr;
  const int32_t* kv_indptr;
  long long sqt, sqh, skt, skh, svt, svh;   // element strides (token, head)
  int B, Tq, Tk, H, causal;
  float scale_log2e;
};

__device__ __forceinline__ v8bf pf_as_v8bf(const uint4 u) {
  union { uint4 u; v8bf v; } x;
  x.u = u;
  return x.v;
}
__device__ __forceinline__ int pf_clamp(const int v, const int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// max / sum of a register over the lane pair (l, l ^ 32): after v_permlane32_swap of v with itself one result holds the lane's own value
// and the other its partner's
__device__ __forceinline__ float pf_pair_max(const float v) {
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(s[0]), __uint_as_float(s[1]));
}
__device__ __forceinline__ float pf_pair_sum(const float v) {
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}

template <int DQK, int DVO>
__global__ __launch_bounds__(256, 2) void mha_prefill_bf16_kernel(const PfParams p) {
  using L = PfLay<DQK, DVO>;
  __shared__ __attribute__((aligned(16))) uint8_t smem[L::kLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int h = blockIdx.y;

  // ---- (request, row tile) of this workgroup: last row tile of the last request first ----
  int req = -1, rt = 0, q_beg = 0, q_len = 0;
  {
    int x = blockIdx.x;
    for (int b = p.B - 1; b >= 0; --b) {
      const int beg = pf_clamp(p.qo_indptr[b], p.Tq), end = pf_clamp(p.qo_indptr[b + 1], p.Tq);
      const int len = end > beg ? end - beg : 0;
      const int nt = (len + kPfRows - 1) / kPfRows;
      if (x < nt) {
        req = b; rt = nt - 1 - x; q_beg = beg; q_len = len;
        break;
      }
      x -= nt;
    }
  }
  if (req < 0) return;   // surplus workgroup
  const int kv_beg = pf_clamp(p.kv_indptr[req], p.Tk);
  const int kv_end = pf_clamp(p.kv_indptr[req + 1], p.Tk);
  const int kv_len = kv_end > kv_beg ? kv_end - kv_beg : 0;
  const int off = kv_len - q_len;   // row i sees keys j <= i + off (causal)

  const int r0 = rt * kPfRows;
  const int wg_last = r0 + kPfRows - 1 < q_len - 1 ? r0 + kPfRows - 1 : q_len - 1;
  const int w_first = r0 + 32 * wave;
  const bool w_any = w_first < q_len;
  const int w_last = w_first + 31 < q_len - 1 ? w_first + 31 : q_len - 1;
  const int row = w_first + li;
  const bool row_ok = row < q_len;
  const int rowc = row_ok ? row : q_len - 1;   // (clamped loads; the tail rows are not stored)

  // visible key range [0, end): of the workgroup (tiles loaded), of the wave (tiles computed / masked), of the lane's row
  auto vis = [&](const int r) {
    int e = p.causal ? (r + off + 1 < kv_len ? r + off + 1 : kv_len) : kv_len;
    return e > 0 ? e : 0;
  };
  const int wg_end = vis(wg_last);
  const int w_end = w_any ? vis(w_last) : 0;
  const int w_full = w_any ? vis(w_first) : 0;   // every row of the wave sees keys [0, w_full)
  const int lim = vis(rowc);
  const int n_tiles = (wg_end + kPfTile - 1) / kPfTile;

  // ---- Q fragment: B operand of S^T = K . Q^T — lane (li, lh) holds q[row li][16 s + 8 lh .. + 7] of k-step s ----
  v8bf qf[L::kKSteps];
  {
    const uint16_t* qp = p.q + (long long)(q_beg + rowc) * p.sqt + (long long)h * p.sqh + 8 * lh;
#pragma unroll
    for (int s = 0; s < L::kKSteps; ++s) qf[s] = pf_as_v8bf(*reinterpret_cast<const uint4*>(qp + 16 * s));
  }

  // ---- staging of a KV tile: K rows by 8 lanes x kKJ chunks (32 rows per pass, 2 passes), V rows by 16 lanes (16 rows per pass, 4) ----
  const uint16_t* kp = p.k + (long long)kv_beg * p.skt + (long long)h * p.skh + 8 * (tid & 7);
  const uint16_t* vp = p.v + (long long)kv_beg * p.svt + (long long)h * p.svh + 8 * (tid & 15);
  const int k_row = tid >> 3, v_row = tid >> 4;
  uint4 kreg[2][L::kKJ], vreg[4];
  auto load_tile = [&](const int t0) {
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int tk = t0 + 32 * ps + k_row;
      const bool ok = tk < wg_end;
      const uint16_t* src = kp + (long long)(ok ? tk : 0) * p.skt;
#pragma unroll
      for (int j = 0; j < L::kKJ; ++j) kreg[ps][j] = ok ? *reinterpret_cast<const uint4*>(src + 64 * j) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int tk = t0 + 16 * ps + v_row;
      const bool ok = tk < wg_end;
      vreg[ps] = ok ? *reinterpret_cast<const uint4*>(vp + (long long)(ok ? tk : 0) * p.svt) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int ps = 0; ps < 2; ++ps)
#pragma unroll
      for (int j = 0; j < L::kKJ; ++j)
        *reinterpret_cast<uint4*>(smem + (32 * ps + k_row) * L::kKPitch + 16 * ((tid & 7) + 8 * j)) = kreg[ps][j];
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) *reinterpret_cast<uint4*>(smem + L::kOffV + (16 * ps + v_row) * L::kVPitch + 16 * (tid & 15)) = vreg[ps];
  };

  v16f o[L::kDTiles];
#pragma unroll
  for (int mt = 0; mt < L::kDTiles; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[mt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;   // l_run: this lane's HALF of the row sum (tokens 4 lh .. 4 lh + 3 of every 8)

  // K fragment of (sub-tile st, k-step s): row 32 st + li, bytes 32 s + 16 lh
  const uint8_t* kb = smem + li * L::kKPitch + 16 * lh;
  // V^T fragment by ds_read_b64_tr_b16: inside a 16-lane group source lane s16 points at token (s16 >> 2) and dims 4 (s16 & 3) .. + 3 of the
  // group's 16 dims; destination lane i receives dim i of tokens 0 .. 3.  Group (lh, b16): tokens 4 lh + .., dims 16 b16 + ..
  const uint8_t* vb = smem + L::kOffV + (4 * lh + ((lane & 15) >> 2)) * L::kVPitch + 2 * (16 * ((lane >> 4) & 1) + 4 * (lane & 3));

  if (n_tiles > 0) load_tile(0);
  for (int t = 0; t < n_tiles; ++t) {
    const int t0 = t * kPfTile;
    __syncthreads();   // tile t - 1 has been read by every wave
    store_tile();
    __syncthreads();   // tile t is in LDS
    if (t + 1 < n_tiles) load_tile(t0 + kPfTile);
    if (t0 >= w_end) continue;   // wholly above this wave's diagonal (wave-uniform)

    // ---- S^T = K . Q^T: two 32-token sub-tiles, two independent MFMA chains ----
    v16f sc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[0][r] = sc[1][r] = 0.f;
#pragma unroll
    for (int s = 0; s < L::kKSteps; ++s) {
      const v8bf a0 = pf_as_v8bf(*reinterpret_cast<const uint4*>(kb + 32 * s));
      const v8bf a1 = pf_as_v8bf(*reinterpret_cast<const uint4*>(kb + 32 * L::kKPitch + 32 * s));
      sc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, qf[s], sc[0], 0, 0, 0);
      sc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, qf[s], sc[1], 0, 0, 0);
    }
    // register r of sub-tile st = token t0 + 32 st + (r & 3) + 8 (r >> 2) + 4 lh of query row li
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[st][r] *= p.scale_log2e;
    if (t0 + kPfTile > w_full) {   // the tile crosses the wave's diagonal or the end of the KV
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (t0 + 32 * st + (r & 3) + 8 * (r >> 2) + 4 * lh >= lim) sc[st][r] = -INFINITY;
    }
    float mx = sc[0][0];
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[st][r]);
    mx = pf_pair_max(mx);
    const float m_new = fmaxf(m_run, mx);
    const float m_safe = m_new == -INFINITY ? 0.f : m_new;   // a row that has seen no key yet: every weight 2^(-inf) = 0, no NaN
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_safe);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[st][r] = __builtin_amdgcn_exp2f(sc[st][r] - m_safe);
        psum += sc[st][r];
      }
    l_run = l_run * alpha + psum;
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int mt = 0; mt < L::kDTiles; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[mt][r] *= alpha;
    }
    // ---- O^T += V^T . P^T: k-step ks = tokens 16 ks .. + 15 of the tile = accumulator registers 8 (ks & 1) .. + 7 of sub-tile ks >> 1 ----
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      union { uint4 u; v8bf v; } pb;
      const int st = ks >> 1, rb = 8 * (ks & 1);
      pb.u = make_uint4(fl_pack_bf16(sc[st][rb], sc[st][rb + 1]), fl_pack_bf16(sc[st][rb + 2], sc[st][rb + 3]),
                        fl_pack_bf16(sc[st][rb + 4], sc[st][rb + 5]), fl_pack_bf16(sc[st][rb + 6], sc[st][rb + 7]));
#pragma unroll
      for (int mt = 0; mt < L::kDTiles; ++mt) {
        union { v8bf v; v4s hv[2]; } a;
#pragma unroll
        for (int u = 0; u < 2; ++u)   // elements 4 u .. 4 u + 3: tokens 16 ks + 8 u + 4 lh + (0 .. 3)
          a.hv[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) v4s*)(vb + (16 * ks + 8 * u) * L::kVPitch + 64 * mt));
        o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, pb.v, o[mt], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: the two halves of the row sum meet, normalise, store.  O^T register r of tile mt = dim 32 mt + (r & 3) + 8 (r >> 2) + 4 lh ----
  const float l_tot = pf_pair_sum(l_run);
  if (!row_ok) return;
  const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
  const long long orow = (long long)(q_beg + row) * p.H + h;
  if (p.lse != nullptr && lh == 0) p.lse[orow] = l_tot > 0.f ? m_run + __builtin_amdgcn_logf(l_tot) : -INFINITY;
  uint16_t* op = p.o + orow * DVO + 4 * lh;
#pragma unroll
  for (int mt = 0; mt < L::kDTiles; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<uint2*>(op + 32 * mt + 8 * g) = make_uint2(fl_pack_bf16(o[mt][4 * g] * inv, o[mt][4 * g + 1] * inv),
                                                                   fl_pack_bf16(o[mt][4 * g + 2] * inv, o[mt][4 * g + 3] * inv));
}

// ---- merge_state: two partial attention states over disjoint key sets -> the state over their union (base-2 lse) ----
// One thread per 8 dims of a (token, head) row; fp32.  A side with s = -inf has weight exactly 0 and is not even multiplied in:
// the other side comes back unchanged (weight 1, divisor 1); both -inf: v = 0, s = -inf.
__global__ __launch_bounds__(256) void merge_state_kernel(const uint16_t* __restrict__ va, const float* __restrict__ sa,
                                                          const uint16_t* __restrict__ vb, const float* __restrict__ sb,
                                                          uint16_t* __restrict__ vo, float* __restrict__ so, const long long rows,
                                                          const int chunks) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = gid / chunks;
  if (row >= rows) return;
  const int c = (int)(gid - row * chunks);
  const float a = sa[row], b = sb[row];
  const float m = fmaxf(a, b);
  const bool none = m == -INFINITY;
  const float wa = none ? 0.f : __builtin_amdgcn_exp2f(a - m), wb = none ? 0.f : __builtin_amdgcn_exp2f(b - m);
  const float den = wa + wb;
  const float inv = none ? 0.f : 1.f / den;
  const long long e = (row * chunks + c) * 8;
  const uint4 ua = *reinterpret_cast<const uint4*>(va + e), ub = *reinterpret_cast<const uint4*>(vb + e);
  const uint32_t xa[4] = {ua.x, ua.y, ua.z, ua.w}, xb[4] = {ub.x, ub.y, ub.z, ub.w};
  uint32_t r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float f[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float fa = fl_bf16_to_f32((uint16_t)(xa[i] >> (16 * j))), fb = fl_bf16_to_f32((uint16_t)(xb[i] >> (16 * j)));
      f[j] = ((wa != 0.f ? fa * wa : 0.f) + (wb != 0.f ? fb * wb : 0.f)) * inv;
    }
    r[i] = fl_pack_bf16(f[0], f[1]);
  }
  *reinterpret_cast<uint4*>(vo + e) = make_uint4(r[0], r[1], r[2], r[3]);
  if (c == 0) so[row] = none ? -INFINITY : m + __builtin_amdgcn_logf(den);
}

}  // namespace

extern "C" int fl_mha_prefill_ragged_bf16(const FlPrefillArgs* a, fl_stream_t stream) {
  FL_CHECK_ARG(a != nullptr, "fl_mha_prefill_ragged_bf16: null argument struct");
  FL_CHECK_ARG(a->struct_bytes == (int32_t)sizeof(FlPrefillArgs),
               "fl_mha_prefill_ragged_bf16: struct_bytes = %d, this library's FlPrefillArgs has %d (caller built against another header)",
               (int)a->struct_bytes, (int)sizeof(FlPrefillArgs));
  FL_CHECK_ARG(a->head_dim_qk == 192 && a->head_dim_vo == 128,
               "fl_mha_prefill_ragged_bf16: only head_dim_qk=192, head_dim_vo=128 (got %d, %d)", a->head_dim_qk, a->head_dim_vo);
  FL_CHECK_ARG(a->batch >= 0 && a->num_heads >= 1 && a->num_heads <= 65535 && a->num_q_tokens >= 0 && a->num_kv_tokens >= 0 &&
                   a->num_q_tokens < (1ll << 31) - 256 && a->num_kv_tokens < (1ll << 31) - 256,
               "fl_mha_prefill_ragged_bf16: bad sizes");
  if (a->batch == 0 || a->num_q_tokens == 0) return FL_OK;
  FL_CHECK_ARG(a->q && a->out && a->qo_indptr && a->kv_indptr && (a->num_kv_tokens == 0 || (a->k && a->v)),
               "fl_mha_prefill_ragged_bf16: null pointer");
  FL_CHECK_ARG(((uintptr_t)a->q % 16) == 0 && ((uintptr_t)a->k % 16) == 0 && ((uintptr_t)a->v % 16) == 0 && ((uintptr_t)a->out % 16) == 0 &&
                   a->q_stride_token % 8 == 0 && a->q_stride_head % 8 == 0 && a->k_stride_token % 8 == 0 && a->k_stride_head % 8 == 0 &&
                   a->v_stride_token % 8 == 0 && a->v_stride_head % 8 == 0,
               "fl_mha_prefill_ragged_bf16: q / k / v rows must be 16-byte aligned (pointers, and strides multiples of 8 elements)");
  PfParams p;
  p.q = (const uint16_t*)a->q; p.k = (const uint16_t*)a->k; p.v = (const uint16_t*)a->v;
  p.o = (uint16_t*)a->out; p.lse = a->lse;
  p.qo_indptr = a->qo_indptr; p.kv_indptr = a->kv_indptr;
  p.sqt = a->q_stride_token; p.sqh = a->q_stride_head; p.skt = a->k_stride_token; p.skh = a->k_stride_head;
  p.svt = a->v_stride_token; p.svh = a->v_stride_head;
  p.B = a->batch; p.Tq = (int)a->num_q_tokens; p.Tk = (int)a->num_kv_tokens; p.H = a->num_heads; p.causal = a->causal != 0;
  p.scale_log2e = a->sm_scale * kPfLog2e;
  // every request has at most ceil(len / 128) <= len / 128 + 1 row tiles
  const long long tiles = (a->num_q_tokens + kPfRows - 1) / kPfRows + a->batch;
  FL_CHECK_ARG(tiles < (1ll << 31), "fl_mha_prefill_ragged_bf16: grid too large");
  mha_prefill_bf16_kernel<192, 128><<<dim3((unsigned)tiles, (unsigned)a->num_heads), dim3(256), 0, (hipStream_t)stream>>>(p);
  FL_CHECK_LAUNCH("mha_prefill_bf16_kernel");
  return FL_OK;
}

extern "C" int fl_merge_state(const void* v_a, const float* s_a, const void* v_b, const float* s_b, void* v_out, float* s_out,
                              int64_t rows, int head_dim, fl_stream_t stream) {
  FL_CHECK_ARG(rows >= 0 && head_dim > 0 && head_dim % 8 == 0, "fl_merge_state: rows=%lld, head_dim=%d must be a multiple of 8",
               (long long)rows, head_dim);
  if (rows == 0) return FL_OK;
  FL_CHECK_ARG(v_a && s_a && v_b && s_b && v_out && s_out, "fl_merge_state: null pointer");
  FL_CHECK_ARG(((uintptr_t)v_a % 16) == 0 && ((uintptr_t)v_b % 16) == 0 && ((uintptr_t)v_out % 16) == 0,
               "fl_merge_state: v rows must be 16-byte aligned");
  const int chunks = head_dim / 8;
  const long long blocks = (rows * chunks + 255) / 256;
  FL_CHECK_ARG(blocks < (1ll << 31), "fl_merge_state: grid too large");
  merge_state_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(
      (const uint16_t*)v_a, s_a, (const uint16_t*)v_b, s_b, (uint16_t*)v_out, s_out, rows, chunks);
  FL_CHECK_LAUNCH("merge_state_kernel");
  return FL_OK;
}
