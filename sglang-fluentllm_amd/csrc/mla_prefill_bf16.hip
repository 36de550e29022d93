// P2 — absorbed (MQA) paged MLA attention over token-indexed KV, bf16, ragged and causal, gfx950 (MI355X) only.
//
// Replaces flashinfer.BatchMLAPagedAttentionWrapper.run as the DeepSeek-V3 / LongCat MLA backend calls it with page size 1
// (srt/layers/attention/flashinfer_mla_backend.py:486-541 forward_absorbed — prompts under a captured prefill graph, prompts with
// flashinfer_mla_disable_ragged — and :472-483, decode / verify of the plain backend):
//   per request b, query token i, head h, key j:  slot(j) = kv_indices[kv_indptr[b] + j]
//     s[i, h, j] = sm_scale * (q_nope[i, h, :512] . ckv[slot(j), :512] + q_pe[i, h, :64] . kpe[slot(j), :64])
//     o[i, h, :] = softmax_j(s[i, h, :] + mask) . ckv[slot(.), :512],   lse[i, h] = log2 sum_j 2^(s * log2 e)   (BASE 2)
//   kv_len = max(0, min(kv_len_arr[b], kv_indptr[b + 1] - kv_indptr[b]));  causal, bottom-right aligned: token i sees j <= i + kv_len - q_len;
//   a row that sees no key: o = 0, lse = -inf;  query rows of no request stay unwritten;  slot indices are clamped into [0, N).
// Every head of a token attends over the SAME latent row per key: 576 dims for the scores, the first 512 of them are the values.
//
// Mapping.  The (token, head) pairs of one request are flattened as r = i * H + h and cut into row tiles of 64; a workgroup = 4 waves =
// one row tile (4 tokens at H = 16, half a token at H = 128; H need not divide 64), the causal limit is per row from r / H.  Grid =
// ceil(T H / 64) + B: only T, B and H are known on the host, a workgroup finds its (request, row tile) by a scan of qo_indptr from the LAST
// row tile of the last request backwards (row tiles of one request are adjacent and share its KV in L2; under a causal mask the long
// ones go first), surplus workgroups exit.  The KV walks past in tiles of 32 tokens; tiles wholly above the workgroup's last token are
// never loaded, only tiles that cross a wave's limit or the KV end take the masking pass.
//   * Gather: one ckv row is 1,024 B = ONE wave-wide LDS-DMA piece (global_load_lds_dwordx4, 16 B per lane), eight kpe rows the next;
//     a wave gathers tile rows 8 w .. 8 w + 7, whose slot indices it read one tile ahead.  Two tile buffers (2 x 36 KiB): the pieces of
//     tile t + 1 are in flight under all of tile t, no staging registers.  A DMA lane lands at (base + 16 lane) but fetches from ANY
//     address, so the swizzle costs nothing: position p of tile row j holds source chunk p ^ sw(j), sw(j) = 4 (j & 3) + ((j >> 2) & 3) —
//     the 16 rows of a K fragment read (ds_read_b128, one column) start in 16 different 16-B bank groups, and the 4 tokens of a V^T read
//     sit in the four 64-B quarters of the bank period.  kpe pieces are permuted likewise (see issue()).  ckv rows past the visible end
//     are ZERO in LDS (0 x NaN would poison PV); kpe rows there come from a clamped slot and only feed scores that are masked.
//   * One KV tile, read twice: as K (576 dims) for S^T[32 tok x 16 rows] = K . Q^T of each wave's 16 rows on v_mfma_f32_16x16x32_bf16
//     with the wave's Q fragment (18 k-steps, 72 VGPRs) resident; as V (first 512 dims) for O^T[128 dims x 64 rows] += V^T . P^T on
//     v_mfma_f32_32x32x16_bf16, wave w owning dims 128 w .. 128 w + 127 of ALL 64 rows (8 accumulators, 128 VGPRs); V^T comes from the
//     row-major tile by ds_read_b64_tr_b16.  Between the two: online softmax in base 2 (fp32 statistics; a lane owns 8 scores of one
//     row, the four lane groups meet by v_permlane16/32_swap), P rounded to bf16 and the row's rescale factor go to LDS, one barrier,
//     and every wave reads all 64 rows' P as its B operand.  O is rescaled only when some row's maximum moved.
//   * Two barriers per tile; 79,360 B of LDS and 256 registers per wave: two workgroups per CU cover each other's barriers.
// No split over the KV: with one token per request (decode form) this is correct but runs on B ceil(H / 64) workgroups.
// No host synchronisation, no allocation: hipGraph-capturable.
#include "fl_common.h"

namespace {

typedef short v4s __attribute__((ext_vector_type(4)));

constexpr int kMpRows = 64;                    // (token, head) rows per workgroup, 16 per wave in the score phase
constexpr int kMpTile = 32;                    // KV tokens per tile
constexpr int kMpRowB = 1024;                  // one ckv row in LDS (swizzled, unpadded)
constexpr int kMpOffR = kMpTile * kMpRowB;     // kpe: four pieces of 8 rows x 128 B
constexpr int kMpBuf = kMpOffR + 4 * 1024;     // 36,864 B per tile buffer
constexpr int kMpOffP = 2 * kMpBuf;            // P: 64 rows x 32 bf16, pitch 80 B (5 chunks: 16 rows start in 16 bank groups)
constexpr int kMpPPitch = 80;
constexpr int kMpOffA = kMpOffP + kMpRows * kMpPPitch;   // f32 [64] rescale factor of the tile
constexpr int kMpOffL = kMpOffA + kMpRows * 4;           // f32 [64] 1 / row sum (epilogue)
constexpr int kMpLds = kMpOffL + kMpRows * 4;            // 79,360 B
constexpr float kMpLog2e = 1.4426950408889634f;
static_assert(2 * kMpLds <= 160 * 1024, "two workgroups per CU");

struct MpParams {
  const uint16_t* q_nope;
  const uint16_t* q_pe;
  const uint16_t* ckv;
  const uint16_t* kpe;
  uint16_t* o;
  float* lse;   // may be null
  const int32_t* qo_indptr;
  const int32_t* kv_indptr;
  const int32_t* kv_indices;
  const int32_t* kv_len_arr;
  long long sqnt, sqnh, sqpt, sqph, sct, skt;   // element strides
  int B, T, N, NI, H, causal;
  float scale_log2e;
};

__device__ __forceinline__ v8bf mp_as_v8bf(const uint4 u) {
  union { uint4 u; v8bf v; } x;
  x.u = u;
  return x.v;
}
__device__ __forceinline__ int mp_clamp(const int v, const int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// max / sum over the four lanes (l & 15) + 16 g: v_permlane16_swap pairs lane groups (0, 1) and (2, 3), v_permlane32_swap the pairs
__device__ __forceinline__ float mp_quad_max(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float mp_quad_sum(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

__global__ __launch_bounds__(256, 2) void mla_prefill_bf16_kernel(const MpParams p) {
  __shared__ __attribute__((aligned(1024))) uint8_t smem[kMpLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15, g = lane >> 4;    // score phase: query row of the wave, token quarter
  const int n32 = lane & 31, lh = lane >> 5;   // PV phase: query row of a 32-row half, token half

  // ---- (request, row tile) of this workgroup: last row tile of the last request first ----
  int req = -1, rt = 0, q_beg = 0, q_len = 0;
  {
    int x = blockIdx.x;
    for (int b = p.B - 1; b >= 0; --b) {
      const int beg = mp_clamp(p.qo_indptr[b], p.T), end = mp_clamp(p.qo_indptr[b + 1], p.T);
      const int len = end > beg ? end - beg : 0;
      const int nt = (len * p.H + kMpRows - 1) / kMpRows;
      if (x < nt) {
        req = b; rt = nt - 1 - x; q_beg = beg; q_len = len;
        break;
      }
      x -= nt;
    }
  }
  if (req < 0) return;   // surplus workgroup
  const int kv_beg = mp_clamp(p.kv_indptr[req], p.NI);
  const int kv_span = mp_clamp(p.kv_indptr[req + 1], p.NI) - kv_beg;
  int kv_len = p.kv_len_arr[req];
  kv_len = kv_len < kv_span ? kv_len : kv_span;
  kv_len = (kv_len > 0 && p.N > 0) ? kv_len : 0;
  const int off = kv_len - q_len;   // token i sees keys j <= i + off (causal)
  const int nrows = q_len * p.H;    // >= 1: this request has a row tile

  // visible key range [0, end) of query token i
  auto vis = [&](const int i) {
    const int e = p.causal ? (i + off + 1 < kv_len ? i + off + 1 : kv_len) : kv_len;
    return e > 0 ? e : 0;
  };
  const int r0 = rt * kMpRows;
  const int wg_end = vis((r0 + kMpRows - 1 < nrows - 1 ? r0 + kMpRows - 1 : nrows - 1) / p.H);   // tiles loaded
  const int n_tiles = (wg_end + kMpTile - 1) / kMpTile;
  const int w_first = r0 + 16 * wave;
  const bool w_any = w_first < nrows;
  const int w_end = w_any ? vis((w_first + 15 < nrows - 1 ? w_first + 15 : nrows - 1) / p.H) : 0;   // tiles this wave scores
  const int w_full = w_any ? vis(w_first / p.H) : 0;   // every row of the wave sees keys [0, w_full)
  const int row = w_first + n16;
  const int rowc = row < nrows ? row : nrows - 1;   // (clamped loads; the tail rows are not stored)
  const int ti = rowc / p.H, hh = rowc - ti * p.H;
  const int lim = vis(ti);

  // ---- Q fragment: B operand of S^T = K . Q^T — lane (n16, g) holds q[row n16][32 s + 8 g .. + 7] of k-step s; steps 16, 17 are q_pe ----
  v8bf qf[18];
  {
    const uint16_t* qn = p.q_nope + (long long)(q_beg + ti) * p.sqnt + (long long)hh * p.sqnh + 8 * g;
    const uint16_t* qp = p.q_pe + (long long)(q_beg + ti) * p.sqpt + (long long)hh * p.sqph + 8 * g;
#pragma unroll
    for (int s = 0; s < 16; ++s) qf[s] = mp_as_v8bf(*reinterpret_cast<const uint4*>(qn + 32 * s));
    qf[16] = mp_as_v8bf(*reinterpret_cast<const uint4*>(qp));
    qf[17] = mp_as_v8bf(*reinterpret_cast<const uint4*>(qp + 32));
  }

  // ---- gather of a KV tile: wave w brings tile rows 8 w .. 8 w + 7; lane l holds the (clamped) slot of row 8 w + (l & 7) ----
  auto load_slot = [&](const int t) {
    const int tok = t * kMpTile + 8 * wave + (lane & 7);
    const int s = tok < kv_len ? p.kv_indices[kv_beg + tok] : 0;
    return mp_clamp(s, p.N - 1);
  };
  auto issue = [&](const int t, const int slotv) {
    uint8_t* buf = smem + (t & 1) * kMpBuf;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int j = 8 * wave + jj;
      uint8_t* dst = buf + j * kMpRowB;
      if (t * kMpTile + j < wg_end) {   // wave-uniform
        const int s = __builtin_amdgcn_readlane(slotv, jj);
        const int sw = ((j & 3) << 2) | ((j >> 2) & 3);
        fl_dma16_s(p.ckv + (long long)s * p.sct, 16u * (unsigned)(lane ^ sw), dst);
      } else {
        *reinterpret_cast<uint4*>(dst + 16 * lane) = make_uint4(0, 0, 0, 0);
      }
    }
    // kpe piece w = rows 8 w .. 8 w + 7 x 8 chunks: position 16 a + b holds row 8 w + (b & 7), chunk 2 a + (((b >> 3) ^ w) & 1) — the 16
    // rows of a K fragment read (two pieces, one chunk) start in 16 different 16-B bank groups
    const int ch = 2 * (lane >> 4) + (((lane >> 3) ^ wave) & 1);
    fl_dma16(p.kpe + (long long)slotv * p.skt + 8 * ch, buf + kMpOffR + 1024 * wave);
  };

  v16f acc[4][2];   // O^T: [32-dim tile of the wave's 128 dims][32-row half]
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][h2][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;   // l_run: this lane's QUARTER of the row sum
  float* const alpha_s = reinterpret_cast<float*>(smem + kMpOffA);
  float* const inv_s = reinterpret_cast<float*>(smem + kMpOffL);

  int slot_next = 0;
  if (n_tiles > 0) {
    issue(0, load_slot(0));
    if (n_tiles > 1) slot_next = load_slot(1);
  }
  // this lane's P destination: row 16 w + n16; token 16 st + 4 g + r of the tile sits at position 16 st + 8 (g & 1) + 4 (g >> 1) + r,
  // the order in which the PV B operand (k = 8 lh + e <-> token 16 ks + 8 (e >> 2) + 4 lh + (e & 3)) reads 16 contiguous bytes
  uint8_t* const prow = smem + kMpOffP + (16 * wave + n16) * kMpPPitch + 2 * (8 * (g & 1) + 4 * (g >> 1));
  // swizzle of tile rows n16 and 16 + n16: chunk c at position c ^ (4 (n16 & 3) + ((n16 >> 2) & 3)); the k-step enters by XOR on bits 6, 7
  const int k_off = n16 * kMpRowB + 64 * (n16 & 3) + 16 * (g ^ ((n16 >> 2) & 3));
  // V^T fragment by ds_read_b64_tr_b16: inside a 16-lane group source lane s16 points at token (s16 >> 2) and dims 4 (s16 & 3) .. + 3 of
  // the group's 16 dims; destination lane i receives dim i of tokens 0 .. 3.  Group (lh, b16): tokens 4 lh + .., dims 16 b16 + ..
  // Lane part of the address of tile row 4 lh + k4 (swizzle 4 k4 + lh), dims 128 w + 16 b16 + 4 (l & 3): the 32-dim tile mt and the
  // token octet u (swizzle + 2 u) enter by XOR on bits 5 .. 7, the token sub-tile as an immediate offset
  const int k4 = (lane & 15) >> 2;
  const int v_off = (4 * lh + k4) * kMpRowB + 256 * wave + 64 * k4 + 16 * ((2 * ((lane >> 4) & 1) + ((lane & 3) >> 1)) ^ lh) + 8 * (lane & 1);
  const int kp_off = kMpOffR + 1024 * (n16 >> 3) + 16 * (16 * (g >> 1) + ((n16 & 7) | ((((g & 1) ^ (n16 >> 3)) & 1) << 3)));

  for (int t = 0; t < n_tiles; ++t) {
    const int t0 = t * kMpTile;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile t
    __syncthreads();   // tile t is in LDS; tile t - 1, its P and its rescale factors have been read by every wave
    if (t + 1 < n_tiles) {
      issue(t + 1, slot_next);
      if (t + 2 < n_tiles) slot_next = load_slot(t + 2);
    }
    const uint8_t* kb = smem + (t & 1) * kMpBuf;

    if (t0 < w_end) {   // (wave-uniform)
      // ---- S^T[32 tok x 16 rows] = K . Q^T: two 16-token sub-tiles, two independent MFMA chains ----
      v4f sc0 = {0.f, 0.f, 0.f, 0.f}, sc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 16; ++s) {   // chunk 4 s + g of rows n16 and 16 + n16 (same swizzle): position 4 (s ^ swc) + (g ^ swd)
        const uint8_t* ka = kb + (k_off ^ (64 * (s & 3))) + 256 * (s >> 2);
        const v8bf a0 = mp_as_v8bf(*reinterpret_cast<const uint4*>(ka));
        const v8bf a1 = mp_as_v8bf(*reinterpret_cast<const uint4*>(ka + 16 * kMpRowB));
        sc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, qf[s], sc0, 0, 0, 0);
        sc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, qf[s], sc1, 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const v8bf a0 = mp_as_v8bf(*reinterpret_cast<const uint4*>(kb + kp_off + 512 * s));
        const v8bf a1 = mp_as_v8bf(*reinterpret_cast<const uint4*>(kb + kp_off + 2048 + 512 * s));
        sc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, qf[16 + s], sc0, 0, 0, 0);
        sc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, qf[16 + s], sc1, 0, 0, 0);
      }
      // y[r] = token t0 + 16 (r >> 2) + 4 g + (r & 3) of query row n16
      float y[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) y[r] = (r < 4 ? sc0[r & 3] : sc1[r & 3]) * p.scale_log2e;
      if (t0 + kMpTile > w_full) {   // the tile crosses a row's causal limit or the end of the KV
#pragma unroll
        for (int r = 0; r < 8; ++r)
          if (t0 + 16 * (r >> 2) + 4 * g + (r & 3) >= lim) y[r] = -INFINITY;
      }
      float mx = y[0];
#pragma unroll
      for (int r = 1; r < 8; ++r) mx = fmaxf(mx, y[r]);
      mx = mp_quad_max(mx);
      const float m_new = fmaxf(m_run, mx);
      const float m_safe = m_new == -INFINITY ? 0.f : m_new;   // a row that has seen no key yet: every weight 2^(-inf) = 0, no NaN
      const float alpha = m_new == m_run ? 1.f : __builtin_amdgcn_exp2f(m_run - m_safe);
      m_run = m_new;
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        y[r] = __builtin_amdgcn_exp2f(y[r] - m_safe);
        psum += y[r];
      }
      l_run = l_run * alpha + psum;
      *reinterpret_cast<uint2*>(prow) = make_uint2(fl_pack_bf16(y[0], y[1]), fl_pack_bf16(y[2], y[3]));
      *reinterpret_cast<uint2*>(prow + 32) = make_uint2(fl_pack_bf16(y[4], y[5]), fl_pack_bf16(y[6], y[7]));
      if (g == 0) alpha_s[16 * wave + n16] = alpha;
    } else {   // wholly above this wave's rows (or the wave has none): P = 0, nothing moves
      *reinterpret_cast<uint2*>(prow) = make_uint2(0, 0);
      *reinterpret_cast<uint2*>(prow + 32) = make_uint2(0, 0);
      if (g == 0) alpha_s[16 * wave + n16] = 1.f;
    }
    __syncthreads();   // P and the rescale factors of all 64 rows are in LDS

    // ---- O^T[128 dims x 64 rows] += V^T . P^T; accumulator register r of acc[mt][h2] = dim 128 w + 32 mt + (r & 3) + 8 (r >> 2) + 4 lh
    //      of row 32 h2 + n32 ----
    const float al0 = alpha_s[n32], al1 = alpha_s[32 + n32];
    if (__any(al0 != 1.f || al1 != 1.f)) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc[mt][0][r] *= al0;
          acc[mt][1][r] *= al1;
        }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      v8bf pb[2];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2)
        pb[h2] = mp_as_v8bf(*reinterpret_cast<const uint4*>(smem + kMpOffP + (32 * h2 + n32) * kMpPPitch + 2 * (16 * ks + 8 * lh)));
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        union { v8bf v; v4s hv[2]; } a;
#pragma unroll
        for (int u = 0; u < 2; ++u)   // elements 4 u .. 4 u + 3: tokens 16 ks + 8 u + 4 lh + (0 .. 3)
          a.hv[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) v4s*)(kb + (v_off ^ (64 * mt + 32 * u)) + (16 * ks + 8 * u) * kMpRowB));
        acc[mt][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, pb[0], acc[mt][0], 0, 0, 0);
        acc[mt][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, pb[1], acc[mt][1], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: the four quarters of the row sum meet; 1 / sum goes through LDS to the lanes that hold the row's O ----
  const float l_tot = mp_quad_sum(l_run);
  if (g == 0) {
    inv_s[16 * wave + n16] = l_tot > 0.f ? 1.f / l_tot : 0.f;
    if (p.lse != nullptr && row < nrows)
      p.lse[(long long)q_beg * p.H + row] = l_tot > 0.f ? m_run + __builtin_amdgcn_logf(l_tot) : -INFINITY;
  }
  __syncthreads();
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2) {
    const int rr = r0 + 32 * h2 + n32;
    if (rr >= nrows) continue;
    const float inv = inv_s[32 * h2 + n32];
    uint16_t* op = p.o + ((long long)q_beg * p.H + rr) * 512 + 128 * wave + 4 * lh;   // out is [T, H, 512] contiguous: row (q_beg + i) H + h
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4)
        *reinterpret_cast<uint2*>(op + 32 * mt + 8 * q4) =
            make_uint2(fl_pack_bf16(acc[mt][h2][4 * q4] * inv, acc[mt][h2][4 * q4 + 1] * inv),
                       fl_pack_bf16(acc[mt][h2][4 * q4 + 2] * inv, acc[mt][h2][4 * q4 + 3] * inv));
  }
}

}  // namespace

extern "C" int fl_mla_prefill_paged_bf16(const FlMlaPrefillArgs* a, fl_stream_t stream) {
  FL_CHECK_ARG(a != nullptr, "fl_mla_prefill_paged_bf16: null argument struct");
  FL_CHECK_ARG(a->struct_bytes == (int32_t)sizeof(FlMlaPrefillArgs),
               "fl_mla_prefill_paged_bf16: struct_bytes = %d, this library's FlMlaPrefillArgs has %d (caller built against another header)",
               (int)a->struct_bytes, (int)sizeof(FlMlaPrefillArgs));
  FL_CHECK_ARG(a->head_dim_ckv == 512 && a->head_dim_kpe == 64,
               "fl_mla_prefill_paged_bf16: only head_dim_ckv=512, head_dim_kpe=64 (got %d, %d)", a->head_dim_ckv, a->head_dim_kpe);
  const long long lim = (1ll << 31) - 256;
  FL_CHECK_ARG(a->batch >= 0 && a->num_heads >= 1 && a->num_q_tokens >= 0 && a->num_kv_slots >= 0 && a->num_kv_indices >= 0 &&
                   a->num_q_tokens < lim && a->num_kv_slots < lim && a->num_kv_indices < lim && a->num_q_tokens * a->num_heads < lim,
               "fl_mla_prefill_paged_bf16: bad sizes (batch %d, tokens %lld, slots %lld, indices %lld, heads %d; tokens x heads must stay "
               "below 2^31)", a->batch, (long long)a->num_q_tokens, (long long)a->num_kv_slots, (long long)a->num_kv_indices, a->num_heads);
  if (a->batch == 0 || a->num_q_tokens == 0) return FL_OK;
  FL_CHECK_ARG(a->q_nope && a->q_pe && a->out && a->qo_indptr && a->kv_indptr && a->kv_len_arr &&
                   (a->num_kv_indices == 0 || a->kv_indices) && (a->num_kv_slots == 0 || (a->ckv && a->kpe)),
               "fl_mla_prefill_paged_bf16: null pointer");
  FL_CHECK_ARG(((uintptr_t)a->q_nope % 16) == 0 && ((uintptr_t)a->q_pe % 16) == 0 && ((uintptr_t)a->ckv % 16) == 0 &&
                   ((uintptr_t)a->kpe % 16) == 0 && ((uintptr_t)a->out % 16) == 0 && a->q_nope_stride_token % 8 == 0 &&
                   a->q_nope_stride_head % 8 == 0 && a->q_pe_stride_token % 8 == 0 && a->q_pe_stride_head % 8 == 0 &&
                   a->ckv_stride_slot % 8 == 0 && a->kpe_stride_slot % 8 == 0,
               "fl_mla_prefill_paged_bf16: q_nope / q_pe / ckv / kpe / out rows must be 16-byte aligned (pointers, and strides multiples of "
               "8 elements)");
  MpParams p;
  p.q_nope = (const uint16_t*)a->q_nope; p.q_pe = (const uint16_t*)a->q_pe;
  p.ckv = (const uint16_t*)a->ckv; p.kpe = (const uint16_t*)a->kpe;
  p.o = (uint16_t*)a->out; p.lse = a->lse;
  p.qo_indptr = a->qo_indptr; p.kv_indptr = a->kv_indptr; p.kv_indices = a->kv_indices; p.kv_len_arr = a->kv_len_arr;
  p.sqnt = a->q_nope_stride_token; p.sqnh = a->q_nope_stride_head; p.sqpt = a->q_pe_stride_token; p.sqph = a->q_pe_stride_head;
  p.sct = a->ckv_stride_slot; p.skt = a->kpe_stride_slot;
  p.B = a->batch; p.T = (int)a->num_q_tokens; p.N = (int)a->num_kv_slots; p.NI = (int)a->num_kv_indices; p.H = a->num_heads;
  p.causal = a->causal != 0;
  p.scale_log2e = a->sm_scale * kMpLog2e;
  // every request has at most ceil(len H / 64) <= len H / 64 + 1 row tiles
  const long long tiles = (a->num_q_tokens * a->num_heads + kMpRows - 1) / kMpRows + a->batch;
  FL_CHECK_ARG(tiles < (1ll << 31), "fl_mla_prefill_paged_bf16: grid too large");
  mla_prefill_bf16_kernel<<<dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream>>>(p);
  FL_CHECK_LAUNCH("mla_prefill_bf16_kernel");
  return FL_OK;
}
