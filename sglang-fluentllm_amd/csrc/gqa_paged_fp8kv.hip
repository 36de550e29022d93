// P3, fp8 KV — paged GQA attention over a token-indexed e4m3fn KV cache, head dim 128, bf16 q / o, ragged and causal, with a split over the
// KV for decode; gfx950 (MI355X) only.  The statement, the row space, the two forms, the split and its merge are those of
// gqa_paged_bf16.hip; what differs is everything that follows from a K / V row being 128 BYTES:
//     o = v_scale softmax_j(sm_scale k_scale q . K8[slot(j)] + mask) . V8[slot(.)],   lse = log2 sum_j 2^(sm_scale k_scale log2e q . K8)
//   k_scale is folded into scale_log2e on the host, v_scale into the final normaliser in fp32 (the split partials carry it: the merge kernel
//   is the bf16 path's).  K8 / V8 bytes are dequantised EXACTLY (every e4m3fn value is a bf16 value: v_cvt_pk_f32_fp8, v_cvt_pk_bf16_f32)
//   in registers into the same bf16 MFMAs with fp32 accumulation and bf16 P; neither Q nor P is quantised.  An fp8 NaN byte of a live
//   token propagates.
//
// LDS layout.  One row = 128 B = 8 chunks of 16 B (16 head dims), unpadded: two rows share one 256-byte bank period.  Gather by LDS-DMA
// (global_load_lds_dwordx4): a row is 8 lanes, a wave-wide piece brings EIGHT token rows.  Position p of tile row R holds source chunk
// p ^ sw(R),   sw(R) = R[2] | R[1] << 1 | (R[3] ^ R[4]) << 2   (R[i] = bit i of the tile row).  Derived, not counted (no counter run):
//   * K fragment (ds_read_b128, 16 consecutive aligned rows at one chunk): R[0] picks the half of the bank period, (R[1], R[2], R[3]) map
//     one-to-one onto the three position bits -> 16 different 16-B bank groups.
//   * V^T (ds_read_b64_tr_b8; a 16-lane group reads 8 token rows x 16 B, lane pairs share a 16-B group), taken as two phases of 32 lanes:
//     decode form — rows {4 g .. 4 g + 3} + {0, 16} of g = 0, 1 (2, 3) at one chunk: (R[1], R[2], R[4]) vary, R[3] is fixed -> 16 different
//     groups.  Row form — rows 16 ks + 4 lh + {0 .. 3, 8 .. 11} at chunks 2 mt, 2 mt + 1: (R[1], R[3]) map onto position bits 1, 2 and the
//     chunk's bit 0 stays free -> 16 different groups.
//   What remains: the two 8-byte halves of a 16-B group are read by neighbouring lanes (same group, different banks: no conflict), and the
//   phase split of the transpose read is an assumption.
// Tile rows past the range a workgroup fetches repeat its last fetched token (their P is exactly 0): LDS never holds bytes of a slot that
// no request owns.
//
// Operand layouts.  The head dims of Q and K are permuted alike (a dot product does not care): one ds_read_b128 of a K row = 16 dims feeds
// TWO k-steps (bytes 0 .. 7 and 8 .. 15), and Q is loaded from global memory in the matching order.
//   * Decode form: 128-token tiles (16 KiB K + 16 KiB V per buffer, two buffers, 64 KiB, two workgroups per CU — the bf16 kernel's bytes in
//     flight).  Wave w gathers and consumes tile rows 32 w .. 32 w + 31 (4 K + 4 V pieces): no barrier in the tile loop.  Two 16-token groups
//     u = 0, 1 give two independent chains S_u^T[16 tok x 16 rows] = K . Q^T on v_mfma_f32_16x16x32_bf16: lane (n16, g) reads chunk 4 i + g
//     (i = 0, 1) of row 16 u + n16, k-step 2 i + h = its byte half h.  A lane then holds tokens 16 u + 4 g + r (r = 0 .. 3) of query row n16:
//     its EIGHT P values are the B operand of ONE v_mfma_f32_16x16x32_bf16 per 16-dim tile, O^T[16 dims x 16 rows] += V^T . P^T with
//     k = 8 g + e <-> token 16 (e >> 2) + 4 g + (e & 3); the transpose read delivers exactly those 8 tokens (source lane s16 of group g points
//     at token j = s16 >> 1, half s16 & 1).  Per wave and 32 tokens: 4 ds_read_b128 + 8 ds_read_b64_tr_b8, 8 + 8 MFMAs, 128 conversion VALU.
//   * Row form: 64-token tiles (8 + 8 KiB, two buffers, 32 KiB), wave w gathers rows 16 w .. + 15 (2 + 2 pieces), one barrier per tile.
//     S^T[64 tok x 32 rows] on v_mfma_f32_32x32x16_bf16: lane (li, lh) reads chunk 2 i + lh (i = 0 .. 3) of rows li and 32 + li, k-step
//     2 i + h = byte half h.  O^T[128 dims x 32 rows] += V^T . P^T: ONE transpose read is the whole 8-token A operand of a 32x32x16 MFMA
//     (lane group (lh, b16): tokens 16 ks + 4 lh + {0 .. 3, 8 .. 11} — the token permutation of the score registers — at chunk 2 mt + b16).
//     Every wave dequantises the fragments it reads (8 ds_read_b128 + 16 ds_read_b64_tr_b8, 32 MFMAs, 256 conversion VALU per tile): the
//     conversion is repeated in the four waves instead of paying a second barrier or 96 KiB for a shared bf16 tile.
// No host synchronisation, no allocation: hipGraph-capturable; a replay sees new contents of the same index buffers.
#include "fl_common.h"

namespace {

#include "gqa_paged_shared.h"   // GqParams, the lane-swap reductions, gq_decode_tokens, gqa_split_merge_kernel

constexpr int kG8Rows = 128;                   // row form: rows per workgroup, 32 per wave
constexpr int kG8RowB = 128;                   // one K or V row in LDS (swizzled, unpadded)
constexpr int kG8OffM = 4 * 32 * 64 * 4;       // decode combine (overlays the tile buffers): f32 [4 waves][32 regs][64 lanes], then max, sum
template <bool kDecode>
struct G8 {
  static constexpr int kTile = kDecode ? 128 : 64;   // KV tokens per tile
  static constexpr int kWave = kTile / 4;            // tile rows a wave gathers
  static constexpr int kOffV = kTile * kG8RowB;      // V follows K
  static constexpr int kBuf = 2 * kOffV;
  static constexpr int kLds = 2 * kBuf;              // 65,536 / 32,768 B
};
static_assert(2 * G8<true>::kLds <= 160 * 1024, "two workgroups per CU");
static_assert(kG8OffM + 2 * 4 * 16 * 4 <= G8<true>::kLds, "the combine area fits in the tile buffers");

__device__ __forceinline__ int g8_sw(const int r) { return ((r >> 2) & 1) | (r & 2) | ((((r >> 3) ^ (r >> 4)) & 1) << 2); }
// eight e4m3fn bytes -> eight bf16, exact; element e = byte e
__device__ __forceinline__ uint2 g8_cvt4(const int w) {
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
  const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  return make_uint2(fl_pack_bf16(lo[0], lo[1]), fl_pack_bf16(hi[0], hi[1]));
}
__device__ __forceinline__ v8bf g8_cvt8(const int w0, const int w1) {
  const uint2 a = g8_cvt4(w0), b = g8_cvt4(w1);
  return gq_as_v8bf(make_uint4(a.x, a.y, b.x, b.y));
}
__device__ __forceinline__ v8bf g8_vt(const uint8_t* src) {   // V^T operand: 8 tokens of one dim
  const v2i t = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i*)src);
  return g8_cvt8(t[0], t[1]);
}

template <bool kDecode>
__global__ __launch_bounds__(256, 2) void gqa_paged_fp8kv_kernel(const GqParams p, const float v_scale) {
  using C = G8<kDecode>;
  constexpr int kTile = C::kTile, kWave = C::kWave, kOffV = C::kOffV, kBuf = C::kBuf;
  __shared__ __attribute__((aligned(1024))) uint8_t smem[C::kLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;    // row form: query row of the wave, token half
  const int n16 = lane & 15, g = lane >> 4;    // decode form: query row, token quarter of a 16-token group
  const int hk = blockIdx.y;
  const uint8_t* const k8 = reinterpret_cast<const uint8_t*>(p.k);
  const uint8_t* const v8 = reinterpret_cast<const uint8_t*>(p.v);

  // ---- (request, row tile) of this workgroup ----
  int req = -1, rt = 0, q_beg = 0, q_len = 0;
  if constexpr (kDecode) {
    req = blockIdx.x;
    gq_decode_tokens(p, req, q_beg, q_len);
    if (q_len == 0) return;
  } else {   // last row tile of the last request first
    int x = blockIdx.x;
    for (int b = p.B - 1; b >= 0; --b) {
      const int beg = gq_clamp(p.qo_indptr[b], p.T), end = gq_clamp(p.qo_indptr[b + 1], p.T);
      const int len = end > beg ? end - beg : 0;
      const int nt = (len * p.G + kG8Rows - 1) / kG8Rows;
      if (x < nt) {
        req = b; rt = nt - 1 - x; q_beg = beg; q_len = len;
        break;
      }
      x -= nt;
    }
    if (req < 0) return;   // surplus workgroup
  }
  const int kv_beg = gq_clamp(p.kv_indptr[req], p.NI);
  int kv_len = gq_clamp(p.kv_indptr[req + 1], p.NI) - kv_beg;
  kv_len = (kv_len > 0 && p.N > 0) ? kv_len : 0;
  const int off = kv_len - q_len;   // token i sees keys j <= i + off (causal)
  const int nrows = q_len * p.G;    // >= 1
  auto vis = [&](const int i) {     // visible key range [0, end) of query token i
    const int e = p.causal ? (i + off + 1 < kv_len ? i + off + 1 : kv_len) : kv_len;
    return e > 0 ? e : 0;
  };

  // keys [f_lo, f_hi) are fetched by this workgroup (f_lo tile-aligned); this lane's row sees [.., lim), every row of the wave [.., w_full),
  // some row of the wave [.., w_end)
  int f_lo = 0, f_hi, w_end, w_full, row, lim;
  if constexpr (kDecode) {
    const int per = ((kv_len + p.S - 1) / p.S + kTile - 1) / kTile * kTile;
    f_lo = (int)blockIdx.z * per;   // <= kv_len + 16 * 128: no overflow
    f_hi = f_lo + per < kv_len ? f_lo + per : kv_len;
    row = n16;
    w_end = f_hi;   // the last token sees every key
    w_full = vis(0) < f_hi ? vis(0) : f_hi;
  } else {
    const int r0 = rt * kG8Rows;
    f_hi = vis((r0 + kG8Rows - 1 < nrows - 1 ? r0 + kG8Rows - 1 : nrows - 1) / p.G);
    const int w_first = r0 + 32 * wave;
    const bool w_any = w_first < nrows;
    w_end = w_any ? vis((w_first + 31 < nrows - 1 ? w_first + 31 : nrows - 1) / p.G) : 0;
    w_full = w_any ? vis(w_first / p.G) : 0;
    row = w_first + li;
  }
  const int rowc = row < nrows ? row : nrows - 1;   // (clamped loads; the tail rows are not stored)
  const int ti = rowc / p.G, hq = hk * p.G + (rowc - ti * p.G);
  lim = vis(ti) < f_hi ? vis(ti) : f_hi;
  const int t_beg = f_lo / kTile, t_end = f_hi > f_lo ? (f_hi + kTile - 1) / kTile : t_beg;   // an empty slice has no tile

  // ---- Q fragment, B operand of S^T = K . Q^T, in the dim order of the K reads: k-step 2 i + h holds dims 16 c + 8 h .. + 7 of the chunk
  //      c the lane reads from a K row — row form c = 2 i + lh (i = 0 .. 3), decode form c = 4 i + g (i = 0, 1) ----
  constexpr int kQSteps = kDecode ? 4 : 8;
  v8bf qf[kQSteps];
  {
    const uint16_t* qp = p.q + (long long)(q_beg + ti) * p.sqt + (long long)hq * p.sqh + (kDecode ? 16 * g : 16 * lh);
#pragma unroll
    for (int s = 0; s < kQSteps; ++s)
      qf[s] = gq_as_v8bf(*reinterpret_cast<const uint4*>(qp + (kDecode ? 64 : 32) * (s >> 1) + 8 * (s & 1)));
  }

  // ---- gather of a KV tile: wave w brings tile rows kWave w .. + kWave - 1; lane l holds the (clamped) slot of row kWave w + (l % kWave) ----
  auto load_slot = [&](const int t) {
    int tok = t * kTile + kWave * wave + (lane & (kWave - 1));
    tok = tok < f_hi ? tok : f_hi - 1;   // f_hi >= 1 wherever a tile is fetched
    const int s = p.kv_indices ? p.kv_indices[kv_beg + tok] : kv_beg + tok;
    return gq_clamp(s, p.N - 1);
  };
  auto issue = [&](const int t, const int slotv) {
    uint8_t* buf = smem + (t & 1) * kBuf + kWave * wave * kG8RowB;
#pragma unroll
    for (int jj = 0; jj < kWave / 8; ++jj) {   // piece jj: tile rows kWave w + 8 jj + (lane >> 3), one 16-B chunk per lane
      const long long s = __shfl(slotv, 8 * jj + (lane >> 3));
      const int ch = (lane & 7) ^ g8_sw(kWave * wave + 8 * jj + (lane >> 3));
      fl_dma16(k8 + s * p.sks + (long long)hk * p.skh + 16 * ch, buf + 8 * jj * kG8RowB);
      fl_dma16(v8 + s * p.svs + (long long)hk * p.svh + 16 * ch, buf + kOffV + 8 * jj * kG8RowB);
    }
  };

  float m_run = -INFINITY, l_run = 0.f;   // l_run: this lane's share of the row sum (row form: a half, decode form: a quarter)
  int slot_next = 0;
  if (t_beg < t_end) {
    issue(t_beg, load_slot(t_beg));
    if (t_beg + 1 < t_end) slot_next = load_slot(t_beg + 1);
  }

  if constexpr (!kDecode) {
    v16f o[4];   // O^T: register r of tile mt = dim 32 mt + (r & 3) + 8 (r >> 2) + 4 lh of row li
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[mt][r] = 0.f;
    // K fragment of (sub-tile st, read i): tile row 32 st + li (sw does not see bit 5), chunk 2 i + lh; i enters by XOR
    const int k_off = li * kG8RowB + 16 * (lh ^ g8_sw(li));
    // V^T fragment of (k-step ks, dim tile mt): lane group (lh, b16) = lane >> 4, source lane s16 points at token j = s16 >> 1 of the group's
    // eight = tile row 16 ks + 4 lh + (j & 3) + 8 (j >> 2), chunk 2 mt + b16, byte half s16 & 1; mt and the parity of ks (bit 4 of the row:
    // bit 2 of sw) enter by XOR
    const int vj = (lane & 15) >> 1, vr = 4 * lh + (vj & 3) + 8 * (vj >> 2);
    const int v_off = kOffV + vr * kG8RowB + 16 * (((lane >> 4) & 1) ^ g8_sw(vr)) + 8 * (lane & 1);

    for (int t = t_beg; t < t_end; ++t) {
      const int t0 = t * kTile;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile t
      __syncthreads();   // tile t is in LDS; tile t - 1 has been read by every wave
      if (t + 1 < t_end) {
        issue(t + 1, slot_next);
        if (t + 2 < t_end) slot_next = load_slot(t + 2);
      }
      if (t0 >= w_end) continue;   // wholly above this wave's rows (wave-uniform)
      const uint8_t* kb = smem + (t & 1) * kBuf;

      // ---- S^T[64 tok x 32 rows] = K . Q^T: two 32-token sub-tiles, two independent MFMA chains; one read = two k-steps ----
      v16f sc[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[0][r] = sc[1][r] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint8_t* ka = kb + (k_off ^ (32 * i));
        const uint4 a0 = *reinterpret_cast<const uint4*>(ka);
        const uint4 a1 = *reinterpret_cast<const uint4*>(ka + 32 * kG8RowB);
        sc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g8_cvt8(a0.x, a0.y), qf[2 * i], sc[0], 0, 0, 0);
        sc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g8_cvt8(a1.x, a1.y), qf[2 * i], sc[1], 0, 0, 0);
        sc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g8_cvt8(a0.z, a0.w), qf[2 * i + 1], sc[0], 0, 0, 0);
        sc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g8_cvt8(a1.z, a1.w), qf[2 * i + 1], sc[1], 0, 0, 0);
      }
      // register r of sub-tile st = token t0 + 32 st + (r & 3) + 8 (r >> 2) + 4 lh of query row li
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[st][r] *= p.scale_log2e;
      if (t0 + kTile > w_full) {   // the tile crosses a row's causal limit or the end of the KV
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
      mx = gq_pair_max(mx);
      const float m_new = fmaxf(m_run, mx);
      const float m_safe = m_new == -INFINITY ? 0.f : m_new;   // a row that has seen no key yet: every weight 2^(-inf) = 0, no NaN
      const float alpha = m_new == m_run ? 1.f : __builtin_amdgcn_exp2f(m_run - m_safe);
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
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[mt][r] *= alpha;
      }
      // ---- O^T += V^T . P^T: k-step ks = tokens 16 ks .. + 15 = score registers 8 (ks & 1) .. + 7 of sub-tile ks >> 1, under the token
      //      permutation k = 8 lh + e <-> token 16 ks + (e & 3) + 8 (e >> 2) + 4 lh ----
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        union { uint4 u; v8bf v; } pb;
        const int st = ks >> 1, rb = 8 * (ks & 1);
        pb.u = make_uint4(fl_pack_bf16(sc[st][rb], sc[st][rb + 1]), fl_pack_bf16(sc[st][rb + 2], sc[st][rb + 3]),
                          fl_pack_bf16(sc[st][rb + 4], sc[st][rb + 5]), fl_pack_bf16(sc[st][rb + 6], sc[st][rb + 7]));
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g8_vt(kb + (v_off ^ (32 * mt) ^ (64 * (ks & 1))) + 16 * ks * kG8RowB), pb.v,
                                                          o[mt], 0, 0, 0);
      }
    }

    // ---- epilogue: the two halves of the row sum meet, normalise (v_scale rides on the normaliser), store ----
    const float l_tot = gq_pair_sum(l_run);
    if (row >= nrows) return;
    const float inv = l_tot > 0.f ? v_scale / l_tot : 0.f;
    const long long orow = (long long)(q_beg + ti) * p.Hq + hq;
    if (p.lse != nullptr && lh == 0) p.lse[orow] = l_tot > 0.f ? m_run + __builtin_amdgcn_logf(l_tot) : -INFINITY;
    uint16_t* op = p.o + orow * 128 + 4 * lh;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4)
        *reinterpret_cast<uint2*>(op + 32 * mt + 8 * q4) = make_uint2(fl_pack_bf16(o[mt][4 * q4] * inv, o[mt][4 * q4 + 1] * inv),
                                                                      fl_pack_bf16(o[mt][4 * q4 + 2] * inv, o[mt][4 * q4 + 3] * inv));
  } else {
    v4f o[8];   // O^T: register r of tile dt = dim 16 dt + 4 g + r of row n16, over THIS wave's tokens
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[dt] = v4f{0.f, 0.f, 0.f, 0.f};
    // K fragment of (group u, read i): tile row 32 w + 16 u + n16 (sw does not see 32 w), chunk 4 i + g; i enters by XOR
    int k_off[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) k_off[u] = (32 * wave + 16 * u + n16) * kG8RowB + 16 * (g ^ g8_sw(16 * u + n16));
    // V^T fragment of dim tile dt: source lane s16 = n16 of group g points at token j = s16 >> 1 of the group's eight = tile row
    // 32 w + 4 g + (j & 3) + 16 (j >> 2), chunk dt (by XOR), byte half s16 & 1
    const int vj = n16 >> 1, vr = 4 * g + (vj & 3) + 16 * (vj >> 2);
    const int v_off = kOffV + (32 * wave + vr) * kG8RowB + 16 * g8_sw(vr) + 8 * (n16 & 1);

    for (int t = t_beg; t < t_end; ++t) {
      const int tb = t * kTile + 32 * wave;   // this wave's 32 tokens: the rows it gathered itself — no barrier
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (t + 1 < t_end) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads of tile t - 1 have left the buffer tile t + 1 lands in
        issue(t + 1, slot_next);
        if (t + 2 < t_end) slot_next = load_slot(t + 2);
      }
      if (tb >= w_end) continue;   // (wave-uniform)
      const uint8_t* kb = smem + (t & 1) * kBuf;

      // ---- S_u^T[16 tok x 16 rows] = K . Q^T, u = 0, 1; register r of group u = token tb + 16 u + 4 g + r of query row n16 ----
      v4f sc[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint4 a0 = *reinterpret_cast<const uint4*>(kb + (k_off[0] ^ (64 * i)));
        const uint4 a1 = *reinterpret_cast<const uint4*>(kb + (k_off[1] ^ (64 * i)));
        sc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g8_cvt8(a0.x, a0.y), qf[2 * i], sc[0], 0, 0, 0);
        sc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g8_cvt8(a1.x, a1.y), qf[2 * i], sc[1], 0, 0, 0);
        sc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g8_cvt8(a0.z, a0.w), qf[2 * i + 1], sc[0], 0, 0, 0);
        sc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g8_cvt8(a1.z, a1.w), qf[2 * i + 1], sc[1], 0, 0, 0);
      }
      float y[8];   // y[4 u + r]
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = sc[e >> 2][e & 3] * p.scale_log2e;
      if (tb + 32 > w_full) {   // crosses a row's causal limit or the end of the slice
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (tb + 16 * (e >> 2) + 4 * g + (e & 3) >= lim) y[e] = -INFINITY;
      }
      const float mx = gq_quad_max(fmaxf(fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3])), fmaxf(fmaxf(y[4], y[5]), fmaxf(y[6], y[7]))));
      const float m_new = fmaxf(m_run, mx);
      const float m_safe = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = m_new == m_run ? 1.f : __builtin_amdgcn_exp2f(m_run - m_safe);
      m_run = m_new;
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = __builtin_amdgcn_exp2f(y[e] - m_safe);
      l_run = l_run * alpha + (((y[0] + y[1]) + (y[2] + y[3])) + ((y[4] + y[5]) + (y[6] + y[7])));
      if (__any(alpha != 1.f)) {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[dt] *= alpha;
      }
      // ---- O^T[16 dims x 16 rows] += V^T . P^T on 16x16x32: the lane's eight P values ARE its B operand (k = 8 g + e) ----
      union { uint4 u; v8bf v; } pb;
      pb.u = make_uint4(fl_pack_bf16(y[0], y[1]), fl_pack_bf16(y[2], y[3]), fl_pack_bf16(y[4], y[5]), fl_pack_bf16(y[6], y[7]));
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g8_vt(kb + (v_off ^ (16 * dt))), pb.v, o[dt], 0, 0, 0);
    }

    // ---- combine the four waves' states through LDS; wave w finishes dim tiles 2 w, 2 w + 1 ----
    const float l_wave = gq_quad_sum(l_run);
    __syncthreads();   // every wave has left the tile buffers
    float* const part = reinterpret_cast<float*>(smem);
    float* const m_s = reinterpret_cast<float*>(smem + kG8OffM);
    float* const l_s = m_s + 4 * 16;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(wave * 32 + 4 * dt + r) * 64 + lane] = o[dt][r];
    if (g == 0) {
      m_s[16 * wave + n16] = m_run;
      l_s[16 * wave + n16] = l_wave;
    }
    __syncthreads();
    if (row >= nrows) return;
    float mw[4], m_all = -INFINITY, l_all = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) m_all = fmaxf(m_all, m_s[16 * w + n16]);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float mv = m_s[16 * w + n16];
      mw[w] = mv == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mv - m_all);
      l_all += mw[w] * l_s[16 * w + n16];
    }
    const float inv = l_all > 0.f ? v_scale / l_all : 0.f;   // (a split partial carries v_scale: the merge is the bf16 path's)
    const float lse = l_all > 0.f ? m_all + __builtin_amdgcn_logf(l_all) : -INFINITY;
    const long long orow = (long long)(q_beg + ti) * p.Hq + hq;
    const long long prow = (long long)blockIdx.z * p.T * p.Hq + orow;
    if (wave == 0 && g == 0) {
      if (p.S > 1) p.part_lse[prow] = lse;
      else if (p.lse != nullptr) p.lse[orow] = lse;
    }
#pragma unroll
    for (int d2 = 0; d2 < 2; ++d2) {
      const int dt = 2 * wave + d2;
      float x[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) acc += mw[w] != 0.f ? mw[w] * part[(w * 32 + 4 * dt + r) * 64 + lane] : 0.f;
        x[r] = acc * inv;
      }
      if (p.S > 1)
        *reinterpret_cast<float4*>(p.part_o + prow * 128 + 16 * dt + 4 * g) = make_float4(x[0], x[1], x[2], x[3]);
      else
        *reinterpret_cast<uint2*>(p.o + orow * 128 + 16 * dt + 4 * g) = make_uint2(fl_pack_bf16(x[0], x[1]), fl_pack_bf16(x[2], x[3]));
    }
  }
}

}  // namespace

#define G8_NAME "fl_gqa_paged_attention_fp8kv"
extern "C" int fl_gqa_paged_attention_fp8kv(const FlGqaPagedArgs* a, float k_scale, float v_scale, fl_stream_t stream) {
  FL_CHECK_ARG(a != nullptr, G8_NAME ": null argument struct");
  FL_CHECK_ARG(a->struct_bytes == (int32_t)sizeof(FlGqaPagedArgs),
               G8_NAME ": struct_bytes = %d, this library's FlGqaPagedArgs has %d (caller built against another header)",
               (int)a->struct_bytes, (int)sizeof(FlGqaPagedArgs));
  FL_CHECK_ARG(a->head_dim == 128, G8_NAME ": only head_dim=128 (got %d)", a->head_dim);
  FL_CHECK_ARG(k_scale > 0.f && k_scale <= 3.0e38f && v_scale > 0.f && v_scale <= 3.0e38f,
               G8_NAME ": k_scale = %g, v_scale = %g; both must be finite and positive", (double)k_scale, (double)v_scale);
  const long long lim = (1ll << 31) - 256;
  FL_CHECK_ARG(a->batch >= 0 && a->num_kv_heads >= 1 && a->num_kv_heads <= 65535 && a->num_qo_heads >= 1 &&
                   a->num_qo_heads % a->num_kv_heads == 0 && a->num_q_tokens >= 0 && a->num_kv_slots >= 0 && a->num_kv_indices >= 0 &&
                   a->num_q_tokens < lim && a->num_kv_slots < lim && a->num_kv_indices < lim && a->num_q_tokens * a->num_qo_heads < lim,
               G8_NAME ": bad sizes (batch %d, tokens %lld, slots %lld, indices %lld, heads %d / %d; the query heads must "
               "be a multiple of the KV heads and tokens x heads stay below 2^31)", a->batch, (long long)a->num_q_tokens,
               (long long)a->num_kv_slots, (long long)a->num_kv_indices, a->num_qo_heads, a->num_kv_heads);
  const int G = a->num_qo_heads / a->num_kv_heads;
  const bool dec = a->decode_form != 0;
  FL_CHECK_ARG(a->decode_form == 0 || a->decode_form == 1, G8_NAME ": decode_form = %d", a->decode_form);
  FL_CHECK_ARG(dec ? (a->num_splits >= 1 && a->num_splits <= kGqMaxSplits && G <= kGqDecRows) : a->num_splits == 1,
               G8_NAME ": num_splits = %d (decode form: 1 .. %d and a group of at most %d heads, got %d; row form: 1)",
               a->num_splits, kGqMaxSplits, kGqDecRows, G);
  FL_CHECK_ARG(dec || a->qo_indptr != nullptr, G8_NAME ": the row form needs qo_indptr");
  FL_CHECK_ARG(a->qo_indptr != nullptr || a->num_q_tokens == a->batch,
               G8_NAME ": without qo_indptr every request has one query token (tokens %lld, batch %d)",
               (long long)a->num_q_tokens, a->batch);
  FL_CHECK_ARG(a->kv_indices != nullptr || a->num_kv_indices == a->num_kv_slots,
               G8_NAME ": without kv_indices num_kv_indices must equal num_kv_slots");
  if (a->batch == 0 || a->num_q_tokens == 0) return FL_OK;
  FL_CHECK_ARG(a->q && a->out && a->kv_indptr && (a->num_kv_slots == 0 || (a->k && a->v)), G8_NAME ": null pointer");
  FL_CHECK_ARG(((uintptr_t)a->q % 16) == 0 && ((uintptr_t)a->k % 16) == 0 && ((uintptr_t)a->v % 16) == 0 && ((uintptr_t)a->out % 16) == 0 &&
                   a->q_stride_token % 8 == 0 && a->q_stride_head % 8 == 0 && a->k_stride_slot % 16 == 0 && a->k_stride_head % 16 == 0 &&
                   a->v_stride_slot % 16 == 0 && a->v_stride_head % 16 == 0,
               G8_NAME ": q / k / v / out rows must be 16-byte aligned (pointers; q strides multiples of 8 elements, k / v strides "
               "multiples of 16 bytes)");
  GqParams p;
  p.q = (const uint16_t*)a->q; p.k = (const uint16_t*)a->k; p.v = (const uint16_t*)a->v;
  p.o = (uint16_t*)a->out; p.lse = a->lse;
  p.part_o = nullptr; p.part_lse = nullptr;
  p.qo_indptr = a->qo_indptr; p.kv_indptr = a->kv_indptr; p.kv_indices = a->kv_indices;
  p.sqt = a->q_stride_token; p.sqh = a->q_stride_head; p.sks = a->k_stride_slot; p.skh = a->k_stride_head;
  p.svs = a->v_stride_slot; p.svh = a->v_stride_head;
  p.B = a->batch; p.T = (int)a->num_q_tokens; p.N = (int)a->num_kv_slots; p.NI = (int)a->num_kv_indices;
  p.Hq = a->num_qo_heads; p.G = G; p.S = a->num_splits; p.causal = a->causal != 0;
  p.scale_log2e = a->sm_scale * k_scale * kGqLog2e;
  const hipStream_t st = (hipStream_t)stream;
  if (dec) {
    if (p.S > 1) {
      const long long rows = (long long)p.S * a->num_q_tokens * a->num_qo_heads;
      FL_CHECK_ARG(a->workspace != nullptr && ((uintptr_t)a->workspace % 16) == 0 && a->workspace_bytes >= rows * 129 * 4,
                   G8_NAME ": %d splits need a 16-byte aligned workspace of %lld bytes (got %lld)", p.S, rows * 129 * 4,
                   (long long)a->workspace_bytes);
      p.part_o = (float*)a->workspace;
      p.part_lse = p.part_o + rows * 128;
    }
    const dim3 grid((unsigned)a->batch, (unsigned)a->num_kv_heads, (unsigned)p.S);
    gqa_paged_fp8kv_kernel<true><<<grid, dim3(256), 0, st>>>(p, v_scale);
    FL_CHECK_LAUNCH("gqa_paged_fp8kv_kernel<decode>");
    if (p.S > 1) {
      gqa_split_merge_kernel<<<dim3((unsigned)a->batch, (unsigned)a->num_kv_heads), dim3(256), 0, st>>>(p);
      FL_CHECK_LAUNCH("gqa_split_merge_kernel");
    }
  } else {
    // every request has at most ceil(len G / 128) <= len G / 128 + 1 row tiles
    const long long tiles = (a->num_q_tokens * G + kG8Rows - 1) / kG8Rows + a->batch;
    FL_CHECK_ARG(tiles < (1ll << 31), G8_NAME ": grid too large");
    gqa_paged_fp8kv_kernel<false><<<dim3((unsigned)tiles, (unsigned)a->num_kv_heads), dim3(256), 0, st>>>(p, v_scale);
    FL_CHECK_LAUNCH("gqa_paged_fp8kv_kernel<row>");
  }
  return FL_OK;
}
