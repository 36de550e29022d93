// P3 — paged GQA attention over token-indexed KV, head dim 128, bf16, ragged and causal, with a split over the KV for decode; gfx950
// (MI355X) only.
//
// Replaces flashinfer.BatchDecodeWithPagedKVCacheWrapper / BatchPrefillWithPagedKVCacheWrapper (page size 1) and, through the identity-index
// mode, BatchPrefillWithRaggedKVCacheWrapper at 128/128, as the GQA models' default attention backend calls them
// (srt/layers/attention/flashinfer_backend.py):
//   per request b, query token i, query head h (KV head hk = h / G, G = Hq / Hkv), key j:  slot(j) = kv_indices[kv_indptr[b] + j],
//   or kv_indptr[b] + j itself when kv_indices is null (the ragged form: same kernel, address arithmetic instead of the index read)
//     s[i, h, j] = sm_scale * q[i, h, :] . k[slot(j), hk, :],   o[i, h, :] = softmax_j(s + mask) . v[slot(.), hk, :]
//     lse[i, h] = log2 sum_j 2^(s * log2 e)   (BASE 2, the base fl_merge_state reads)
//   causal, bottom-right aligned: token i sees j <= i + kv_len - q_len;  a row that sees no key: o = 0, lse = -inf;  query rows of no
//   request stay unwritten;  slot indices are clamped into [0, N).
//
// Row space.  For one (request, KV head) the rows are flattened as r = i * G + g: all G heads of a group share ONE pass over that KV
// head's K / V bytes; the causal limit is per row from r / G.
//
// KV tiles.  A tile = 64 tokens of one KV head = K 16 KiB + V 16 KiB, gathered by LDS-DMA (global_load_lds_dwordx4): one 256-byte row is
// 16 lanes, a wave-wide piece brings four token rows, wave w brings tile rows 16 w .. 16 w + 15 of K and of V (8 pieces), whose slot
// indices it read one tile ahead.  Two tile buffers (64 KiB): the pieces of tile t + 1 are in flight under all of tile t.  A DMA lane
// lands at (base + 16 lane) but fetches from ANY address, so the swizzle is free: position p of tile row j holds source chunk
// p ^ sw(j), sw(j) = 4 (j & 3) + ((j >> 2) & 3) — 16 consecutive rows of a K-fragment read (ds_read_b128, one column) start in 16
// different 16-B bank groups, and the 4 tokens of a V^T read (ds_read_b64_tr_b16) sit in the four 64-B quarters of the bank period.
// Tile rows past the range a workgroup fetches repeat its last fetched token (their P is exactly 0): LDS never holds bytes of a slot
// that no request owns, so 0 x NaN cannot arise from unwritten pool rows.
//
// Two forms of one template.
//   * Row form (prompts, extend over a prefix, verify with many rows): workgroup = 4 waves = 128 rows, 32 per wave.  Grid =
//     (ceil(T G / 128) + B, Hkv); a workgroup finds its (request, row tile) by a scan of qo_indptr from the last row tile of the last
//     request backwards, surplus workgroups exit.  S^T[64 tok x 32 rows] = K . Q^T on v_mfma_f32_32x32x16_bf16 with the wave's Q fragment
//     (8 k-steps, 32 VGPRs) resident; a lane owns 32 scores of ONE row: online softmax in registers (base 2, fp32 statistics), P rounded
//     to bf16 feeds O^T[128 dims x 32 rows] += V^T . P^T straight from the score registers (the token permutation of
//     mha_prefill_bf16.hip); O is 64 registers.  No P exchange through LDS: the only barrier is the tile hand-over, one per tile.
//   * Decode form (rows per (request, KV head) <= 16: decode at any G <= 16, verify with q_len G <= 16): the rows cannot fill a workgroup,
//     so the waves split the TOKENS of a tile, 16 each — exactly the rows the wave gathered itself, so the tile loop has no barrier at all.
//     S^T[16 tok x 16 rows] = K . Q^T on v_mfma_f32_16x16x32_bf16 (K is the 16-token operand); a lane holds 4 tokens of one row, which IS
//     the B operand of v_mfma_f32_16x16x16_bf16 for O^T[16 dims x 16 rows] += V^T . P^T (8 dim tiles, 32 registers), V^T again by
//     ds_read_b64_tr_b16.  Each wave keeps its own (max, sum, O partial); one LDS combine at the end of the workgroup's KV range.
//     Split over the KV: grid = (B, Hkv, S), split s takes the tile-aligned slice of ceil(kv_len / S) tokens (computed on the device) and,
//     when S > 1, writes a normalised partial (o f32, lse) to the workspace; gqa_split_merge_kernel merges the S partials per row in slice
//     order (deterministic; an empty slice has lse = -inf and is skipped).  No spin-waits, no tickets.
// No host synchronisation, no allocation: hipGraph-capturable; a replay sees new contents of the same index buffers.
#include "fl_common.h"

namespace {

#include "gqa_paged_shared.h"   // GqParams, the lane-swap reductions, gq_decode_tokens, gqa_split_merge_kernel

constexpr int kGqRows = 128;                   // row form: rows per workgroup, 32 per wave
constexpr int kGqTile = 64;                    // KV tokens per tile
constexpr int kGqRowB = 256;                   // one K or V row in LDS (swizzled, unpadded)
constexpr int kGqOffV = kGqTile * kGqRowB;     // V follows K
constexpr int kGqBuf = 2 * kGqOffV;            // 32,768 B per tile buffer
constexpr int kGqLds = 2 * kGqBuf;             // 65,536 B
constexpr int kGqOffM = 4 * 32 * 64 * 4;       // decode combine (overlays the tile buffers): f32 [4 waves][32 regs][64 lanes], then max, sum
static_assert(2 * kGqLds <= 160 * 1024, "two workgroups per CU");
static_assert(kGqOffM + 2 * 4 * 16 * 4 <= kGqLds, "the combine area fits in the tile buffers");

template <bool kDecode>
__global__ __launch_bounds__(256, 2) void gqa_paged_bf16_kernel(const GqParams p) {
  __shared__ __attribute__((aligned(1024))) uint8_t smem[kGqLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;    // row form: query row of the wave, token half
  const int n16 = lane & 15, g = lane >> 4;    // decode form: query row, token quarter of the wave's 16 tokens
  const int hk = blockIdx.y;

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
      const int nt = (len * p.G + kGqRows - 1) / kGqRows;
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
    const int per = ((kv_len + p.S - 1) / p.S + kGqTile - 1) / kGqTile * kGqTile;
    f_lo = (int)blockIdx.z * per;   // <= kv_len + 16 * 64: no overflow
    f_hi = f_lo + per < kv_len ? f_lo + per : kv_len;
    row = n16;
    w_end = f_hi;   // the last token sees every key
    w_full = vis(0) < f_hi ? vis(0) : f_hi;
  } else {
    const int r0 = rt * kGqRows;
    f_hi = vis((r0 + kGqRows - 1 < nrows - 1 ? r0 + kGqRows - 1 : nrows - 1) / p.G);
    const int w_first = r0 + 32 * wave;
    const bool w_any = w_first < nrows;
    w_end = w_any ? vis((w_first + 31 < nrows - 1 ? w_first + 31 : nrows - 1) / p.G) : 0;
    w_full = w_any ? vis(w_first / p.G) : 0;
    row = w_first + li;
  }
  const int rowc = row < nrows ? row : nrows - 1;   // (clamped loads; the tail rows are not stored)
  const int ti = rowc / p.G, hq = hk * p.G + (rowc - ti * p.G);
  lim = vis(ti) < f_hi ? vis(ti) : f_hi;
  const int t_beg = f_lo / kGqTile, t_end = f_hi > f_lo ? (f_hi + kGqTile - 1) / kGqTile : t_beg;   // an empty slice has no tile

  // ---- Q fragment, B operand of S^T = K . Q^T.  Row form: lane (li, lh) holds q[row li][16 s + 8 lh .. + 7] of k-step s (8 steps);
  //      decode form: lane (n16, g) holds q[row n16][32 s + 8 g .. + 7] (4 steps) ----
  constexpr int kQSteps = kDecode ? 4 : 8;
  v8bf qf[kQSteps];
  {
    const uint16_t* qp = p.q + (long long)(q_beg + ti) * p.sqt + (long long)hq * p.sqh + (kDecode ? 8 * g : 8 * lh);
#pragma unroll
    for (int s = 0; s < kQSteps; ++s) qf[s] = gq_as_v8bf(*reinterpret_cast<const uint4*>(qp + (kDecode ? 32 : 16) * s));
  }

  // ---- gather of a KV tile: wave w brings tile rows 16 w .. 16 w + 15; lane l holds the (clamped) slot of row 16 w + (l & 15) ----
  auto load_slot = [&](const int t) {
    int tok = t * kGqTile + 16 * wave + (lane & 15);
    tok = tok < f_hi ? tok : f_hi - 1;   // f_hi >= 1 wherever a tile is fetched
    const int s = p.kv_indices ? p.kv_indices[kv_beg + tok] : kv_beg + tok;
    return gq_clamp(s, p.N - 1);
  };
  auto issue = [&](const int t, const int slotv) {
    uint8_t* buf = smem + (t & 1) * kGqBuf + 16 * wave * kGqRowB;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {   // piece jj: tile rows 16 w + 4 jj + (lane >> 4), swizzle 4 (lane >> 4) + jj
      const long long s = __shfl(slotv, 4 * jj + (lane >> 4));
      const int ch = (lane & 15) ^ (4 * (lane >> 4) + jj);
      fl_dma16(p.k + s * p.sks + (long long)hk * p.skh + 8 * ch, buf + 4 * jj * kGqRowB);
      fl_dma16(p.v + s * p.svs + (long long)hk * p.svh + 8 * ch, buf + kGqOffV + 4 * jj * kGqRowB);
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
    // K fragment of (sub-tile st, k-step s): tile row 32 st + li, chunk 2 s + lh at position (2 s + lh) ^ sw(li)
    const int k_off = li * kGqRowB + 16 * (lh ^ (4 * (li & 3) + ((li >> 2) & 3)));
    // V^T fragment by ds_read_b64_tr_b16: inside a 16-lane group source lane s16 points at token (s16 >> 2) and dims 4 (s16 & 3) .. + 3 of the
    // group's 16 dims; destination lane i receives dim i of tokens 0 .. 3.  Group (lh, b16): tokens 4 lh + .., dims 16 b16 + ..  Lane part of
    // the address of tile row 4 lh + k4 (swizzle 4 k4 + lh): the 32-dim tile mt and the token octet u (swizzle + 2 u) enter by XOR
    const int k4 = (lane & 15) >> 2;
    const int v_off = kGqOffV + (4 * lh + k4) * kGqRowB + 64 * k4 + 16 * ((2 * ((lane >> 4) & 1) + ((lane & 3) >> 1)) ^ lh) + 8 * (lane & 1);

    for (int t = t_beg; t < t_end; ++t) {
      const int t0 = t * kGqTile;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile t
      __syncthreads();   // tile t is in LDS; tile t - 1 has been read by every wave
      if (t + 1 < t_end) {
        issue(t + 1, slot_next);
        if (t + 2 < t_end) slot_next = load_slot(t + 2);
      }
      if (t0 >= w_end) continue;   // wholly above this wave's rows (wave-uniform)
      const uint8_t* kb = smem + (t & 1) * kGqBuf;

      // ---- S^T[64 tok x 32 rows] = K . Q^T: two 32-token sub-tiles, two independent MFMA chains ----
      v16f sc[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[0][r] = sc[1][r] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const uint8_t* ka = kb + (k_off ^ (32 * s));
        const v8bf a0 = gq_as_v8bf(*reinterpret_cast<const uint4*>(ka));
        const v8bf a1 = gq_as_v8bf(*reinterpret_cast<const uint4*>(ka + 32 * kGqRowB));
        sc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, qf[s], sc[0], 0, 0, 0);
        sc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, qf[s], sc[1], 0, 0, 0);
      }
      // register r of sub-tile st = token t0 + 32 st + (r & 3) + 8 (r >> 2) + 4 lh of query row li
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[st][r] *= p.scale_log2e;
      if (t0 + kGqTile > w_full) {   // the tile crosses a row's causal limit or the end of the KV
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
        for (int mt = 0; mt < 4; ++mt) {
          union { v8bf v; v4s hv[2]; } a;
#pragma unroll
          for (int u = 0; u < 2; ++u)   // elements 4 u .. 4 u + 3: tokens 16 ks + 8 u + 4 lh + (0 .. 3)
            a.hv[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) v4s*)(kb + (v_off ^ (64 * mt + 32 * u)) + (16 * ks + 8 * u) * kGqRowB));
          o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, pb.v, o[mt], 0, 0, 0);
        }
      }
    }

    // ---- epilogue: the two halves of the row sum meet, normalise, store ----
    const float l_tot = gq_pair_sum(l_run);
    if (row >= nrows) return;
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
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
    // K fragment of k-step s: tile row 16 w + n16, chunk 4 s + g at position (4 s + g) ^ sw(n16)
    const int k_off = (16 * wave + n16) * kGqRowB + 64 * (n16 & 3) + 16 * (g ^ ((n16 >> 2) & 3));
    // V^T fragment of dim tile dt: lane group g reads tokens 16 w + 4 g + (0 .. 3), source lane s16 = n16 points at token k4 = s16 >> 2
    // (swizzle 4 k4 + g) and dims 16 dt + 4 (s16 & 3) .. + 3 = chunk 2 dt + ((s16 & 3) >> 1); dt enters by XOR
    const int k4 = n16 >> 2;
    const int v_off = kGqOffV + (16 * wave + 4 * g + k4) * kGqRowB + 16 * (((n16 & 3) >> 1) ^ (4 * k4 + g)) + 8 * (n16 & 1);

    for (int t = t_beg; t < t_end; ++t) {
      const int tb = t * kGqTile + 16 * wave;   // this wave's 16 tokens: the rows it gathered itself — no barrier
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (t + 1 < t_end) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads of tile t - 1 have left the buffer tile t + 1 lands in
        issue(t + 1, slot_next);
        if (t + 2 < t_end) slot_next = load_slot(t + 2);
      }
      if (tb >= w_end) continue;   // (wave-uniform)
      const uint8_t* kb = smem + (t & 1) * kGqBuf;

      // ---- S^T[16 tok x 16 rows] = K . Q^T; register r = token tb + 4 g + r of query row n16 ----
      v4f sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s)
        sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gq_as_v8bf(*reinterpret_cast<const uint4*>(kb + (k_off ^ (64 * s)))), qf[s], sc, 0, 0, 0);
      float y[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = sc[r] * p.scale_log2e;
      if (tb + 16 > w_full) {   // crosses a row's causal limit or the end of the slice
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (tb + 4 * g + r >= lim) y[r] = -INFINITY;
      }
      const float mx = gq_quad_max(fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3])));
      const float m_new = fmaxf(m_run, mx);
      const float m_safe = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = m_new == m_run ? 1.f : __builtin_amdgcn_exp2f(m_run - m_safe);
      m_run = m_new;
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = __builtin_amdgcn_exp2f(y[r] - m_safe);
      l_run = l_run * alpha + ((y[0] + y[1]) + (y[2] + y[3]));
      if (__any(alpha != 1.f)) {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[dt] *= alpha;
      }
      // ---- O^T[16 dims x 16 rows] += V^T . P^T on 16x16x16: the lane's four P values ARE its B operand (k = 4 g + r) ----
      union { uint2 u; v4s v; } pb;
      pb.u = make_uint2(fl_pack_bf16(y[0], y[1]), fl_pack_bf16(y[2], y[3]));
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) {
        const v4s a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(kb + (v_off ^ (32 * dt))));
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, pb.v, o[dt], 0, 0, 0);
      }
    }

    // ---- combine the four waves' states through LDS; wave w finishes dim tiles 2 w, 2 w + 1 ----
    const float l_wave = gq_quad_sum(l_run);
    __syncthreads();   // every wave has left the tile buffers
    float* const part = reinterpret_cast<float*>(smem);
    float* const m_s = reinterpret_cast<float*>(smem + kGqOffM);
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
    const float inv = l_all > 0.f ? 1.f / l_all : 0.f;
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

extern "C" int fl_gqa_paged_attention_bf16(const FlGqaPagedArgs* a, fl_stream_t stream) {
  FL_CHECK_ARG(a != nullptr, "fl_gqa_paged_attention_bf16: null argument struct");
  FL_CHECK_ARG(a->struct_bytes == (int32_t)sizeof(FlGqaPagedArgs),
               "fl_gqa_paged_attention_bf16: struct_bytes = %d, this library's FlGqaPagedArgs has %d (caller built against another header)",
               (int)a->struct_bytes, (int)sizeof(FlGqaPagedArgs));
  FL_CHECK_ARG(a->head_dim == 128, "fl_gqa_paged_attention_bf16: only head_dim=128 (got %d)", a->head_dim);
  const long long lim = (1ll << 31) - 256;
  FL_CHECK_ARG(a->batch >= 0 && a->num_kv_heads >= 1 && a->num_kv_heads <= 65535 && a->num_qo_heads >= 1 &&
                   a->num_qo_heads % a->num_kv_heads == 0 && a->num_q_tokens >= 0 && a->num_kv_slots >= 0 && a->num_kv_indices >= 0 &&
                   a->num_q_tokens < lim && a->num_kv_slots < lim && a->num_kv_indices < lim && a->num_q_tokens * a->num_qo_heads < lim,
               "fl_gqa_paged_attention_bf16: bad sizes (batch %d, tokens %lld, slots %lld, indices %lld, heads %d / %d; the query heads must "
               "be a multiple of the KV heads and tokens x heads stay below 2^31)", a->batch, (long long)a->num_q_tokens,
               (long long)a->num_kv_slots, (long long)a->num_kv_indices, a->num_qo_heads, a->num_kv_heads);
  const int G = a->num_qo_heads / a->num_kv_heads;
  const bool dec = a->decode_form != 0;
  FL_CHECK_ARG(a->decode_form == 0 || a->decode_form == 1, "fl_gqa_paged_attention_bf16: decode_form = %d", a->decode_form);
  FL_CHECK_ARG(dec ? (a->num_splits >= 1 && a->num_splits <= kGqMaxSplits && G <= kGqDecRows) : a->num_splits == 1,
               "fl_gqa_paged_attention_bf16: num_splits = %d (decode form: 1 .. %d and a group of at most %d heads, got %d; row form: 1)",
               a->num_splits, kGqMaxSplits, kGqDecRows, G);
  FL_CHECK_ARG(dec || a->qo_indptr != nullptr, "fl_gqa_paged_attention_bf16: the row form needs qo_indptr");
  FL_CHECK_ARG(a->qo_indptr != nullptr || a->num_q_tokens == a->batch,
               "fl_gqa_paged_attention_bf16: without qo_indptr every request has one query token (tokens %lld, batch %d)",
               (long long)a->num_q_tokens, a->batch);
  FL_CHECK_ARG(a->kv_indices != nullptr || a->num_kv_indices == a->num_kv_slots,
               "fl_gqa_paged_attention_bf16: without kv_indices num_kv_indices must equal num_kv_slots");
  if (a->batch == 0 || a->num_q_tokens == 0) return FL_OK;
  FL_CHECK_ARG(a->q && a->out && a->kv_indptr && (a->num_kv_slots == 0 || (a->k && a->v)), "fl_gqa_paged_attention_bf16: null pointer");
  FL_CHECK_ARG(((uintptr_t)a->q % 16) == 0 && ((uintptr_t)a->k % 16) == 0 && ((uintptr_t)a->v % 16) == 0 && ((uintptr_t)a->out % 16) == 0 &&
                   a->q_stride_token % 8 == 0 && a->q_stride_head % 8 == 0 && a->k_stride_slot % 8 == 0 && a->k_stride_head % 8 == 0 &&
                   a->v_stride_slot % 8 == 0 && a->v_stride_head % 8 == 0,
               "fl_gqa_paged_attention_bf16: q / k / v / out rows must be 16-byte aligned (pointers, and strides multiples of 8 elements)");
  GqParams p;
  p.q = (const uint16_t*)a->q; p.k = (const uint16_t*)a->k; p.v = (const uint16_t*)a->v;
  p.o = (uint16_t*)a->out; p.lse = a->lse;
  p.part_o = nullptr; p.part_lse = nullptr;
  p.qo_indptr = a->qo_indptr; p.kv_indptr = a->kv_indptr; p.kv_indices = a->kv_indices;
  p.sqt = a->q_stride_token; p.sqh = a->q_stride_head; p.sks = a->k_stride_slot; p.skh = a->k_stride_head;
  p.svs = a->v_stride_slot; p.svh = a->v_stride_head;
  p.B = a->batch; p.T = (int)a->num_q_tokens; p.N = (int)a->num_kv_slots; p.NI = (int)a->num_kv_indices;
  p.Hq = a->num_qo_heads; p.G = G; p.S = a->num_splits; p.causal = a->causal != 0;
  p.scale_log2e = a->sm_scale * kGqLog2e;
  const hipStream_t st = (hipStream_t)stream;
  if (dec) {
    if (p.S > 1) {
      const long long rows = (long long)p.S * a->num_q_tokens * a->num_qo_heads;
      FL_CHECK_ARG(a->workspace != nullptr && ((uintptr_t)a->workspace % 16) == 0 && a->workspace_bytes >= rows * 129 * 4,
                   "fl_gqa_paged_attention_bf16: %d splits need a 16-byte aligned workspace of %lld bytes (got %lld)", p.S, rows * 129 * 4,
                   (long long)a->workspace_bytes);
      p.part_o = (float*)a->workspace;
      p.part_lse = p.part_o + rows * 128;
    }
    const dim3 grid((unsigned)a->batch, (unsigned)a->num_kv_heads, (unsigned)p.S);
    gqa_paged_bf16_kernel<true><<<grid, dim3(256), 0, st>>>(p);
    FL_CHECK_LAUNCH("gqa_paged_bf16_kernel<decode>");
    if (p.S > 1) {
      gqa_split_merge_kernel<<<dim3((unsigned)a->batch, (unsigned)a->num_kv_heads), dim3(256), 0, st>>>(p);
      FL_CHECK_LAUNCH("gqa_split_merge_kernel");
    }
  } else {
    // every request has at most ceil(len G / 128) <= len G / 128 + 1 row tiles
    const long long tiles = (a->num_q_tokens * G + kGqRows - 1) / kGqRows + a->batch;
    FL_CHECK_ARG(tiles < (1ll << 31), "fl_gqa_paged_attention_bf16: grid too large");
    gqa_paged_bf16_kernel<false><<<dim3((unsigned)tiles, (unsigned)a->num_kv_heads), dim3(256), 0, st>>>(p);
    FL_CHECK_LAUNCH("gqa_paged_bf16_kernel<row>");
  }
  return FL_OK;
}
