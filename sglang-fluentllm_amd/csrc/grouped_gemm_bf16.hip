// G5 — bf16 grouped GEMM of the unquantised MoE experts, bf16 out, gfx950 (MI355X) only.
//
// Replaces eps.executor.AokGroupedGemm.run (srt/layers/moe/gemms/bf16/aok.py:3,18 -> moe/executors/eps_executor.py:35,48: w13, silu, w2
// on the rows AllToAll.dispatch grouped by expert — bf16 checkpoints, bf16 draft / MTP layers, `ignored_layers` of an FP8 checkpoint):
//     out[r, n] = sum_k A[r, k] * W[e, n, k]   for r in [exclusive_sum[e], exclusive_sum[e + 1])      (fp32 accumulate, one RNE rounding)
// Rows outside [exclusive_sum[0], exclusive_sum[E]) are never written; exclusive_sum[0] may be non-zero.  Dense mode: one group, all rows.
//
// Mapping ("SwapAB", as every GEMM here): the WEIGHT rows sit on the MFMA M side and the token rows on the N side
// (D^T[n, m] = W_tile . A_tile^T on v_mfma_f32_32x32x16_bf16), so a lane owns ONE token row and 4 consecutive n per accumulator
// group — its stores are 8 contiguous bytes — and few rows per expert waste MFMA columns, not weight bandwidth.
// One workgroup = 4 waves = 128 weight rows x BM token rows, one template, two forms:
//   BM = 32  (decode):  wave w owns weight rows 32 w .. 32 w + 31 x the 32 tokens: 1 accumulator, 4 MFMAs + 8 ds_read_b128 per k block;
//                       3-stage ring of 20 KiB, two workgroups per CU.
//   BM = 128 (prefill): the waves sit 2 x 2, each owns 64 weight rows x 64 tokens: 4 accumulators (64 VGPRs), 16 MFMAs + 16 ds_read_b128
//                       per k block (every fragment feeds two MFMAs); 2-stage ring of 32 KiB, two workgroups per CU.
// A k block is 64 bf16 = ONE 128-byte line per row.  HBM -> LDS by global_load_lds_dwordx4: a wave-wide piece is 8 rows x 128 B, a
// stage's 16 weight pieces + BM / 8 token pieces are split evenly over the four waves (5 / 8 DMA instructions per wave per stage).
// Rows of 128 B span all 32 banks, so the 32 rows of a fragment read would meet in the same banks: position p of tile row j holds
// source chunk p ^ (j & 7).  The DMA lands lane l at (piece + 16 l) but fetches from ANY address, so the swizzle is applied on the
// SOURCE address and undone in the ds_read_b128 address — no cost on either side.
// Pipeline: stages kb + 1 .. kb + S - 2 stay in flight under the MFMAs of k block kb; completion is certified by a counted
// s_waitcnt vmcnt (the DMA is inline asm, invisible to hipcc's waitcnt pass) and ONE barrier per k block, after which the slot every
// wave left one barrier ago is refilled.
// Tails: token rows at or past the group's end are loaded from the group's last row and not stored; weight rows >= N (N % 128 == 64)
// are loaded from row N - 1 and not stored, and a wave whose rows all lie past N issues no MFMA.
// Scheduling: fl_gemm::locate_tile<BM> over the tile index, n tiles fastest inside a token tile (its rows re-hit L2); the grid is the
// tile upper bound, or the deep_gemm.set_num_sms cap with a stride loop over the tiles.
// The weight pieces go non-temporal when the tile's group fits ONE token tile: its [128 n x K] panel then has exactly one reader.
// No host synchronisation, no allocation, one launch: hipGraph-capturable.
#include "grouped_gemm_shared.h"

namespace {

constexpr int kGbBN = 128;                  // weight rows per workgroup
constexpr int kGbBK = 64;                   // bf16 per k block
constexpr int kGbRowB = 2 * kGbBK;          // one tile row of one stage: 128 B
constexpr int kGbPiece = 8 * kGbRowB;       // one wave-wide DMA piece: 8 rows
constexpr int kGbWBytes = kGbBN * kGbRowB;  // 16 KiB

// Ring depth of the 128-row form.  Measured at T = 16384 (4096 rows per expert, E = 32), w13 / w2 TFLOP/s: 4 stages + one workgroup per CU
// 637 / 575; 2 stages + two workgroups per CU 933 / 865 (profiles/grouped_gemm_bf16_ring_depth_ab.txt) — as on the FP8 kernel, two
// INDEPENDENT workgroups drift apart and one feeds the matrix pipe while the other sits in its barrier, DMA issue or LDS reads.
#ifndef FL_GB_LARGE_STAGES
#define FL_GB_LARGE_STAGES 2
#endif
template <int BM>
struct GbCfg {
  static constexpr int kSub = BM == 32 ? 1 : 2;             // 32-row sub-tiles per wave on either MFMA side
  static constexpr int kStages = BM == 32 ? 3 : FL_GB_LARGE_STAGES;
  static constexpr int kAPieces = BM / 32;                  // token pieces per wave per stage
  static constexpr int kPieces = 4 + kAPieces;              // DMA instructions per wave per stage
  static constexpr int kStageBytes = kGbWBytes + BM * kGbRowB;
  static constexpr int kLds = kStages * kStageBytes;        // 60 KiB / 64 KiB
  static constexpr int kPerCu = 2 * kLds <= 160 * 1024 ? 2 : 1;   // workgroups per CU
};
static_assert(2 * GbCfg<32>::kLds <= 160 * 1024 && GbCfg<128>::kLds <= 160 * 1024, "LDS per CU");
static_assert(GbCfg<128>::kPieces * (GbCfg<128>::kStages - 2) < 64, "vmcnt is a 6-bit field");

template <int N>
__device__ __forceinline__ void gb_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ v8bf gb_frag(const uint8_t* lds) {
  union { uint4 u; v8bf v; } x;
  x.u = *reinterpret_cast<const uint4*>(lds);
  return x.v;
}

// One output tile of one workgroup.  `bid` is the tile index: blockIdx.x, or the loop variable of a capped launch.
template <int BM>
__device__ __forceinline__ void gb_tile(const fl_gemm::GemmParams& p, const uint8_t* __restrict__ gA, const uint8_t* __restrict__ gW,
                                        const int32_t* __restrict__ gmeta, uint8_t* __restrict__ smem, const int bid) {
  using C = GbCfg<BM>;
  constexpr int S = C::kStages, P = C::kPieces, SUB = C::kSub;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kq = lane >> 5;

  // ---- tile -> (expert, token range, weight tile) ----
  const int nt = bid % p.n_tiles;
  const int mt = bid / p.n_tiles;
  int e = 0;
  long long row0 = 0, row_end = 0;
  if (!fl_gemm::locate_tile<BM>(p, gmeta, mt, e, row0, row_end)) return;
  if (row_end > p.M) row_end = p.M;          // (a malformed exclusive_sum must not reach past A / out)
  if (row0 < 0 || row0 >= row_end) return;
  const int n0 = nt * kGbBN;
  const long long g_lo = p.mode == fl_gemm::kOffset ? (long long)gmeta[e] : 0;
  const bool w_nt = row_end - g_lo <= BM;    // the group is this one token tile: nobody else streams this weight panel
  const int KB = p.K / kGbBK;
  const long long row_b = 2ll * p.K;         // bytes per row of A / W

  // ---- per-lane DMA sources: lane l of a piece brings row (l >> 3), LDS position (l & 7) = source chunk (l & 7) ^ (row & 7) ----
  const int sub = lane >> 3;
  const int ch16 = ((lane & 7) ^ sub) << 4;
  const uint8_t* wsrc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {   // this wave fills weight pieces 4 wave + k
    int n = n0 + 8 * (4 * wave + k) + sub;
    n = n < p.N ? n : p.N - 1;
    wsrc[k] = gW + ((long long)e * p.N + n) * row_b + ch16;
  }
  const uint8_t* asrc[C::kAPieces];
#pragma unroll
  for (int k = 0; k < C::kAPieces; ++k) {   // ... and token pieces kAPieces wave + k
    long long m = row0 + 8 * (C::kAPieces * wave + k) + sub;
    m = m < row_end ? m : row_end - 1;
    asrc[k] = gA + m * row_b + ch16;
  }
  auto issue = [&](const int kb) {
    uint8_t* st = smem + (kb % S) * C::kStageBytes;
    const long long k_off = (long long)kb * kGbRowB;
#pragma unroll
    for (int k = 0; k < 4; ++k) fl_dma16_pol(wsrc[k] + k_off, st + (4 * wave + k) * kGbPiece, w_nt);
#pragma unroll
    for (int k = 0; k < C::kAPieces; ++k) fl_dma16(asrc[k] + k_off, st + kGbWBytes + (C::kAPieces * wave + k) * kGbPiece);
  };

  // ---- fragment reads: k step s of row j is chunk 2 s + kq, at position (2 s + kq) ^ (j & 7); sub-tiles start at multiples of 32 ----
  int rb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) rb[s] = li * kGbRowB + (((2 * s + kq) ^ (li & 7)) << 4);
  const int w_row0 = BM == 32 ? 32 * wave : 64 * (wave & 1);   // this wave's first weight row / token row inside the tile
  const int t_row0 = BM == 32 ? 0 : 64 * (wave >> 1);
  const bool w_live = n0 + w_row0 < p.N;                       // (N % 64 == 0: a wave's weight rows are all below N or all past it)
  const int w_off = w_row0 * kGbRowB, t_off = kGbWBytes + t_row0 * kGbRowB;

  v16f acc[SUB][SUB];   // [weight sub-tile][token sub-tile]
#pragma unroll
  for (int i = 0; i < SUB; ++i)
#pragma unroll
    for (int j = 0; j < SUB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- prologue: stages 0 .. S - 2 ----
#pragma unroll
  for (int s = 0; s < S - 1; ++s)
    if (s < KB) issue(s);

  for (int kb = 0; kb < KB; ++kb) {
    // stage kb has landed for this wave; the stages issued after it (at most S - 2 of them exist) stay in flight
    const int later = KB - 1 - kb;
    if (later >= S - 2) gb_wait_vm<(S - 2) * P>();
    else if (S == 4 && later == 1) gb_wait_vm<P>();
    else gb_wait_vm<0>();
    __builtin_amdgcn_s_barrier();   // ... and for every wave; every wave is done with the slot of k block kb - 1
    if (kb + S - 1 < KB) issue(kb + S - 1);
    if (w_live) {
      const uint8_t* st = smem + (kb % S) * C::kStageBytes;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        v8bf wf[SUB], tf[SUB];
#pragma unroll
        for (int i = 0; i < SUB; ++i) wf[i] = gb_frag(st + w_off + i * (32 * kGbRowB) + rb[s]);
#pragma unroll
        for (int j = 0; j < SUB; ++j) tf[j] = gb_frag(st + t_off + j * (32 * kGbRowB) + rb[s]);
#pragma unroll
        for (int i = 0; i < SUB; ++i)
#pragma unroll
          for (int j = 0; j < SUB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i], tf[j], acc[i][j], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: D^T[n, m] -> out[m, n]; lane = token row li of a sub-tile, registers 4 g .. 4 g + 3 = n 8 g + 4 kq + (0 .. 3) ----
  if (!w_live) return;
#pragma unroll
  for (int j = 0; j < SUB; ++j) {
    const long long m = row0 + t_row0 + 32 * j + li;
    if (m >= row_end) continue;
    uint16_t* orow = p.out + m * p.N + n0 + w_row0 + 4 * kq;
#pragma unroll
    for (int i = 0; i < SUB; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<uint2*>(orow + 32 * i + 8 * g) = make_uint2(fl_pack_bf16(acc[i][j][4 * g], acc[i][j][4 * g + 1]),
                                                                      fl_pack_bf16(acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]));
  }
}

template <int BM>
__global__ __launch_bounds__(256, GbCfg<BM>::kPerCu) void grouped_gemm_bf16_kernel(const fl_gemm::GemmParams p, const uint8_t* __restrict__ gA,
                                                                                  const uint8_t* __restrict__ gW,
                                                                                  const int32_t* __restrict__ gmeta) {
  __shared__ __attribute__((aligned(1024))) uint8_t smem[GbCfg<BM>::kLds];
  for (int bid = blockIdx.x; bid < p.total_blocks; bid += gridDim.x) {
    gb_tile<BM>(p, gA, gW, gmeta, smem, bid);
    if (gridDim.x < (unsigned)p.total_blocks) {   // capped launch: every wave is done with the LDS ring before the next tile
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }
}

}  // namespace

#define GB_UNSUPPORTED(cond, ...)    \
  do {                               \
    if (!(cond)) {                   \
      fl_set_error(__VA_ARGS__);     \
      return FL_ERR_UNSUPPORTED;     \
    }                                \
  } while (0)

extern "C" int fl_grouped_gemm_bf16(const FlGemmBf16Args* a, fl_stream_t stream) {
  FL_CHECK_ARG(a != nullptr, "fl_grouped_gemm_bf16: null argument struct");
  FL_CHECK_ARG(a->struct_bytes == (int32_t)sizeof(FlGemmBf16Args),
               "fl_grouped_gemm_bf16: struct_bytes = %d, this library's FlGemmBf16Args has %d (caller built against another header)",
               (int)a->struct_bytes, (int)sizeof(FlGemmBf16Args));
  FL_CHECK_ARG(a->mode == FL_GEMM_OFFSET || a->mode == FL_GEMM_DENSE, "fl_grouped_gemm_bf16: mode %d (offset and dense only)", a->mode);
  FL_CHECK_ARG(a->tile_rows == 0 || a->tile_rows == 32 || a->tile_rows == 128, "fl_grouped_gemm_bf16: tile_rows = %d (0, 32 or 128)",
               a->tile_rows);
  FL_CHECK_ARG(a->num_groups >= 1 && (a->mode == FL_GEMM_OFFSET || a->num_groups == 1) && a->M >= 0 && a->M < (1ll << 31) - 256,
               "fl_grouped_gemm_bf16: bad sizes (groups %d, rows %lld)", a->num_groups, (long long)a->M);
  GB_UNSUPPORTED(a->K >= kGbBK && a->K % kGbBK == 0, "fl_grouped_gemm_bf16: K = %d must be a positive multiple of 64", a->K);
  GB_UNSUPPORTED(a->N >= 64 && a->N % 64 == 0, "fl_grouped_gemm_bf16: N = %d must be a positive multiple of 64", a->N);
  if (a->M == 0) return FL_OK;   // nothing routed to this rank (empty tensors have null pointers)
  FL_CHECK_ARG(a->A && a->W && a->out && (a->mode == FL_GEMM_DENSE || a->group_meta), "fl_grouped_gemm_bf16: null pointer");
  FL_CHECK_ARG(((uintptr_t)a->A % 16) == 0 && ((uintptr_t)a->W % 16) == 0 && ((uintptr_t)a->out % 8) == 0,
               "fl_grouped_gemm_bf16: A and W must be 16-byte aligned, out 8-byte aligned");
  fl_gemm::GemmParams p = {};
  p.mode = a->mode == FL_GEMM_DENSE ? fl_gemm::kDense : fl_gemm::kOffset;
  p.E = a->num_groups; p.M = (int)a->M; p.N = a->N; p.K = a->K;
  p.out = (uint16_t*)a->out;
  p.ksplit = 1;
  p.n_tiles = (a->N + kGbBN - 1) / kGbBN;
  const int bm = a->tile_rows != 0 ? a->tile_rows : (a->M / a->num_groups >= 64 ? 128 : 32);
  // every group has at most ceil(rows / bm) <= rows / bm + 1 token tiles
  const long long m_tiles = (a->M + bm - 1) / bm + (p.mode == fl_gemm::kOffset ? a->num_groups : 0);
  const long long blocks = m_tiles * p.n_tiles;
  FL_CHECK_ARG(blocks < (1ll << 31), "fl_grouped_gemm_bf16: grid too large");
  p.m_tiles_upper = (int)m_tiles;
  p.total_blocks = (int)blocks;
  const int cap = fl_gemm_cu_limit();
  const dim3 grid((unsigned)(cap > 0 && blocks > cap ? cap : blocks)), block(256);
  const hipStream_t s = (hipStream_t)stream;
  if (bm == 32)
    grouped_gemm_bf16_kernel<32><<<grid, block, 0, s>>>(p, (const uint8_t*)a->A, (const uint8_t*)a->W, a->group_meta);
  else
    grouped_gemm_bf16_kernel<128><<<grid, block, 0, s>>>(p, (const uint8_t*)a->A, (const uint8_t*)a->W, a->group_meta);
  FL_CHECK_LAUNCH("grouped_gemm_bf16_kernel");
  return FL_OK;
}
