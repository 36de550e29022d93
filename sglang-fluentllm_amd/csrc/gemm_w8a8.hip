// G6 — W8A8 dense GEMM: 8-bit operands (OCP e4m3fn or int8), per-token x per-channel scales applied ONCE after the product,
// bf16 / fp16 out, gfx950 (MI355X) only.
//
// Replaces flashinfer.fp8_scaled_mm (srt/layers/dense/gemms/fp8/fp8_utils.py:434,605 apply_fp8_linear; layouts/w8a8_fp8.py) and
// flashinfer.int8_scaled_mm (layouts/w8a8_int8.py:203-216 W8A8Int8LinearMethod.apply; compressed_tensors_w8a8_int8.py:167-169):
//     C[m, n] = out_dtype( f32( sum_k A[m, k] * B[n, k] ) * sa[m] * sb[n] + bias[n] )
// A [M, K] one byte per element with a row stride, B [N, K] the weight as stored ("nt"), sa / sb f32 per row / per column or ONE
// entry (element stride 0), bias optional in the output type.  The k loop carries no scale arithmetic: bytes -> LDS -> MFMA.
//
// One template over the element type and the token tile:
//   e4m3fn: v_mfma_scale_f32_32x32x64_f8f6f4 with unit E8M0 scales, f32 accumulators;
//   int8:   v_mfma_i32_32x32x32_i8, i32 accumulators (exact), converted to f32 only in the epilogue.
// Mapping ("SwapAB", as every GEMM here): the WEIGHT rows sit on the MFMA M side and the token rows on the N side, so a lane owns
// ONE token row and 4 consecutive n per accumulator group: sa[m] is one register per lane, its stores are 8 contiguous bytes.
//   BM = 32  (decode): a weight stream.  64 weight rows x 32 tokens per workgroup of TWO waves (wave w: weight rows 32 w .. 32 w + 31),
//                      so N = 7168 gives 112 workgroups; 4-stage ring of 12 KiB, three workgroups per CU (108 KiB in flight per
//                      CU); the weight panel has exactly one reader when M <= 32 and is then loaded non-temporally.
//   BM = 128 (compute): 128 weight rows x 128 tokens per workgroup of four waves sitting 2 x 2, each 64 x 64: 4 accumulators,
//                      every fragment feeds two MFMAs; 2-stage ring of 32 KiB, two workgroups per CU (they drift apart: one
//                      feeds the matrix pipe while the other sits in its barrier / DMA issue / LDS reads — grouped_gemm_bf16.hip).
// A k block is 128 bytes = ONE line per row.  HBM -> LDS by global_load_lds_dwordx4: a wave-wide piece is 8 rows x 128 B.  Rows of
// 128 B span all 32 banks: position p of tile row j holds source chunk p ^ (j & 7), applied on the DMA's SOURCE address and undone
// in the ds_read_b128 address.  Lane half kq reads chunk 2 s + kq for k step s (int8: one MFMA per step; fp8: steps 2 t, 2 t + 1
// make one 32-byte operand) — both operands take the same chunks, so each register slot meets the same k on either side.
// Tails: K % 128 != 0 -> the chunks of the LAST k block at or past K are fetched from a 16-byte device constant of zeros (never
// past the row; the DMA count per stage is unchanged); token rows >= M / weight rows >= N are loaded from the last valid row
// and never stored (N % 16 == 0: a lane's group of 4 columns is all inside or all outside).
// Pipeline: counted s_waitcnt vmcnt (the DMA is inline asm) + ONE barrier per k block, after which the slot every wave left one
// barrier ago is refilled.  One launch, no host synchronisation, no allocation: hipGraph-capturable.
#include "fl_common.h"
#include <type_traits>

namespace {

typedef int v16i __attribute__((ext_vector_type(16)));
typedef _Float16 fl_f16x2 __attribute__((ext_vector_type(2)));

constexpr int kWaBK = 128;            // bytes (= elements) per k block
constexpr int kWaPiece = 8 * kWaBK;   // one wave-wide DMA piece: 8 rows
constexpr int kWaUnit = 0x7F;         // E8M0 2^0

__device__ uint4 g_wa_zero16;         // source of the zero-filled k tail (zero-initialised, never written)

template <int BM>
struct WaCfg {
  static constexpr int kWaves = BM == 32 ? 2 : 4;
  static constexpr int kThreads = 64 * kWaves;
  static constexpr int kBN = BM == 32 ? 64 : 128;           // weight rows per workgroup
  static constexpr int kSub = BM == 32 ? 1 : 2;             // 32-row sub-tiles per wave on either MFMA side
  static constexpr int kStages = BM == 32 ? 4 : 2;
  static constexpr int kWPieces = kBN / 8 / kWaves;         // weight pieces per wave per stage (4)
  static constexpr int kAPieces = BM / 8 / kWaves;          // token pieces per wave per stage (2 / 4)
  static constexpr int kPieces = kWPieces + kAPieces;       // DMA instructions per wave per stage
  static constexpr int kWBytes = kBN * kWaBK;
  static constexpr int kStageBytes = kWBytes + BM * kWaBK;  // 12 KiB / 32 KiB
  static constexpr int kLds = kStages * kStageBytes;        // 48 KiB / 64 KiB
  static constexpr int kPerCu = BM == 32 ? 3 : 2;           // workgroups per CU the LDS allows
};
static_assert(WaCfg<32>::kPerCu * WaCfg<32>::kLds <= 160 * 1024 && WaCfg<128>::kPerCu * WaCfg<128>::kLds <= 160 * 1024, "LDS per CU");
static_assert(WaCfg<32>::kPieces * (WaCfg<32>::kStages - 2) < 64, "vmcnt is a 6-bit field");

struct WaParams {
  int M, N, K, n_tiles;
  long long lda, ldb, ldc;
  int sa_stride, sb_stride, out_fp16;
  const float* sa;
  const float* sb;
  const uint16_t* bias;
  uint16_t* out;
};

template <int N>
__device__ __forceinline__ void wa_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ v4i wa_frag(const uint8_t* lds) {
  union { uint4 u; v4i v; } x;
  x.u = *reinterpret_cast<const uint4*>(lds);
  return x.v;
}
__device__ __forceinline__ v8i wa_cat(const v4i a, const v4i b) {
  return v8i{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
__device__ __forceinline__ float wa_half_to_f32(const uint16_t h) {
  union { uint16_t u; _Float16 f; } x;
  x.u = h;
  return (float)x.f;
}
__device__ __forceinline__ uint32_t wa_pack_f16(const float a, const float b) {   // RNE (v_cvt_f16_f32), not the pkrtz form
  union { fl_f16x2 h; uint32_t u; } x;
  x.h = __builtin_convertvector(fl_f32x2{a, b}, fl_f16x2);
  return x.u;
}

template <bool kInt8, int BM>
__global__ __launch_bounds__(WaCfg<BM>::kThreads, 2) void gemm_w8a8_kernel(const WaParams p, const uint8_t* __restrict__ gA,
                                                                          const uint8_t* __restrict__ gW) {
  using C = WaCfg<BM>;
  using Acc = typename std::conditional<kInt8, v16i, v16f>::type;
  constexpr int S = C::kStages, P = C::kPieces, SUB = C::kSub;
  __shared__ __attribute__((aligned(1024))) uint8_t smem[C::kLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kq = lane >> 5;

  // ---- tile: n tiles fastest inside a token tile (its rows re-hit L2) ----
  const int nt = blockIdx.x % p.n_tiles;
  const int mt = blockIdx.x / p.n_tiles;
  const int n0 = nt * C::kBN;
  const long long row0 = (long long)mt * BM;
  const int KB = (p.K + kWaBK - 1) / kWaBK;
  const int tail_chunks = (p.K >> 4) - 8 * (KB - 1);   // 16-byte chunks of the last k block that lie inside the row: 1 .. 8
  const bool w_nt = p.M <= BM;                         // one token tile: nobody else streams this weight panel

  // ---- per-lane DMA sources: lane l of a piece brings row (l >> 3), LDS position (l & 7) = source chunk (l & 7) ^ (row & 7) ----
  const int sub = lane >> 3;
  const int ch = (lane & 7) ^ sub;
  const uint8_t* wsrc[C::kWPieces];
#pragma unroll
  for (int k = 0; k < C::kWPieces; ++k) {   // this wave fills weight pieces kWPieces wave + k
    int n = n0 + 8 * (C::kWPieces * wave + k) + sub;
    n = n < p.N ? n : p.N - 1;
    wsrc[k] = gW + n * p.ldb + 16 * ch;
  }
  const uint8_t* asrc[C::kAPieces];
#pragma unroll
  for (int k = 0; k < C::kAPieces; ++k) {   // ... and token pieces kAPieces wave + k
    long long m = row0 + 8 * (C::kAPieces * wave + k) + sub;
    m = m < p.M ? m : p.M - 1;
    asrc[k] = gA + m * p.lda + 16 * ch;
  }
  const uint8_t* const zero = reinterpret_cast<const uint8_t*>(&g_wa_zero16);
  const bool in_row = ch < tail_chunks;     // this lane's chunk of the LAST k block lies inside the row
  auto issue = [&](const int kb) {
    uint8_t* st = smem + (kb % S) * C::kStageBytes;
    const long long k_off = (long long)kb * kWaBK;
    if (kb == KB - 1 && tail_chunks < 8) {  // (wave-uniform) the ragged k tail: chunks past K come from the zeros, same DMA count
#pragma unroll
      for (int k = 0; k < C::kWPieces; ++k) fl_dma16(in_row ? wsrc[k] + k_off : zero, st + (C::kWPieces * wave + k) * kWaPiece);
#pragma unroll
      for (int k = 0; k < C::kAPieces; ++k)
        fl_dma16(in_row ? asrc[k] + k_off : zero, st + C::kWBytes + (C::kAPieces * wave + k) * kWaPiece);
    } else {
#pragma unroll
      for (int k = 0; k < C::kWPieces; ++k) fl_dma16_pol(wsrc[k] + k_off, st + (C::kWPieces * wave + k) * kWaPiece, w_nt);
#pragma unroll
      for (int k = 0; k < C::kAPieces; ++k) fl_dma16(asrc[k] + k_off, st + C::kWBytes + (C::kAPieces * wave + k) * kWaPiece);
    }
  };

  // ---- fragment reads: k step s of row j is chunk 2 s + kq, at position (2 s + kq) ^ (j & 7); sub-tiles start at multiples of 32 ----
  int rb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) rb[s] = li * kWaBK + (((2 * s + kq) ^ (li & 7)) << 4);
  const int w_row0 = BM == 32 ? 32 * wave : 64 * (wave & 1);   // this wave's first weight row / token row inside the tile
  const int t_row0 = BM == 32 ? 0 : 64 * (wave >> 1);
  const bool w_live = n0 + w_row0 < p.N && row0 + t_row0 < p.M;   // (wave-uniform) something of this wave's 2 x 2 sub-tiles is stored
  const int w_off = w_row0 * kWaBK, t_off = C::kWBytes + t_row0 * kWaBK;

  Acc acc[SUB][SUB];   // [weight sub-tile][token sub-tile]
#pragma unroll
  for (int i = 0; i < SUB; ++i)
#pragma unroll
    for (int j = 0; j < SUB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  // ---- prologue: stages 0 .. S - 2 ----
#pragma unroll
  for (int s = 0; s < S - 1; ++s)
    if (s < KB) issue(s);

  for (int kb = 0; kb < KB; ++kb) {
    // stage kb has landed for this wave; the stages issued after it (at most S - 2 of them exist) stay in flight
    const int later = KB - 1 - kb;
    if (later >= S - 2) wa_wait_vm<(S - 2) * P>();
    else if (S == 4 && later == 1) wa_wait_vm<P>();
    else wa_wait_vm<0>();
    __builtin_amdgcn_s_barrier();   // ... and for every wave; every wave is done with the slot of k block kb - 1
    if (kb + S - 1 < KB) issue(kb + S - 1);
    if (w_live) {
      const uint8_t* st = smem + (kb % S) * C::kStageBytes;
      if constexpr (kInt8) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          v4i wf[SUB], tf[SUB];
#pragma unroll
          for (int i = 0; i < SUB; ++i) wf[i] = wa_frag(st + w_off + i * (32 * kWaBK) + rb[s]);
#pragma unroll
          for (int j = 0; j < SUB; ++j) tf[j] = wa_frag(st + t_off + j * (32 * kWaBK) + rb[s]);
#pragma unroll
          for (int i = 0; i < SUB; ++i)
#pragma unroll
            for (int j = 0; j < SUB; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[i], tf[j], acc[i][j], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          v8i wf[SUB], tf[SUB];
#pragma unroll
          for (int i = 0; i < SUB; ++i)
            wf[i] = wa_cat(wa_frag(st + w_off + i * (32 * kWaBK) + rb[2 * t]), wa_frag(st + w_off + i * (32 * kWaBK) + rb[2 * t + 1]));
#pragma unroll
          for (int j = 0; j < SUB; ++j)
            tf[j] = wa_cat(wa_frag(st + t_off + j * (32 * kWaBK) + rb[2 * t]), wa_frag(st + t_off + j * (32 * kWaBK) + rb[2 * t + 1]));
#pragma unroll
          for (int i = 0; i < SUB; ++i)
#pragma unroll
            for (int j = 0; j < SUB; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[i], tf[j], acc[i][j], 0, 0, 0, kWaUnit, 0, kWaUnit);
        }
      }
    }
  }

  // ---- epilogue: D^T[n, m] -> out[m, n]; lane = token row li of a sub-tile, registers 4 g .. 4 g + 3 = n 8 g + 4 kq + (0 .. 3) ----
  if (!w_live) return;
  float sbv[SUB][16], bv[SUB][16];   // this lane's 16 columns per weight sub-tile: loaded once, used for every token sub-tile
#pragma unroll
  for (int i = 0; i < SUB; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + w_row0 + 32 * i + 8 * g + 4 * kq + r;
        const bool ok = n < p.N;
        sbv[i][4 * g + r] = ok ? p.sb[(long long)n * p.sb_stride] : 0.f;
        float b = 0.f;
        if (ok && p.bias != nullptr) b = p.out_fp16 ? wa_half_to_f32(p.bias[n]) : fl_bf16_to_f32(p.bias[n]);
        bv[i][4 * g + r] = b;
      }
#pragma unroll
  for (int j = 0; j < SUB; ++j) {
    const long long m = row0 + t_row0 + 32 * j + li;
    if (m >= p.M) continue;
    const float a_s = p.sa[m * p.sa_stride];
    uint16_t* orow = p.out + m * p.ldc + n0 + w_row0 + 4 * kq;
#pragma unroll
    for (int i = 0; i < SUB; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (n0 + w_row0 + 32 * i + 8 * g + 4 * kq >= p.N) continue;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (float)acc[i][j][4 * g + r] * a_s * sbv[i][4 * g + r] + bv[i][4 * g + r];
        *reinterpret_cast<uint2*>(orow + 32 * i + 8 * g) = p.out_fp16 ? make_uint2(wa_pack_f16(v[0], v[1]), wa_pack_f16(v[2], v[3]))
                                                                      : make_uint2(fl_pack_bf16(v[0], v[1]), fl_pack_bf16(v[2], v[3]));
      }
  }
}

template <bool kInt8, int BM>
void wa_launch(const WaParams& p, const void* A, const void* B, const long long m_tiles, hipStream_t s) {
  const dim3 grid((unsigned)(m_tiles * p.n_tiles)), block(WaCfg<BM>::kThreads);
  gemm_w8a8_kernel<kInt8, BM><<<grid, block, 0, s>>>(p, (const uint8_t*)A, (const uint8_t*)B);
}

}  // namespace

// Rows from which the 128-row form is used when tile_rows = 0.  A GUESS with ONE measured point under it: at M = 128 the 32-row
// form (four token tiles re-reading the panel from L2, 4 x the workgroups) is 2 x faster than one 128-row tile per 128 columns on
// all three timed shapes (profiles/gemm_w8a8_first_measurement.txt); between 128 and 4096 rows nothing has been timed.
constexpr long long kWaComputeFormMinRows = 129;

extern "C" int fl_gemm_w8a8(const FlGemmW8A8Args* a, fl_stream_t stream) {
  FL_CHECK_ARG(a != nullptr, "fl_gemm_w8a8: null argument struct");
  FL_CHECK_ARG(a->struct_bytes == (int32_t)sizeof(FlGemmW8A8Args),
               "fl_gemm_w8a8: struct_bytes = %d, this library's FlGemmW8A8Args has %d (caller built against another header)",
               (int)a->struct_bytes, (int)sizeof(FlGemmW8A8Args));
  FL_CHECK_ARG(a->elem_type == FL_W8A8_FP8_E4M3 || a->elem_type == FL_W8A8_INT8, "fl_gemm_w8a8: elem_type %d (e4m3fn or int8)", a->elem_type);
  FL_CHECK_ARG(a->out_type == FL_W8A8_OUT_BF16 || a->out_type == FL_W8A8_OUT_FP16, "fl_gemm_w8a8: out_type %d (bf16 or fp16)", a->out_type);
  FL_CHECK_ARG(a->tile_rows == 0 || a->tile_rows == 32 || a->tile_rows == 128, "fl_gemm_w8a8: tile_rows = %d (0, 32 or 128)", a->tile_rows);
  FL_CHECK_ARG(a->M >= 0 && a->M < (1ll << 31) - 256, "fl_gemm_w8a8: M = %lld", (long long)a->M);
  FL_CHECK_ARG(a->K >= 16 && a->K % 16 == 0, "fl_gemm_w8a8: K = %d must be a positive multiple of 16", a->K);
  FL_CHECK_ARG(a->N >= 16 && a->N % 16 == 0, "fl_gemm_w8a8: N = %d must be a positive multiple of 16", a->N);
  FL_CHECK_ARG(a->lda >= a->K && a->lda % 16 == 0, "fl_gemm_w8a8: lda = %lld must be >= K and a multiple of 16", (long long)a->lda);
  FL_CHECK_ARG(a->ldb >= a->K && a->ldb % 16 == 0, "fl_gemm_w8a8: ldb = %lld must be >= K and a multiple of 16", (long long)a->ldb);
  FL_CHECK_ARG(a->ldc >= a->N && a->ldc % 4 == 0, "fl_gemm_w8a8: ldc = %lld must be >= N and a multiple of 4", (long long)a->ldc);
  FL_CHECK_ARG((a->sa_stride == 0 || a->sa_stride == 1) && (a->sb_stride == 0 || a->sb_stride == 1),
               "fl_gemm_w8a8: scale strides (%lld, %lld) must be 1 (one per row / column) or 0 (one entry)", (long long)a->sa_stride,
               (long long)a->sb_stride);
  if (a->M == 0) return FL_OK;   // (empty tensors have null pointers)
  FL_CHECK_ARG(a->A && a->B && a->sa && a->sb && a->out, "fl_gemm_w8a8: null pointer");
  FL_CHECK_ARG(((uintptr_t)a->A % 16) == 0 && ((uintptr_t)a->B % 16) == 0 && ((uintptr_t)a->out % 8) == 0 &&
                   ((uintptr_t)a->sa % 4) == 0 && ((uintptr_t)a->sb % 4) == 0 && ((uintptr_t)a->bias % 2) == 0,
               "fl_gemm_w8a8: A and B must be 16-byte aligned, out 8-byte aligned");
  const int bm = a->tile_rows != 0 ? a->tile_rows : (a->M >= kWaComputeFormMinRows ? 128 : 32);
  WaParams p = {};
  p.M = (int)a->M; p.N = a->N; p.K = a->K;
  p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc;
  p.sa_stride = (int)a->sa_stride; p.sb_stride = (int)a->sb_stride;
  p.out_fp16 = a->out_type == FL_W8A8_OUT_FP16;
  p.sa = a->sa; p.sb = a->sb; p.bias = (const uint16_t*)a->bias; p.out = (uint16_t*)a->out;
  p.n_tiles = (a->N + (bm == 32 ? 64 : 128) - 1) / (bm == 32 ? 64 : 128);
  const long long m_tiles = (a->M + bm - 1) / bm;
  FL_CHECK_ARG(m_tiles * p.n_tiles < (1ll << 31), "fl_gemm_w8a8: grid too large");
  const hipStream_t s = (hipStream_t)stream;
  const bool i8 = a->elem_type == FL_W8A8_INT8;
  if (bm == 32) {
    if (i8) wa_launch<true, 32>(p, a->A, a->B, m_tiles, s);
    else wa_launch<false, 32>(p, a->A, a->B, m_tiles, s);
  } else {
    if (i8) wa_launch<true, 128>(p, a->A, a->B, m_tiles, s);
    else wa_launch<false, 128>(p, a->A, a->B, m_tiles, s);
  }
  FL_CHECK_LAUNCH("gemm_w8a8_kernel");
  return FL_OK;
}
