// flashinfer.sampling on gfx950: softmax, top-k / top-p renormalisation and top-k / top-p / min-p sampling over probs [B, V] f32.
// Sort-free and rejection-free: ONE workgroup (8 waves) owns one row and finds the row's exact cut value by a radix descent on the f32
// bit pattern (non-negative floats order like their bits), then writes the renormalised row or walks the inverse CDF once.
//
//   key(x) = bits(x) for x > 0, else 0 (31 bits).  Digits 11 / 10 / 10 from the top: three passes.  A pass builds, per WAVE, an LDS
//   histogram {count u32, mass f32} over the current digit of the keys that match the prefix found so far (8 waves x 2048 buckets x 8 B
//   = 128 KiB, dynamic LDS; each wave adds to its own copy, in its own fixed order: the result is deterministic).  Zeros never touch the
//   LDS (a row that top_k_renorm has already filtered is almost all zeros): they are counted in a register.  Each thread then sums the
//   eight copies of `buckets / 512` neighbouring buckets, a workgroup scan from the TOP bucket gives every bucket the count and mass
//   above it, and the first non-empty bucket at which the running count reaches k or the running mass reaches top_p * S_base holds the
//   cut (neither reached, by rounding or because nothing is filtered: the lowest non-empty bucket).  After the last digit the cut key t,
//   count and mass above it and at it are known: kept = {key >= t}, S_kept = mass above + mass at.  "joint" tracks both conditions in one
//   descent (the first to trigger is the higher threshold = the intersection); "top_k_first" descends twice (top-k for its kept mass, then
//   jointly with top_p * that mass).  min-p needs no descent: one pass for the row maximum.
//
//   The row is read with 16-byte loads from the first 16-byte aligned element on (scalar head and tail); a "chunk" is what one wave loads
//   in one instruction (256 consecutive elements; head and tail are chunks of their own), wave w takes chunks w, w + 8, ... four at a time.
//   The first pass reads HBM, the later ones find the row (517 KB at V = 129,280) in the L2 of the XCD the workgroup runs on.
//
//   Sampling: kept mass per chunk (wave reduce) -> LDS, a workgroup scan over the chunks finds the first chunk whose inclusive prefix
//   exceeds u * total, wave 0 scans inside it.  Rounding can let a running sum end below the target: then the LAST kept element (of the
//   chunk, or of the row) is returned, so an id is always a kept element of positive probability.
#include "fl_common.h"

namespace {

constexpr int kSpThreads = 512, kSpWaves = 8, kSpBuckets = 2048;
constexpr int kSpHistBytes = kSpWaves * kSpBuckets * 8;   // counts [8][2048] u32, then masses [8][2048] f32
constexpr int kSpMaxVocab = 1 << 22;                       // chunk sums (V / 256 + 3 floats) must fit the histogram's LDS

struct SpParams {
  const float* probs; long long pitch, num_rows; int V;
  const int* indices;
  const void* top_k; int top_k_i64; long long top_k_val;
  const float* top_p; float top_p_val;
  const float* min_p; float min_p_val;
  const float* temp; float temp_val;
  const float* u;
  int mode;
  void* out;
};

struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };   // 16-byte store at a 4-byte aligned address

struct SpRow { const float* p; int V, head, nvec, tail, nchunks; };

__device__ __forceinline__ SpRow sp_row(const float* p, const int V) {
  SpRow r;
  r.p = p; r.V = V;
  r.head = min(V, (4 - (int)(((uintptr_t)p >> 2) & 3)) & 3);
  r.nvec = (V - r.head) >> 2;
  r.tail = V - r.head - 4 * r.nvec;
  r.nchunks = (r.nvec + 63) / 64 + 2;
  return r;
}

// this lane's up to four consecutive elements of chunk c (c < nchunks): returns how many, i0 = index of the first
__device__ __forceinline__ int sp_load(const SpRow& r, const int c, const int lane, float (&v)[4], int& i0) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (c == 0 || c == r.nchunks - 1) {
    const int n = lane == 0 ? (c == 0 ? r.head : r.tail) : 0;
    i0 = c == 0 ? 0 : r.head + 4 * r.nvec;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < n) v[j] = r.p[i0 + j];
    return n;
  }
  const int vi = (c - 1) * 64 + lane;
  i0 = r.head + 4 * vi;
  if (vi >= r.nvec) return 0;
  const float4 x = *reinterpret_cast<const float4*>(r.p + i0);
  v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  return 4;
}

// f(c, v, n, i0) for every chunk of this wave, loads of four chunks in flight; f also sees c >= nchunks (with n = 0)
template <class F>
__device__ __forceinline__ void sp_for_chunks(const SpRow& r, const int wave, const int lane, F&& f) {
  for (int c0 = wave; c0 < r.nchunks; c0 += kSpWaves * 4) {
    float v[4][4];
    int n[4], i0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + i * kSpWaves;
      i0[i] = 0;
      n[i] = c < r.nchunks ? sp_load(r, c, lane, v[i], i0[i]) : 0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) f(c0 + i * kSpWaves, v[i], n[i], i0[i]);
  }
}

__device__ __forceinline__ unsigned sp_key(const float x) { return x > 0.f ? __float_as_uint(x) : 0u; }

__device__ __forceinline__ float sp_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// small LDS state shared by the passes
struct SpShared {
  unsigned wc[kSpWaves];
  float wm[kSpWaves];
  int first, last;
  unsigned prefix, c_gt, c_eq;
  float m_gt, m_eq, excl;
  unsigned maxkey;
};

// exclusive scan over the workgroup in thread order of (c, m); totals to every thread.  The caller has a barrier between two scans.
__device__ __forceinline__ void sp_block_scan(unsigned& c, float& m, unsigned& totc, float& totm, SpShared& sh, const int wave, const int lane) {
  unsigned ic = c;
  float im = m;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned tc = __shfl_up(ic, d, 64);
    const float tm = __shfl_up(im, d, 64);
    if (lane >= d) { ic += tc; im += tm; }
  }
  if (lane == 63) { sh.wc[wave] = ic; sh.wm[wave] = im; }
  const unsigned ec = __shfl_up(ic, 1, 64);
  const float em = __shfl_up(im, 1, 64);
  __syncthreads();
  unsigned pc = 0; float pm = 0.f;
  totc = 0; totm = 0.f;
#pragma unroll
  for (int w = 0; w < kSpWaves; ++w) {
    if (w == wave) { pc = totc; pm = totm; }
    totc += sh.wc[w]; totm += sh.wm[w];
  }
  c = pc + (lane ? ec : 0u);
  m = pm + (lane ? em : 0.f);
}

// One radix descent.  k: count condition (INT_MAX = none); top_p < 0: no mass condition; else the mass condition is top_p * base, where
// base = the row sum (base < 0) or the given mass.  Leaves the cut in sh (prefix = t, c_gt, m_gt, c_eq, m_eq); returns the row sum.
// `levels` = 1 only sums the row (nothing is filtered).
__device__ float sp_descend(const SpRow& r, unsigned* hist, SpShared& sh, const int k, const float top_p, const float base, const int levels,
                            const int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  unsigned* const cnt = hist + wave * kSpBuckets;
  float* const mass = reinterpret_cast<float*>(hist + kSpWaves * kSpBuckets) + wave * kSpBuckets;
  float row_sum = 0.f, P = top_p < 0.f ? __builtin_inff() : top_p * base;
  if (tid == 0) { sh.prefix = 0; sh.c_gt = 0; sh.m_gt = 0.f; sh.c_eq = 0; sh.m_eq = 0.f; }
  for (int level = 0; level < levels; ++level) {
    const int bits = level == 0 ? 11 : 10, shift = level == 0 ? 20 : (level == 1 ? 10 : 0);
    const int nb = 1 << bits, run = nb / kSpThreads;
    for (int i = tid; i < 2 * kSpWaves * kSpBuckets; i += kSpThreads) hist[i] = 0;
    if (tid == 0) { sh.first = 0x7fffffff; sh.last = -1; }
    __syncthreads();
    const unsigned prefix = sh.prefix, carry_c = sh.c_gt;
    const float carry_m = sh.m_gt;
    unsigned zeros = 0;
    sp_for_chunks(r, wave, lane, [&](int, const float (&v)[4], const int n, int) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned key = sp_key(v[j]);
        if (j < n && (level == 0 || (key >> (shift + bits)) == prefix)) {
          if (key == 0) {
            ++zeros;
          } else {
            const unsigned b = (key >> shift) & (nb - 1);
            atomicAdd(&cnt[b], 1u);
            atomicAdd(&mass[b], v[j]);
          }
        }
      }
    });
    if (zeros) atomicAdd(&cnt[0], zeros);
    __syncthreads();
    // this thread's `run` neighbouring buckets, from the top: position pos <-> bucket nb - 1 - pos
    unsigned c[4], lc = 0;
    float m[4], lm = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = 0; m[j] = 0.f;
      if (j < run) {
        const int b = nb - 1 - (tid * run + j);
#pragma unroll
        for (int w = 0; w < kSpWaves; ++w) {
          c[j] += hist[w * kSpBuckets + b];
          m[j] += reinterpret_cast<const float*>(hist + kSpWaves * kSpBuckets)[w * kSpBuckets + b];
        }
        lc += c[j]; lm += m[j];
      }
    }
    unsigned totc; float totm;
    sp_block_scan(lc, lm, totc, totm, sh, wave, lane);   // lc, lm: count and mass above this thread's first bucket
    if (level == 0) {
      row_sum = totm;
      if (top_p >= 0.f && base < 0.f) P = top_p * row_sum;
    }
    int first = 0x7fffffff, last = -1;
    {
      unsigned rc = lc; float rm = lm;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < run && c[j] > 0) {
          last = tid * run + j;
          if (first == 0x7fffffff && (carry_c + rc + c[j] >= (unsigned)k || carry_m + (rm + m[j]) >= P)) first = last;
        }
        rc += c[j]; rm += m[j];
      }
    }
    if (first != 0x7fffffff) atomicMin(&sh.first, first);
    if (last >= 0) atomicMax(&sh.last, last);
    __syncthreads();
    const int sel = sh.first != 0x7fffffff ? sh.first : sh.last;   // a row has at least one element: sh.last >= 0
    if (sel >= 0 && sel / run == tid) {
      unsigned rc = lc; float rm = lm, me = 0.f; unsigned ce = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < sel % run) { rc += c[j]; rm += m[j]; }
        if (j == sel % run) { ce = c[j]; me = m[j]; }
      }
      sh.c_gt = carry_c + rc; sh.m_gt = carry_m + rm; sh.c_eq = ce; sh.m_eq = me;
      sh.prefix = (prefix << bits) | (unsigned)(nb - 1 - sel);
    }
    __syncthreads();
  }
  return row_sum;
}

// The cut key of this row under `mode` (kept = key >= cut, cut >= 1: zeros are never kept) and, for the renormalisation, S_kept.
__device__ unsigned sp_cut(const SpParams& p, const SpRow& r, const long long row, unsigned* hist, SpShared& sh, const int tid,
                           const bool want_sum, float& s_kept) {
  const int wave = tid >> 6, lane = tid & 63;
  if (p.mode == FL_SAMPLING_MIN_P) {
    if (tid == 0) sh.maxkey = 0;
    __syncthreads();
    unsigned mk = 0;
    sp_for_chunks(r, wave, lane, [&](int, const float (&v)[4], const int n, int) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n) mk = max(mk, sp_key(v[j]));
    });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mk = max(mk, (unsigned)__shfl_xor(mk, d, 64));
    if (lane == 0) atomicMax(&sh.maxkey, mk);
    __syncthreads();
    const float thr = (p.min_p ? p.min_p[row] : p.min_p_val) * __uint_as_float(sh.maxkey);   // ONE f32 multiply
    s_kept = 0.f;   // min-p renormalisation is not served
    return max(sp_key(thr), 1u);
  }
  long long k64 = p.top_k ? (p.top_k_i64 ? ((const long long*)p.top_k)[row] : (long long)((const int*)p.top_k)[row]) : p.top_k_val;
  float top_p = p.top_p ? p.top_p[row] : p.top_p_val;
  if (p.mode == FL_SAMPLING_TOP_P) k64 = 0x7fffffffll;
  if (p.mode == FL_SAMPLING_TOP_K || !(top_p < 1.f)) top_p = -1.f;   // top_p >= 1 keeps everything positive: no mass condition
  int k = (int)min(max(k64, 1ll), 0x7fffffffll);
  if (k >= r.V) k = 0x7fffffff;
  const bool filters = k != 0x7fffffff || top_p >= 0.f;
  if (!filters) {
    if (want_sum) s_kept = sp_descend(r, hist, sh, k, top_p, -1.f, 1, tid);
    return 1u;
  }
  if (p.mode == FL_SAMPLING_TOP_K_THEN_P && top_p >= 0.f && k != 0x7fffffff) {
    sp_descend(r, hist, sh, k, -1.f, -1.f, 3, tid);
    const float s_k = sh.m_gt + sh.m_eq;
    __syncthreads();
    sp_descend(r, hist, sh, k, top_p, s_k, 3, tid);
  } else {
    sp_descend(r, hist, sh, k, top_p, -1.f, 3, tid);
  }
  s_kept = sh.m_gt + sh.m_eq;
  return max(sh.prefix, 1u);
}

template <bool kSample>
__global__ __launch_bounds__(kSpThreads) void sampling_kernel(const SpParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned sp_hist[];
  __shared__ SpShared sh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  long long row = b;
  if (kSample && p.indices) row = min(max((long long)p.indices[b], 0ll), p.num_rows - 1);
  const SpRow r = sp_row(p.probs + row * p.pitch, p.V);
  float s_kept = 0.f;
  const unsigned cut = sp_cut(p, r, row, sp_hist, sh, tid, !kSample, s_kept);

  if constexpr (!kSample) {
    float* const out = (float*)p.out + (long long)b * p.V;
    sp_for_chunks(r, wave, lane, [&](int, const float (&v)[4], const int n, const int i0) {
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = sp_key(v[j]) >= cut ? v[j] / s_kept : 0.f;
      if (n == 4) {
        *reinterpret_cast<f4u*>(out + i0) = f4u{o[0], o[1], o[2], o[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < n) out[i0 + j] = o[j];
      }
    });
    return;
  }

  // kept mass per chunk
  float* const csum = reinterpret_cast<float*>(sp_hist);
  __syncthreads();   // the descent's last reads of the histogram are over
  sp_for_chunks(r, wave, lane, [&](const int c, const float (&v)[4], int, int) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s += sp_key(v[j]) >= cut ? v[j] : 0.f;   // absent elements are 0: below any cut
    s = sp_wave_sum(s);
    if (lane == 0 && c < r.nchunks) csum[c] = s;
  });
  if (tid == 0) { sh.first = 0x7fffffff; sh.last = -1; }
  __syncthreads();
  // thread t owns chunks [t * per, (t + 1) * per)
  const int per = (r.nchunks + kSpThreads - 1) / kSpThreads;
  const int cb = tid * per, ce = min(cb + per, r.nchunks);
  float lm = 0.f;
  for (int c = cb; c < ce; ++c) lm += csum[c];
  unsigned lc = 0, totc;
  float total;
  sp_block_scan(lc, lm, totc, total, sh, wave, lane);
  float u = p.u[b];
  u = u >= 0.f ? u : 0.f;
  const float target = u * total;
  {
    float run = lm, ex = 0.f;
    int first = 0x7fffffff, last = -1;
    for (int c = cb; c < ce; ++c) {
      const float s = csum[c];
      if (s > 0.f) {
        last = c;
        if (first == 0x7fffffff && run + s > target) { first = c; ex = run; }
      }
      run += s;
    }
    if (first != 0x7fffffff) atomicMin(&sh.first, first);
    if (last >= 0) atomicMax(&sh.last, last);
    __syncthreads();
    if (first != 0x7fffffff && sh.first == first) sh.excl = ex;
    __syncthreads();
  }
  if (wave != 0) return;
  const bool crossing = sh.first != 0x7fffffff;
  const int sel = crossing ? sh.first : sh.last;
  int id = 0;   // a row with nothing to keep (all zeros, NaN): token 0
  if (sel >= 0) {
    float v[4]; int i0;
    sp_load(r, sel, lane, v, i0);
    float inc[4], s = 0.f;
    int hi = -1;   // this lane's last kept element
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool kept = sp_key(v[j]) >= cut;
      s += kept ? v[j] : 0.f;
      inc[j] = s;
      if (kept) hi = j;
    }
    float is = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float t = __shfl_up(is, d, 64);
      if (lane >= d) is += t;
    }
    float ex = __shfl_up(is, 1, 64);
    ex = lane ? ex : 0.f;
    int hit = -1;
    if (crossing) {
#pragma unroll
      for (int j = 3; j >= 0; --j)
        if (sp_key(v[j]) >= cut && sh.excl + (ex + inc[j]) > target) hit = j;
    }
    const unsigned long long hits = __ballot(hit >= 0), keeps = __ballot(hi >= 0);
    const int src = hits ? __builtin_ctzll(hits) : 63 - __builtin_clzll(keeps | 1ull);
    id = __shfl(i0 + (hits ? hit : max(hi, 0)), src, 64);
  }
  if (lane == 0) ((int*)p.out)[b] = id;
}

constexpr float kSpLog2e = 1.4426950408889634f;

// softmax(logits / temperature): online max and sum in one read, a second read writes.  One workgroup per row.
__global__ __launch_bounds__(kSpThreads) void sampling_softmax_kernel(const SpParams p) {
  __shared__ float s_m[kSpWaves], s_s[kSpWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  const SpRow r = sp_row(p.probs + (long long)b * p.pitch, p.V);
  const float scale = kSpLog2e / (p.temp ? p.temp[b] : p.temp_val);   // y = logit * scale: base-2 exponent
  float m = -__builtin_inff(), s = 0.f;
  sp_for_chunks(r, wave, lane, [&](int, const float (&v)[4], const int n, int) {
    float y[4], mn = m;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      y[j] = j < n ? v[j] * scale : -__builtin_inff();
      mn = fmaxf(mn, y[j]);
    }
    if (mn > -__builtin_inff()) {
      s *= exp2f(m - mn);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += exp2f(y[j] - mn);
      m = mn;
    }
  });
  const float wm = fl_wave_max(m);
  s = sp_wave_sum(wm > -__builtin_inff() ? s * exp2f(m - wm) : 0.f);
  if (lane == 0) { s_m[wave] = wm; s_s[wave] = s; }
  __syncthreads();
  float rm = -__builtin_inff(), rs = 0.f;
#pragma unroll
  for (int w = 0; w < kSpWaves; ++w) rm = fmaxf(rm, s_m[w]);
#pragma unroll
  for (int w = 0; w < kSpWaves; ++w) rs += rm > -__builtin_inff() ? s_s[w] * exp2f(s_m[w] - rm) : 0.f;
  const bool empty = !(rm > -__builtin_inff());   // every logit -inf: zeros, not NaN
  float* const out = (float*)p.out + (long long)b * p.V;
  sp_for_chunks(r, wave, lane, [&](int, const float (&v)[4], const int n, const int i0) {
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = empty ? 0.f : exp2f(v[j] * scale - rm) / rs;
    if (n == 4) {
      *reinterpret_cast<f4u*>(out + i0) = f4u{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (j < n) out[i0 + j] = o[j];
    }
  });
}

int sp_check(const FlSamplingArgs* a, const char* what, SpParams& p) {
  FL_CHECK_ARG(a != nullptr, "%s: null argument struct", what);
  FL_CHECK_ARG(a->struct_bytes == (int32_t)sizeof(FlSamplingArgs),
               "%s: struct_bytes = %d, this library's FlSamplingArgs has %d (caller built against another header)", what, (int)a->struct_bytes,
               (int)sizeof(FlSamplingArgs));
  FL_CHECK_ARG(a->batch >= 0 && a->vocab >= 1 && a->vocab <= kSpMaxVocab && a->num_rows >= 0 && a->row_pitch >= a->vocab,
               "%s: bad sizes (batch %d, vocab %d — served up to %d — rows %lld, row pitch %lld)", what, (int)a->batch, (int)a->vocab, kSpMaxVocab,
               (long long)a->num_rows, (long long)a->row_pitch);
  p.probs = a->probs; p.pitch = a->row_pitch; p.num_rows = a->num_rows; p.V = a->vocab; p.indices = a->indices;
  p.top_k = a->top_k; p.top_k_i64 = a->top_k_is_i64; p.top_k_val = a->top_k_val;
  p.top_p = a->top_p; p.top_p_val = a->top_p_val; p.min_p = a->min_p; p.min_p_val = a->min_p_val;
  p.temp = a->temperature; p.temp_val = a->temperature_val; p.u = a->u; p.mode = a->mode; p.out = a->out;
  return FL_OK;
}

template <bool kSample>
int sp_launch(const SpParams& p, const int grid, hipStream_t stream) {
  static std::atomic<unsigned char> done[64];
  const hipError_t e = fl_set_max_dynamic_lds((const void*)sampling_kernel<kSample>, kSpHistBytes, done);
  if (e != hipSuccess) {
    fl_set_error("sampling_kernel: cannot reserve %d B of LDS: %s", kSpHistBytes, hipGetErrorString(e));
    return FL_ERR_LAUNCH;
  }
  sampling_kernel<kSample><<<dim3((unsigned)grid), dim3(kSpThreads), kSpHistBytes, stream>>>(p);
  FL_CHECK_LAUNCH("sampling_kernel");
  return FL_OK;
}

}  // namespace

extern "C" int fl_sampling_softmax(const FlSamplingArgs* a, fl_stream_t stream) {
  SpParams p;
  if (const int st = sp_check(a, "fl_sampling_softmax", p)) return st;
  if (a->batch == 0) return FL_OK;
  FL_CHECK_ARG(a->probs && a->out && ((uintptr_t)a->probs % 4) == 0 && ((uintptr_t)a->out % 4) == 0 && a->num_rows >= a->batch,
               "fl_sampling_softmax: null or misaligned pointer, or fewer rows than batch");
  sampling_softmax_kernel<<<dim3((unsigned)a->batch), dim3(kSpThreads), 0, (hipStream_t)stream>>>(p);
  FL_CHECK_LAUNCH("sampling_softmax_kernel");
  return FL_OK;
}

extern "C" int fl_sampling_renorm(const FlSamplingArgs* a, fl_stream_t stream) {
  SpParams p;
  if (const int st = sp_check(a, "fl_sampling_renorm", p)) return st;
  FL_CHECK_ARG(a->mode >= FL_SAMPLING_TOP_K && a->mode <= FL_SAMPLING_JOINT, "fl_sampling_renorm: mode %d (top-k, top-p, top-k-then-p and joint are served)",
               (int)a->mode);
  if (a->batch == 0) return FL_OK;
  FL_CHECK_ARG(a->probs && a->out && ((uintptr_t)a->probs % 4) == 0 && ((uintptr_t)a->out % 4) == 0 && a->num_rows >= a->batch,
               "fl_sampling_renorm: null or misaligned pointer, or fewer rows than batch");
  return sp_launch<false>(p, a->batch, (hipStream_t)stream);
}

extern "C" int fl_sampling_sample(const FlSamplingArgs* a, fl_stream_t stream) {
  SpParams p;
  if (const int st = sp_check(a, "fl_sampling_sample", p)) return st;
  FL_CHECK_ARG(a->mode >= FL_SAMPLING_TOP_K && a->mode <= FL_SAMPLING_MIN_P, "fl_sampling_sample: unknown mode %d", (int)a->mode);
  if (a->batch == 0) return FL_OK;
  FL_CHECK_ARG(a->probs && a->out && a->u && ((uintptr_t)a->probs % 4) == 0 && a->num_rows >= 1 && (a->indices || a->num_rows >= a->batch),
               "fl_sampling_sample: null or misaligned pointer, no rows, or fewer rows than batch without indices");
  return sp_launch<true>(p, a->batch, (hipStream_t)stream);
}
