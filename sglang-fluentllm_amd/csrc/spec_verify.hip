// Speculative CHAIN verification on gfx950: flashinfer.sampling.verify_chain_greedy and chain_speculative_sampling_target_only
// (srt/speculative/eagle_utils.py:234,273).  Every drafted node has one child, so the accept tests of a request are independent of each
// other and the number of accepted tokens is the length of the leading run of accepted steps.
//
//   Greedy: one lane per request walks its chain (D <= 32 compares).
//
//   Sampling: grid (S, B).  A request's final token is drawn from w_i = max(q_i - p_i, 0) over ONE vocabulary row (517 KB at V = 129,280);
//   a single workgroup walking that row is bound by read latency, not bandwidth, and a verify step has at most
//   a few hundred requests for 256 CUs — so S workgroups share the row and the last one to arrive finishes it, in the same launch.
//     phase 0  every workgroup: lanes 1 .. D-1 of wave 0 gather candidate, coin and p_target(candidate); one ballot gives n, the leading
//              accepted steps; n and the rejected token go through LDS.  Slice 0 writes accept_index / accept_token_num / accepted predicts.
//     phase 1  the workgroup sums w over its slice of row n.  The row is cut at the first 16-byte aligned element of q: `head` (<= 3 scalar
//              elements, slice 0), float4 vectors, `tail` (<= 3, slice S - 1).  A slice is L4 vectors (a multiple of 512 = one
//              workgroup-wide load), wave k owns the k-th contiguous eighth and walks it 64 vectors at a time, eight 16-byte loads in
//              flight per lane (four of q + four of p; eight of q when n = D - 1, where p is not read at all).  p is read at q's element
//              index with a 4-byte aligned 16-byte load.  Lane, then wave (xor butterfly), then workgroup (wave order): a fixed order.
//     phase 2  slice sum -> workspace [B, S] (agent-scope store, acknowledged), then an agent-scope ticket add on u32 [B].  The workgroup that draws
//              S - 1 reads the S sums in slice order, picks the slice that holds u * total, and narrows inside it: the same eight-way
//              split re-summed (identical arithmetic to phase 1 on the first level) until 512 vectors remain, then one workgroup scan.
//              Where rounding leaves a running sum short of the target the last element with w > 0 is taken; all weights zero: token 0.
//              It resets the ticket to 0: a graph replay needs no memset.
// The result does not depend on the order in which the workgroups arrive.  draft_probs is only read (upstream zeroes the rejected token's
// entry in place; here that index is skipped by comparison).
#include "fl_common.h"

namespace {

constexpr int kSvThreads = 512, kSvWaves = 8, kSvMaxSlices = 512, kSvMaxDraft = 32, kSvMaxVocab = 1 << 22;
constexpr int kSvGranule = kSvThreads;   // float4 vectors of one workgroup-wide load

struct SvParams {
  int* predicts; int* accept_index; int* accept_num; long long ai_pitch;
  const int* cand; const void* tpred; int tpred_i64;
  const float* coins; const float* u_final;
  const float* q; const float* p; long long q_pb, q_pd, p_pb, p_pd;
  float thr_single, thr_acc;
  int B, D, V, S, L4;
  float* sums; unsigned* tickets;
};

__global__ __launch_bounds__(64) void spec_verify_greedy_kernel(const SvParams p) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= p.B) return;
  const int D = p.D;
  const long long base = (long long)b * D;
  auto target = [&](const int j) { return p.tpred_i64 ? (int)((const long long*)p.tpred)[base + j] : ((const int*)p.tpred)[base + j]; };
  int* const ai = p.accept_index + b * p.ai_pitch;
  int last = 0, n = 0;
  ai[0] = (int)base;
  for (int j = 1; j < D; ++j) {
    const int t = target(last);
    if (p.cand[base + j] != t) break;
    p.predicts[base + last] = t;
    ai[++n] = (int)(base + j);
    last = j;
  }
  p.predicts[base + last] = target(last);
  p.accept_num[b] = n;
}

struct __attribute__((packed, aligned(4))) SvF4u { float x, y, z, w; };   // 16-byte load at a 4-byte aligned address

// the row the final token is drawn from; p == nullptr: every step accepted, no draft row
struct SvRow { const float* q; const float* p; int V, head, nvec, tail, rej; };

__device__ __forceinline__ float sv_w(const float q, const float p, const int i, const int rej) { return i == rej ? 0.f : fmaxf(q - p, 0.f); }

__device__ __forceinline__ void sv_w4(const SvRow& r, const int v, const float4 q, const SvF4u p, float (&w)[4]) {
  const int i0 = r.head + 4 * v;
  w[0] = sv_w(q.x, p.x, i0, r.rej); w[1] = sv_w(q.y, p.y, i0 + 1, r.rej);
  w[2] = sv_w(q.z, p.z, i0 + 2, r.rej); w[3] = sv_w(q.w, p.w, i0 + 3, r.rej);
}

__device__ __forceinline__ float sv_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// sum of w over the vectors [v0, v1) by one wave: 8 loads in flight per lane
template <bool kDraft>
__device__ __forceinline__ float sv_range_sum(const SvRow& r, const int v0, const int v1, const int lane) {
  constexpr int U = kDraft ? 4 : 8;
  float acc = 0.f;
  for (int vb = v0; vb < v1; vb += 64 * U) {   // wave-uniform trip count
    float4 q[U];
    SvF4u d[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      // branch-free so that all U loads issue before the first wait: a lane past the end reloads the range's last vector and drops it below
      const int v = min(vb + 64 * k + lane, v1 - 1);
      q[k] = *reinterpret_cast<const float4*>(r.q + r.head + 4 * v);
      d[k] = SvF4u{0.f, 0.f, 0.f, 0.f};
      if constexpr (kDraft) d[k] = *reinterpret_cast<const SvF4u*>(r.p + r.head + 4 * v);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int v = vb + 64 * k + lane;
      float w[4];
      sv_w4(r, v, q[k], d[k], w);
      acc += v < v1 ? (w[0] + w[1]) + (w[2] + w[3]) : 0.f;
    }
  }
  return sv_wave_sum(acc);
}

// part[k] = sum of w over the k-th of eight contiguous pieces of `per` vectors of [lo, hi), one piece per wave
__device__ __forceinline__ void sv_eighths(const SvRow& r, const int lo, const int hi, const int per, float* part, const int wave, const int lane) {
  const int a = min(lo + wave * per, hi), e = min(a + per, hi);
  const float s = r.p ? sv_range_sum<true>(r, a, e, lane) : sv_range_sum<false>(r, a, e, lane);
  __syncthreads();   // the previous level's reads of part[] are over
  if (lane == 0) part[wave] = s;
  __syncthreads();
}

// the <= 3 scalar elements [i0, i0 + cnt) in order
__device__ __forceinline__ float sv_edge_sum(const SvRow& r, const int i0, const int cnt) {
  float s = 0.f;
  for (int j = 0; j < cnt; ++j) s += sv_w(r.q[i0 + j], r.p ? r.p[i0 + j] : 0.f, i0 + j, r.rej);
  return s;
}

// In order over n values of s[]: the first positive one whose inclusive running sum (from `run`) exceeds target, else (or when the level
// above already fell short: !crossing) the last positive one.  Returns its index (-1: none positive), run = the sum before it.
__device__ __forceinline__ int sv_pick(const float* s, const int n, const float target, float& run, bool& crossing) {
  int first = -1, last = -1;
  float acc = run, ex_first = run, ex_last = run;
  for (int k = 0; k < n; ++k) {
    const float v = s[k];
    if (v > 0.f) {
      last = k; ex_last = acc;
      if (first < 0 && crossing && acc + v > target) { first = k; ex_first = acc; }
    }
    acc += v;
  }
  if (first < 0) crossing = false;
  run = first >= 0 ? ex_first : ex_last;
  return first >= 0 ? first : last;
}

__global__ __launch_bounds__(kSvThreads) void spec_verify_sample_kernel(const SvParams p) {
  __shared__ float s_slice[kSvMaxSlices];
  __shared__ float s_part[kSvWaves + 2];   // the eight pieces, then head and tail
  __shared__ float s_wave[kSvWaves];
  __shared__ int s_n, s_rej, s_first, s_last;
  __shared__ unsigned s_ticket;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, slice = blockIdx.x, b = blockIdx.y;
  const int D = p.D, V = p.V, S = p.S;
  const long long base = (long long)b * D;

  // phase 0: the accept decisions, repeated by every workgroup of the request
  if (wave == 0) {
    bool acc = false;
    int c = -1;
    if (lane >= 1 && lane < D) {
      c = p.cand[base + lane];
      const float coin = p.coins[base + lane - 1];
      if (c >= 0 && c < V) {
        const float pt = p.q[b * p.q_pb + (lane - 1) * p.q_pd + c];
        acc = coin <= pt / fmaxf(p.thr_acc, 1e-9f) || pt >= p.thr_single;
      }
    }
    const unsigned long long accepted = __ballot(acc);
    const int n = __builtin_ctzll((~accepted >> 1) | (1ull << (D - 1)));   // leading accepted steps 1 .. D-1
    const int cr = __shfl(c, min(n + 1, 63), 64);
    if (lane == 0) { s_n = n; s_rej = n < D - 1 && cr >= 0 && cr < V ? cr : -1; }
    if (slice == 0) {
      int* const ai = p.accept_index + b * p.ai_pitch;
      if (lane == 0) { ai[0] = (int)base; p.accept_num[b] = n; }
      if (lane >= 1 && lane <= n) { p.predicts[base + lane - 1] = c; ai[lane] = (int)(base + lane); }
    }
  }
  __syncthreads();
  const int n = s_n;
  SvRow r;
  r.q = p.q + b * p.q_pb + n * p.q_pd;
  r.p = n < D - 1 ? p.p + b * p.p_pb + n * p.p_pd : nullptr;
  r.V = V; r.rej = s_rej;
  r.head = min(V, (4 - (int)(((uintptr_t)r.q >> 2) & 3)) & 3);
  r.nvec = (V - r.head) >> 2;
  r.tail = V - r.head - 4 * r.nvec;

  // phase 1: this slice's sum = head + eight pieces in wave order + tail
  auto slice_parts = [&](const int s, int& lo, int& hi) {
    lo = min(s * p.L4, r.nvec); hi = min(lo + p.L4, r.nvec);
    sv_eighths(r, lo, hi, p.L4 / kSvWaves, s_part, wave, lane);
    if (tid == 0) {
      s_part[kSvWaves] = s == 0 ? sv_edge_sum(r, 0, r.head) : 0.f;
      s_part[kSvWaves + 1] = s == S - 1 ? sv_edge_sum(r, r.head + 4 * r.nvec, r.tail) : 0.f;
    }
    __syncthreads();
  };
  auto slice_sum = [&]() {
    float s = s_part[kSvWaves];
#pragma unroll
    for (int w = 0; w < kSvWaves; ++w) s += s_part[w];
    return s + s_part[kSvWaves + 1];
  };
  int lo, hi;
  slice_parts(slice, lo, hi);
  const float mine = slice_sum();

  // phase 2: the last workgroup of the request to arrive goes on
  if (S > 1) {
    if (tid == 0) {
      __hip_atomic_store(reinterpret_cast<unsigned*>(p.sums + (long long)b * S + slice), __float_as_uint(mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // the sum is an agent-scope store (served by the memory side, not by this XCD's non-coherent L2) and is acknowledged before the
      // ticket goes out; the reader loads it the same way.  FL_SV_THREADFENCE builds the cache-wide form instead (__threadfence on
      // both sides: an L2 write-back and invalidate per workgroup, under the other workgroups' row streams) for an A/B.
#ifdef FL_SV_THREADFENCE
      __threadfence();
#else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
      s_ticket = __hip_atomic_fetch_add(p.tickets + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s_ticket != (unsigned)(S - 1)) return;
#ifdef FL_SV_THREADFENCE
    __threadfence();
#endif
    for (int s = tid; s < S; s += kSvThreads)
      s_slice[s] = __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned*>(p.sums + (long long)b * S + s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  } else if (tid == 0) {
    s_slice[0] = mine;
  }
  if (tid == 0) { s_first = 0x7fffffff; s_last = -1; }
  __syncthreads();

  float total = 0.f;
  for (int s = 0; s < S; ++s) total += s_slice[s];
  float u = p.u_final[b];
  u = u >= 0.f ? u : 0.f;
  const float target = u * total;
  float run = 0.f;
  bool crossing = true;
  const int sel = sv_pick(s_slice, S, target, run, crossing);
  int token = 0;   // all weights zero: token 0
  if (sel >= 0) {
    // inside slice `sel`: head, eight pieces, tail — the sums phase 1 made of them (recomputed unless it is this workgroup's own)
    if (sel != slice) slice_parts(sel, lo, hi);
    float order[kSvWaves + 2];
    order[0] = s_part[kSvWaves];
#pragma unroll
    for (int w = 0; w < kSvWaves; ++w) order[1 + w] = s_part[w];
    order[kSvWaves + 1] = s_part[kSvWaves + 1];
    int part = sv_pick(order, kSvWaves + 2, target, run, crossing);
    if (part == 0 || part == kSvWaves + 1) {
      // a scalar edge: every thread walks its <= 3 elements
      const int i0 = part == 0 ? 0 : r.head + 4 * r.nvec, cnt = part == 0 ? r.head : r.tail;
      int first = -1, last = -1;
      float acc = run;
      for (int j = 0; j < cnt; ++j) {
        const float w = sv_w(r.q[i0 + j], r.p ? r.p[i0 + j] : 0.f, i0 + j, r.rej);
        if (w > 0.f) {
          last = i0 + j;
          if (first < 0 && crossing && acc + w > target) first = i0 + j;
        }
        acc += w;
      }
      token = first >= 0 ? first : max(last, 0);
    } else if (part > 0) {
      int per = p.L4 / kSvWaves;
      lo = min(lo + (part - 1) * per, hi); hi = min(lo + per, hi);
      while (hi - lo > kSvGranule) {
        per = ((hi - lo + kSvWaves - 1) / kSvWaves + 63) & ~63;
        sv_eighths(r, lo, hi, per, s_part, wave, lane);
        float e[kSvWaves];
#pragma unroll
        for (int w = 0; w < kSvWaves; ++w) e[w] = s_part[w];
        part = sv_pick(e, kSvWaves, target, run, crossing);
        if (part < 0) break;   // (cannot happen: the piece above had a positive sum of the same terms; then `token` stays 0)
        lo = min(lo + part * per, hi); hi = min(lo + per, hi);
      }
      // one vector per thread: workgroup inclusive scan
      const int v = lo + tid;
      float w[4] = {0.f, 0.f, 0.f, 0.f}, inc[4];
      if (part >= 0 && v < hi) {
        const float4 q = *reinterpret_cast<const float4*>(r.q + r.head + 4 * v);
        const SvF4u d = r.p ? *reinterpret_cast<const SvF4u*>(r.p + r.head + 4 * v) : SvF4u{0.f, 0.f, 0.f, 0.f};
        sv_w4(r, v, q, d, w);
      }
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) { s += w[j]; inc[j] = s; }
      float is = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const float t = __shfl_up(is, d, 64);
        if (lane >= d) is += t;
      }
      if (lane == 63) s_wave[wave] = is;
      __syncthreads();
      float ex = run;
      for (int k = 0; k < wave; ++k) ex += s_wave[k];
      ex += is - s;
      int first = 0x7fffffff, last = -1;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        if (w[j] > 0.f) {
          last = max(last, r.head + 4 * v + j);
          if (crossing && ex + inc[j] > target) first = r.head + 4 * v + j;
        }
      }
      if (first != 0x7fffffff) atomicMin(&s_first, first);
      if (last >= 0) atomicMax(&s_last, last);
      __syncthreads();
      token = s_first != 0x7fffffff ? s_first : max(s_last, 0);
    }
  }
  if (tid == 0) {
    p.predicts[base + n] = token;
    if (S > 1) __hip_atomic_store(p.tickets + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

int sv_check(const FlSpecVerifyArgs* a, const char* what, SvParams& p) {
  FL_CHECK_ARG(a != nullptr, "%s: null argument struct", what);
  FL_CHECK_ARG(a->struct_bytes == (int32_t)sizeof(FlSpecVerifyArgs),
               "%s: struct_bytes = %d, this library's FlSpecVerifyArgs has %d (caller built against another header)", what, (int)a->struct_bytes,
               (int)sizeof(FlSpecVerifyArgs));
  FL_CHECK_ARG(a->batch >= 0 && a->batch <= 65535 && a->num_draft >= 1 && a->num_draft <= kSvMaxDraft && a->accept_index_pitch >= a->num_draft,
               "%s: bad sizes (batch %d — served up to 65535 — draft tokens %d — served 1 .. %d — accept_index pitch %lld, at least the draft tokens)", what,
               (int)a->batch, (int)a->num_draft, kSvMaxDraft, (long long)a->accept_index_pitch);
  if (a->batch == 0) return FL_OK;
  FL_CHECK_ARG(a->predicts && a->accept_index && a->accept_token_num && a->candidates, "%s: null predicts, accept_index, accept_token_num or candidates", what);
  p.predicts = a->predicts; p.accept_index = a->accept_index; p.accept_num = a->accept_token_num; p.ai_pitch = a->accept_index_pitch;
  p.cand = a->candidates; p.tpred = a->target_predict; p.tpred_i64 = a->target_predict_is_i64;
  p.coins = a->uniform_samples; p.u_final = a->uniform_final;
  p.q = a->target_probs; p.p = a->draft_probs;
  p.q_pb = a->target_pitch_b; p.q_pd = a->target_pitch_d; p.p_pb = a->draft_pitch_b; p.p_pd = a->draft_pitch_d;
  p.thr_single = a->threshold_single; p.thr_acc = a->threshold_acc;
  p.B = a->batch; p.D = a->num_draft; p.V = a->vocab; p.S = a->num_slices; p.L4 = 0;
  p.sums = a->slice_sums; p.tickets = a->tickets;
  return FL_OK;
}

}  // namespace

extern "C" int fl_spec_verify_greedy(const FlSpecVerifyArgs* a, fl_stream_t stream) {
  SvParams p;
  if (const int st = sv_check(a, "fl_spec_verify_greedy", p)) return st;
  if (a->batch == 0) return FL_OK;
  FL_CHECK_ARG(a->target_predict != nullptr, "fl_spec_verify_greedy: null target_predict");
  spec_verify_greedy_kernel<<<dim3((unsigned)((a->batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream>>>(p);
  FL_CHECK_LAUNCH("spec_verify_greedy_kernel");
  return FL_OK;
}

extern "C" int fl_spec_verify_sample(const FlSpecVerifyArgs* a, fl_stream_t stream) {
  SvParams p;
  if (const int st = sv_check(a, "fl_spec_verify_sample", p)) return st;
  FL_CHECK_ARG(a->vocab >= 1 && a->vocab <= kSvMaxVocab && a->num_slices >= 1 && a->num_slices <= kSvMaxSlices,
               "fl_spec_verify_sample: vocab %d (served 1 .. %d) or slices %d (served 1 .. %d)", (int)a->vocab, kSvMaxVocab, (int)a->num_slices, kSvMaxSlices);
  if (a->batch == 0) return FL_OK;
  FL_CHECK_ARG(a->uniform_samples && a->uniform_final && a->target_probs && a->draft_probs && ((uintptr_t)a->target_probs % 4) == 0 &&
                   ((uintptr_t)a->draft_probs % 4) == 0,
               "fl_spec_verify_sample: null or misaligned uniform_samples, uniform_final, target_probs or draft_probs");
  FL_CHECK_ARG(a->target_pitch_d >= a->vocab && a->draft_pitch_d >= a->vocab && a->target_pitch_b >= 0 && a->draft_pitch_b >= 0,
               "fl_spec_verify_sample: rows of target_probs / draft_probs overlap (pitch below the vocabulary)");
  FL_CHECK_ARG(a->num_slices == 1 || (a->slice_sums && a->tickets), "fl_spec_verify_sample: %d slices need the slice_sums and tickets workspace", (int)a->num_slices);
  // slice length in float4 vectors: the whole row (at most V / 4 vectors) over S slices, a multiple of one workgroup-wide load
  const int per = (a->vocab / 4 + a->num_slices - 1) / a->num_slices;
  p.L4 = (per + kSvGranule - 1) / kSvGranule * kSvGranule;
  if (p.L4 == 0) p.L4 = kSvGranule;
  spec_verify_sample_kernel<<<dim3((unsigned)a->num_slices, (unsigned)a->batch), dim3(kSvThreads), 0, (hipStream_t)stream>>>(p);
  FL_CHECK_LAUNCH("spec_verify_sample_kernel");
  return FL_OK;
}
