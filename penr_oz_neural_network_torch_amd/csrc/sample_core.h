// pz::sample_row — steps 1-3c of the sampling rule described in sample.hip (row maximum, exact top-k
// threshold, min-p, nucleus threshold, segment sums, prefix scan and the walk), as one device function shared by
// sample_rows_kernel (logits in global memory, one call per launch) and generate_resident_kernel
// (logits in LDS, one call per token of a loop). One code, one set of instructions: the same logits,
// scalars and (row, key) give the same token in both.
//
// Every thread of the NT-thread workgroup calls it (it holds __syncthreads()); there is no early
// return, so a loop may call it again. The token comes back in every lane of wave 0 (in every thread
// when temperature == 0); the other waves' return value is meaningless. A caller that repeats the call
// puts a barrier between two calls: the greedy path reads best_w after its only barrier, and the next
// call's first write goes to best_w.
#pragma once

#include "row_core.h"

namespace pz {

constexpr int kSegments = 64;      // one per lane of the selecting wave
constexpr int kSampleMaxWaves = 16;
constexpr int kMassBins = 1 << 11;  // 64-bit bins in hist; nucleus digits from the top: 11, 11 and 10 bits

// the LDS a workgroup needs for one row (16.5 KiB), wherever the kernel keeps it. The nucleus select
// (64-bit masses) runs after the maximum and the top-k select are done with their words and re-uses them.
struct alignas(16) SampleScratch {
  union {
    unsigned long long best_w[kSampleMaxWaves];
    unsigned long long wtot64[kSampleMaxWaves];
  };
  union {
    int hist[kMaxBins];
    unsigned long long hist64[kMassBins];
  };
  union {
    int wtot[kSampleMaxWaves];
    unsigned long long sel64[2];
  };
  int sel[2];
  int lastk_w[kSampleMaxWaves];
  float segsum[kSegments];
};
static_assert(sizeof(SampleScratch) == kSampleScratchBytes, "pz_kernels.h: kSampleScratchBytes");
static_assert(sizeof(int) * kMaxBins == sizeof(unsigned long long) * kMassBins, "hist as 64-bit bins");

// kMinP false: the weigher of a call without min-p, with no trace of it in the instructions
template <bool kMinP>
struct Weigher {
  float mx, temperature, min_p;
  uint32_t thr;
  PZ_DEV float operator()(float l, bool& kept) const {
    kept = okey(l) >= thr;
    const float w = kept ? __expf((l - mx) / temperature) : 0.f;
    if (kMinP && w < min_p) kept = false;
    return kept ? w : 0.f;
  }
};

// 2b. the nucleus threshold: the largest key t such that the kept columns with key >= t hold at least
// top_p of the kept mass; columns with key >= t stay (ties at t all stay, the maximum always stays).
// The top-k select with mass where it counts columns: a column weighs m_c = floor(w_c * 2^32) as an
// integer (w_c <= 1 and V <= 2^30, so a row's total stays under 2^63), the histograms add integers
// (ds_add_u64: no order enters, so no float atomics and the same bits every time), and the target is
// ceil(top_p * total) in [1, total], which exactly one thread's bins cross in every digit pass.
// weigh: the top-k threshold and min_p, nucleus off. Every thread calls it; 4 barriers per digit.
template <int NT>
PZ_DEV uint32_t nucleus_key(const float* __restrict__ x, int V, const Weigher<true>& weigh, float top_p, SampleScratch& sm) {
  static_assert(kMassBins % NT == 0, "block shape");
  const int tid = threadIdx.x;
  uint32_t prefix = 0u, mask = 0u;
  unsigned long long rem = 0ull;
#pragma unroll
  for (int d = 0; d < kDigits; ++d) {
    const int shift = d == 0 ? 21 : d == 1 ? 10 : 0, bins = d == 2 ? kBins : kMassBins;
    for (int b = tid; b < bins; b += NT) sm.hist64[b] = 0ull;
    // a row without mass (all NaN) has no finder: digit 0 and rem 0 then stand through every pass. Only before
    // the first pass: later passes' readers of sel64 have no barrier between their read and this point.
    if (d == 0 && tid == 0) sm.sel64[0] = sm.sel64[1] = 0ull;
    __syncthreads();
    for_strided(x, tid, NT, V, [&](int, float l) {
      const uint32_t k = okey(l);
      if ((k & mask) == prefix) {
        bool kept = false;
        const float w = weigh(l, kept);
        const unsigned long long m = w > 0.f ? static_cast<unsigned long long>(w * 0x1p32f) : 0ull;
        if (m != 0ull) atomicAdd(&sm.hist64[(k >> shift) & (bins - 1)], m);
      }
    });
    __syncthreads();
    // the target, once the first pass knows the row's mass (no thread's bins cross it when total == 0)
    auto target = [&](unsigned long long total, unsigned long long r) {
      if (d != 0) return r;
      const double want = ceil(static_cast<double>(top_p) * static_cast<double>(total));
      r = want >= static_cast<double>(total) ? total : static_cast<unsigned long long>(want);
      return r < 1ull ? 1ull : r;
    };
    pick_digit<NT>(sm.hist64, sm.wtot64, sm.sel64, shift, bins, prefix, mask, rem, target);
  }
  return prefix;
}

// x: the row's V fp32 logits (global memory or LDS); urow = row0 + row; key = layer_key(seed, step);
// top_p >= 1 and min_p == 0: off. kNucleus false ignores both: the kernels instantiate that form for
// calls without the options, so such a call runs the instructions it ran before the options existed.
template <int NT, bool kNucleus>
PZ_DEV int sample_row(const float* __restrict__ x, int V, float temperature, int top_k, float top_p, float min_p,
                      uint32_t urow, uint32_t key, SampleScratch& sm) {
  constexpr int kWaves = NT / kWave;
  static_assert(NT % kWave == 0 && kWaves <= kSampleMaxWaves && kBins % NT == 0 && kMaxBins % NT == 0, "block shape");
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;

  // 1. row maximum and the lowest index among the maxima
  unsigned long long best = 0ull;
  for_strided(x, tid, NT, V, [&](int c, float l) {
    const unsigned long long p = pack_col(l, c);
    best = p > best ? p : best;
  });
  best = group_max_u64<kWave>(best);
  if (lane == 0) sm.best_w[wave] = best;
  __syncthreads();
  best = sm.best_w[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) best = sm.best_w[w] > best ? sm.best_w[w] : best;
  const uint32_t kmax = packed_key(best);
  const int argmax = packed_col(best);

  int token = argmax;
  if (temperature > 0.f) {
    // 2. the k-th largest key, exactly
    uint32_t thr = 0u;
    if (top_k > 0 && top_k < V) {
      uint32_t prefix = 0u, mask = 0u;
      int krem = top_k;
#pragma unroll
      for (int d = 0; d < kDigits; ++d) {
        const int shift = d == 0 ? 20 : d == 1 ? 10 : 0, bins = d == 0 ? kMaxBins : kBins;
        for (int b = tid; b < bins; b += NT) sm.hist[b] = 0;
        __syncthreads();
        for_strided(x, tid, NT, V, [&](int, float l) {
          const uint32_t k = okey(l);
          if ((k & mask) == prefix) atomicAdd(&sm.hist[(k >> shift) & (bins - 1)], 1);
        });
        __syncthreads();
        pick_digit<NT>(sm.hist, sm.wtot, sm.sel, shift, bins, prefix, mask, krem);
      }
      thr = prefix;
    }

    // 2b. min-p is a condition of the weigher; the nucleus raises the threshold key (workgroup-uniform)
    if (kNucleus && top_p < 1.f) {
      const uint32_t t = nucleus_key<NT>(x, V, Weigher<true>{okey_inv(kmax), temperature, min_p, thr}, top_p, sm);
      thr = t > thr ? t : thr;
    }

    // 3a. segment sums
    const Weigher<kNucleus> weigh{okey_inv(kmax), temperature, min_p, thr};
    const int chunks = (V + kWave - 1) / kWave;
    const int segch = (chunks + kSegments - 1) / kSegments;
    // a wave owns kOwn consecutive segments and walks them side by side, kStep chunks of each per round
    // (kSampleLoads loads in flight); every (segment, lane) sum still adds its chunks in chunk order
    constexpr int kOwn = kSegments / kWaves, kStep = kSampleLoads / kOwn;
    static_assert(kOwn * kWaves == kSegments && kStep * kOwn == kSampleLoads, "segments per wave");
    int lastk = -1;
    float p[kOwn];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) p[k] = 0.f;
    for (int i0 = 0; i0 < segch; i0 += kStep) {
      float l[kOwn][kStep];
      int col[kOwn][kStep];  // -1: no such column
#pragma unroll
      for (int k = 0; k < kOwn; ++k)
#pragma unroll
        for (int j = 0; j < kStep; ++j) {
          const int64_t c = (static_cast<int64_t>(wave * kOwn + k) * segch + i0 + j) * kWave + lane;
          col[k][j] = i0 + j < segch && c < V ? static_cast<int>(c) : -1;
          l[k][j] = col[k][j] >= 0 ? x[col[k][j]] : 0.f;
        }
#pragma unroll
      for (int k = 0; k < kOwn; ++k)
#pragma unroll
        for (int j = 0; j < kStep; ++j) {
          bool kept = false;
          const float w = col[k][j] >= 0 ? weigh(l[k][j], kept) : 0.f;
          p[k] += w;  // (+ 0 where there is no column: exact)
          if (kept) lastk = max(lastk, col[k][j]);
        }
    }
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
      const float total = wave_sum(p[k]);
      if (lane == 0) sm.segsum[wave * kOwn + k] = total;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lastk = max(lastk, __shfl_xor(lastk, o, kWave));
    if (lane == 0) sm.lastk_w[wave] = lastk;
    __syncthreads();
    if (wave == 0) {  // (no barrier below)
      // 3b. segment prefixes and the draw
      const float P = scan_incl(sm.segsum[lane], lane);
      const float S = __shfl(P, kWave - 1, kWave);
      const float u = static_cast<float>(mix32(urow ^ key) >> 8) * 0x1p-24f;
      const float target = u * S;
      token = sm.lastk_w[0];  // the last kept column: where a walk that runs off the row ends
#pragma unroll
      for (int w = 1; w < kWaves; ++w) token = max(token, sm.lastk_w[w]);
      if (token < 0) token = argmax;  // (a row of NaNs)
      const unsigned long long over = __ballot(P > target);
      if (over != 0ull) {
        // 3c. the walk (the next chunk's logits are loaded before this chunk's scan)
        const int s = __ffsll(over) - 1;
        float R = __shfl(P, s > 0 ? s - 1 : 0, kWave);
        if (s == 0) R = 0.f;
        int ch = s * segch;
        float l = ch * kWave + lane < V ? x[ch * kWave + lane] : 0.f;
        for (; ch < chunks; ++ch) {
          const int c = ch * kWave + lane;
          const float lnext = ch + 1 < chunks && c + kWave < V ? x[c + kWave] : 0.f;
          bool kept = false;
          const float w = c < V ? weigh(l, kept) : 0.f;
          kept = kept && c < V;
          const float incl = scan_incl(w, lane);
          const unsigned long long hit = __ballot(kept && R + incl > target);
          if (hit != 0ull) {
            token = ch * kWave + __ffsll(hit) - 1;
            break;
          }
          R += __shfl(incl, kWave - 1, kWave);
          l = lnext;
        }
      }
    }
  }
  return token;
}

}  // namespace pz
