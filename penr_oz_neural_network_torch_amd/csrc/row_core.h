// What the per-row heads on fp32 logits share: sample_row (sample_core.h), token_logprob.hip and
// topk_rows.hip. Everything here is about a row of logits, nothing about drawing a token: the ordered key
// of a float, the (key, column) pack and its maximum, one digit of the exact radix select, and the forms
// of a row (16 lanes, a wave, a workgroup) with the launch that picks one by V alone.
//
// SUMMATION ORDER of S = sum_c __expf(l_c - max) in token_logprob and topk_rows (a function of V only; no
// float atomics, nothing leaves the workgroup), the contract behind "topk_rows has the bits of
// token_logprob". G = 16, 64, 256 or 1024 is the number of lanes / threads that share a row:
//   a. lane l adds its columns l, l + G, ... in column order: onto its first column in the register
//      forms (LaneRow::sum_exp: ceil(V / G) - 1 additions), onto 0 in the workgroup forms (for_strided:
//      ceil(V / G) additions);
//   b. the lane sums of a DPP row of 16 fold as pz_common.h's row16_reduce (xor 1, xor 2, half mirror,
//      mirror: 4 levels), G = 16 ends here; the four rows of a wave fold as (r0 + r1) + (r2 + r3)
//      (wave_sum: 2 more levels), G = 64 ends here;
//   c. workgroup forms (wave_sums_put, wave_sums_fold): the wave sums w_0 .. w_(G/64 - 1), zeros behind
//      them, fold once more as b. (4 waves: (w0 + w1) + (w2 + w3); a level that adds exact zeros does
//      not round).
// Longest chain of dependent fp32 additions: ceil(V / 16) + 3 <= 7, ceil(V / 64) + 5 <= 21,
// ceil(V / 256) + 8 <= 40 and ceil(V / 1024) + 10: all within ceil(V / 256) + 24.
#pragma once

#include <cmath>
#include <type_traits>

#include "pz_common.h"
#include "pz_kernels.h"

namespace pz {

constexpr int kSampleLoads = 16;  // loads in flight per thread
constexpr int kDigits = 3;        // key digits from the top: 12, 10 and 10 bits
constexpr int kMaxBins = 1 << 12;
constexpr int kBins = 1 << 10;
constexpr int kRowThreads = 256;  // the workgroup of the register forms (and of the narrow workgroup form)
constexpr int kRowGroupCols = 64;  // up to here 16 lanes own a row

// order-preserving image of a float: a > b (as floats, -0 == +0) <=> okey(a) > okey(b)
PZ_DEV uint32_t okey(float x) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PZ_DEV float okey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// (key << 32 | ~column): the larger logit wins, then the lower column; an existing column packs to more than 0
PZ_DEV unsigned long long pack_col(float l, int c) {
  return (static_cast<unsigned long long>(okey(l)) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(c));
}
PZ_DEV uint32_t packed_key(unsigned long long p) { return static_cast<uint32_t>(p >> 32); }
PZ_DEV int packed_col(unsigned long long p) { return static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(p)); }

// the maximum over the G lanes that share a row (xor offsets below G stay inside the group)
template <int G>
PZ_DEV unsigned long long group_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, kWave);
    v = t > v ? t : v;
  }
  return v;
}

// a fold over the G lanes that share a row; every lane of the group gets the result
template <int G, typename Op>
PZ_DEV float group_reduce(float v, Op op) {
  if constexpr (G == 16)
    return row16_reduce(v, op);
  else
    return wave_reduce(v, op);
}

template <typename T>
PZ_DEV T scan_incl(T v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const T t = __shfl_up(v, d, kWave);
    if (lane >= d) v += t;
  }
  return v;
}

// f(c, x[c]) for c = first, first + stride, ... < n, in that order: kSampleLoads loads, then their uses
template <class F>
PZ_DEV void for_strided(const float* __restrict__ x, int first, int stride, int n, F f) {
  int c = first;
  for (; static_cast<int64_t>(c) + static_cast<int64_t>(kSampleLoads - 1) * stride < n; c += kSampleLoads * stride) {
    float v[kSampleLoads];
#pragma unroll
    for (int k = 0; k < kSampleLoads; ++k) v[k] = x[c + k * stride];
#pragma unroll
    for (int k = 0; k < kSampleLoads; ++k) f(c + k * stride, v[k]);
  }
  for (; c < n; c += stride) f(c, x[c]);
}

struct KeepTarget {};  // pick_digit's target where rem is known before the pass (top-k)

// One digit of the exact radix select, by all NT threads, after the digit's histogram is complete (a barrier
// behind it): the digit of the key that holds the rem-th unit from the top (a column, or a unit of mass)
// among the keys that match `prefix` under `mask`, and how many of that digit's units are still wanted.
// Thread t owns the `per` bins below bins - t * per, descending: a prefix scan over the threads is a suffix
// count over the digits. A caller whose target depends on the row total passes target(total, rem) -> rem;
// every thread then adds all wave totals (unrolled, with selects) where otherwise it loops over the waves
// below its own: either form measured slower in the other's place. The one thread whose bins cross rem
// writes sel[0..1]; where none does (a row without units) sel stands as the caller left it. 2 barriers.
template <int NT, typename Count, class Target = KeepTarget>
PZ_DEV void pick_digit(const Count* hist, Count* wtot, Count* sel, int shift, int bins, uint32_t& prefix, uint32_t& mask,
                       Count& rem, Target target = Target{}) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int per = bins / NT, top = bins - 1 - tid * per;
  Count mine = 0;
  for (int j = 0; j < per; ++j) mine += hist[top - j];
  Count incl = scan_incl(mine, lane);
  if (lane == kWave - 1) wtot[wave] = incl;
  __syncthreads();
  if constexpr (std::is_same<Target, KeepTarget>::value) {
    for (int w = 0; w < wave; ++w) incl += wtot[w];
  } else {
    Count total = 0;
#pragma unroll
    for (int w = 0; w < NT / kWave; ++w) {
      const Count t = wtot[w];
      incl += w < wave ? t : Count(0);
      total += t;
    }
    rem = target(total, rem);
  }
  Count run = incl - mine;
  if (run < rem && rem <= incl) {  // exactly one thread
    for (int j = 0; j < per; ++j) {
      const Count h = hist[top - j];
      if (run + h >= rem) {
        sel[0] = static_cast<Count>(top - j);
        sel[1] = rem - run;
        break;
      }
      run += h;
    }
  }
  __syncthreads();
  prefix |= static_cast<uint32_t>(sel[0]) << shift;
  mask |= static_cast<uint32_t>(bins - 1) << shift;
  rem = sel[1];
}

// The register forms: G lanes per row (16: one DPP row, V <= kRowGroupCols; 64: the wave,
// V <= kTokenLogprobWaveCols), kRowThreads / G rows per workgroup; lane l holds the columns l, l + G, ...
// (at most kPer) in v. No LDS, no barriers, the row is read once.
template <int G>
struct LaneRow {
  static constexpr int kPer = (G == 16 ? kRowGroupCols : kTokenLogprobWaveCols) / G;
  static constexpr int kRowsPerBlock = kRowThreads / G;
  float v[kPer];
  int lane;
  int64_t row;
  bool live;  // (whole groups; a dead group recomputes the last row, stores nothing)

  PZ_DEV explicit LaneRow(int64_t rows) {
    lane = threadIdx.x & (G - 1);
    const int64_t row_raw = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + threadIdx.x / G;
    live = row_raw < rows;
    row = live ? row_raw : rows - 1;
  }

  // loads the row, f(k, c, v[k]) on every column c = k * G + lane the lane holds; the row maximum
  template <class F>
  PZ_DEV float load(const float* __restrict__ x, int V, F f) {
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      v[k] = -INFINITY;
      if (k * G < V) {  // wave-uniform
        const int c = k * G + lane;
        if (c < V) {
          v[k] = x[c];
          f(k, c, v[k]);
        }
        mx = fmaxf(mx, v[k]);
      }
    }
    return group_reduce<G>(mx, OpMax{});
  }

  // S, in the SUMMATION ORDER above; f(k, c, v[k]) on every column the lane holds
  template <class F>
  PZ_DEV float sum_exp(int V, float mx, F f) const {
    float s = lane < V ? __expf(v[0] - mx) : 0.f;
    if (lane < V) f(0, lane, v[0]);
#pragma unroll
    for (int k = 1; k < kPer; ++k) {
      if (k * G >= V) break;  // wave-uniform: the columns beyond cost nothing
      const int c = k * G + lane;
      s += c < V ? __expf(v[k] - mx) : 0.f;
      if (c < V) f(k, c, v[k]);
    }
    return group_reduce<G>(s, OpAdd{});
  }
};

// The workgroup forms: NT threads per row, thread t folds the columns t, t + NT, ... (for_strided); the wave
// results meet in NT / 64 words of LDS. block_max: the maximum of every thread's mx, in every thread; one
// barrier, which also stands behind whatever LDS the caller wrote before the call.
template <int NT>
PZ_DEV float block_max(float mx, float* red) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  return wave_max(lane < NT / kWave ? red[lane] : -INFINITY);
}

// every thread's s into its wave's word; after a barrier, wave_sums_fold in any one wave gives the sum
PZ_DEV void wave_sums_put(float s, float* red) {
  s = wave_sum(s);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = s;
}
template <int NT>
PZ_DEV float wave_sums_fold(const float* red) {
  const int lane = threadIdx.x & (kWave - 1);
  return wave_sum(lane < NT / kWave ? red[lane] : 0.f);
}

// the form by V alone (a row's bits never depend on the row count or on its neighbours): 16 lanes per row
// up to kRowGroupCols columns, a wave up to kTokenLogprobWaveCols, 256 threads up to kSampleNarrowCols
// (as the sampler), 1024 beyond
template <class Args>
hipError_t launch_row_forms(void (*lanes16)(Args), void (*lanes64)(Args), void (*block256)(Args), void (*block1024)(Args),
                            const Args& a, hipStream_t s) {
  auto blocks = [&](int rows_per_block) { return dim3(static_cast<unsigned>((a.rows + rows_per_block - 1) / rows_per_block)); };
  if (a.cols <= kRowGroupCols)
    hipLaunchKernelGGL(lanes16, blocks(LaneRow<16>::kRowsPerBlock), dim3(kRowThreads), 0, s, a);
  else if (a.cols <= kTokenLogprobWaveCols)
    hipLaunchKernelGGL(lanes64, blocks(LaneRow<kWave>::kRowsPerBlock), dim3(kRowThreads), 0, s, a);
  else if (a.cols <= kSampleNarrowCols)
    hipLaunchKernelGGL(block256, blocks(1), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(block1024, blocks(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

}  // namespace pz
