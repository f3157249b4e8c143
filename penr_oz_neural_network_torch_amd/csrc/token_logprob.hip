// pz::token_logprob — the log-probability and the rank of one given token per row of fp32 logits, on
// the device: the head of sequence scoring (engine/predictor.py: FusedPredictor.score; the host rule
// is ops/functional.py: token_logprob_reference). Where the sampler (sample.hip) sees few rows of any
// width, scoring sees every position of every sequence, often at a tiny vocabulary, so the row kernel
// has several forms, chosen by V alone (a row's bits never depend on the row count or on its neighbours):
//
//   V <= 64    16 LANES PER ROW (one DPP row): 4 rows per wave, 16 per 256-thread workgroup; lane l of
//              the group holds the columns l, l + 16, ... (at most 4) in registers.
//   V <= 1024  WAVE PER ROW: 4 rows per workgroup; lane l holds the columns l, l + 64, ... (at most 16).
//              Both: no LDS, no barriers, cross-lane folds, the row is read once; the target's logit is
//              taken from the registers (an OR-fold of its bits), so the loads of the target id and of
//              the row do not wait for each other.
//   V >  1024  WORKGROUP PER ROW: 256 threads up to 8192 columns, 1024 beyond (as the sampler); thread t
//              reads the columns t, t + NT, ... twice (the maximum and the rank first, the sum second:
//              the second read comes from the caches); the wave results meet in LDS behind one barrier
//              per pass.
//
// Per row, with target t and l_t = x[t] (a target outside [0, V) reads nothing through it, writes
// logprob = NaN and rank = -1):
//   max     = the row maximum (fmaxf folds: order-free);
//   rank    = #{c : l_c > l_t} + #{c < t : l_c == l_t}, float comparisons (-0 == +0, as okey of
//             sample_core.h orders them); counted in integers (the register forms fold the lane counts,
//             at most 1024 in all, as exact small floats through the DPP folds); 0 is the column greedy
//             sampling picks;
//   S       = sum_c exp(l_c - max) with __expf (a -inf column gives exactly 0);
//   logprob = (l_t - max) - logf(S): the target's weight is never formed, so a target 160 below the
//             maximum gives about -160 and a -inf target gives -inf.
//
// SUMMATION ORDER of S (a function of V only; no float atomics, nothing leaves the workgroup). G = 16,
// 64, 256 or 1024 is the number of lanes / threads that share a row:
//   a. lane l adds its columns l, l + G, ... in column order: onto its first column in the register
//      forms (ceil(V / G) - 1 additions), onto 0 in the workgroup forms (ceil(V / G) additions);
//   b. the lane sums of a DPP row of 16 fold as pz_common.h's row16_reduce (xor 1, xor 2, half mirror,
//      mirror: 4 levels), G = 16 ends here; the four rows of a wave fold as (r0 + r1) + (r2 + r3)
//      (wave_sum: 2 more levels), G = 64 ends here;
//   c. workgroup forms: the wave sums w_0 .. w_(G/64 - 1), zeros behind them, fold once more as b.
//      (4 waves: (w0 + w1) + (w2 + w3); a level that adds exact zeros does not round).
// Longest chain of dependent fp32 additions: ceil(V / 16) + 3 <= 7, ceil(V / 64) + 5 <= 21,
// ceil(V / 256) + 8 <= 40 and ceil(V / 1024) + 10: all within ceil(V / 256) + 24.
//
// logits rows may be strided (row stride >= V, unit column stride); targets, logprob and rank take any
// element stride. Loads are 4-byte and coalesced (a 27-column row is not 16-B aligned), the workgroup
// forms issue kSampleLoads of them before their uses, as the sampler does.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch:
//   token_logprob_lanes_kernel<16>  20 VGPRs, 0 B LDS     token_logprob_block_kernel<256>   39 VGPRs, 48 B LDS
//   token_logprob_lanes_kernel<64>  32 VGPRs, 0 B LDS     token_logprob_block_kernel<1024>  39 VGPRs, 192 B LDS
#include <cmath>

#include "sample_core.h"

namespace pz {
namespace {

constexpr int kLpThreads = 256;
constexpr int kLpGroupCols = 64;  // up to here 16 lanes own a row

PZ_DEV int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

struct OpOrBits {
  PZ_DEV float operator()(float a, float b) const { return __int_as_float(__float_as_int(a) | __float_as_int(b)); }
};

// a fold over the G lanes that share a row; every lane of the group gets the result
template <int G, typename Op>
PZ_DEV float group_reduce(float v, Op op) {
  if constexpr (G == 16)
    return row16_reduce(v, op);
  else
    return wave_reduce(v, op);
}

PZ_DEV void lp_store(const TokenLogprobArgs& a, int64_t row, bool valid, float lt, float mx, float s, int rank) {
  a.logprob[row * a.logprob_stride] = valid ? (lt - mx) - logf(s) : __int_as_float(0x7FC00000);
  if (a.rank != nullptr) a.rank[row * a.rank_stride] = valid ? rank : -1;
}

// G lanes per row (16: one DPP row, V <= 64; 64: the wave, V <= 1024); kPer columns per lane
template <int G>
__global__ void __launch_bounds__(kLpThreads) token_logprob_lanes_kernel(TokenLogprobArgs a) {
  constexpr int kPer = (G == 16 ? kLpGroupCols : kTokenLogprobWaveCols) / G;
  constexpr int kRowsPerBlock = kLpThreads / G;
  const int lane = threadIdx.x & (G - 1);
  const int64_t row_raw = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + threadIdx.x / G;
  const bool live = row_raw < a.rows;                // (whole groups; a dead group recomputes the last row, stores nothing)
  const int64_t row = live ? row_raw : a.rows - 1;
  const int V = a.cols;
  const float* __restrict__ x = a.logits + row * a.ld;
  const int64_t t = a.targets[row * a.targets_stride];
  const bool valid = t >= 0 && t < V;
  const int ti = valid ? static_cast<int>(t) : -1;

  float v[kPer];
  float mx = -INFINITY, ltb = 0.f;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    v[k] = -INFINITY;
    if (k * G < V) {  // wave-uniform
      const int c = k * G + lane;
      if (c < V) v[k] = x[c];
      mx = fmaxf(mx, v[k]);
      if (c == ti) ltb = v[k];
    }
  }
  mx = group_reduce<G>(mx, OpMax{});
  const float lt = group_reduce<G>(ltb, OpOrBits{});  // one lane holds the bits, the others 0
  float s = lane < V ? __expf(v[0] - mx) : 0.f;
  int cnt = (lane < V && (v[0] > lt || (v[0] == lt && lane < ti))) ? 1 : 0;
#pragma unroll
  for (int k = 1; k < kPer; ++k)
    if (k * G < V) {
      const int c = k * G + lane;
      s += c < V ? __expf(v[k] - mx) : 0.f;
      cnt += (c < V && (v[k] > lt || (v[k] == lt && c < ti))) ? 1 : 0;
    }
  s = group_reduce<G>(s, OpAdd{});
  const int rank = static_cast<int>(group_reduce<G>(static_cast<float>(cnt), OpAdd{}));
  if (live && lane == 0) lp_store(a, row, valid, lt, mx, s, rank);
}

template <int NT>
__global__ void __launch_bounds__(NT) token_logprob_block_kernel(TokenLogprobArgs a) {
  constexpr int kWaves = NT / kWave;
  __shared__ float red_m[kWaves];
  __shared__ int red_c[kWaves];
  __shared__ float red_s[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int V = a.cols;
  const float* __restrict__ x = a.logits + row * a.ld;
  const int64_t t = a.targets[row * a.targets_stride];
  const bool valid = t >= 0 && t < V;  // block-uniform
  const float lt = valid ? x[t] : 0.f;
  const int ti = valid ? static_cast<int>(t) : -1;

  float mx = -INFINITY;
  int cnt = 0;
  for_strided(x, tid, NT, V, [&](int c, float l) {
    mx = fmaxf(mx, l);
    cnt += (l > lt || (l == lt && c < ti)) ? 1 : 0;
  });
  mx = wave_max(mx);
  const int wcnt = wave_sum_i(cnt);
  if (lane == 0) {
    red_m[wave] = mx;
    red_c[wave] = wcnt;
  }
  __syncthreads();
  mx = wave_max(lane < kWaves ? red_m[lane] : -INFINITY);
  const int rank = wave_sum_i(lane < kWaves ? red_c[lane] : 0);

  float s = 0.f;
  for_strided(x, tid, NT, V, [&](int, float l) { s += __expf(l - mx); });
  s = wave_sum(s);
  if (lane == 0) red_s[wave] = s;
  __syncthreads();
  if (wave == 0) {
    s = wave_sum(lane < kWaves ? red_s[lane] : 0.f);
    if (lane == 0) lp_store(a, row, valid, lt, mx, s, rank);
  }
}

}  // namespace

hipError_t token_logprob(const TokenLogprobArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.cols <= 0 || a.cols > kSampleMaxCols) return hipErrorInvalidValue;
  if (a.cols <= kLpGroupCols) {
    constexpr int kRows = kLpThreads / 16;
    hipLaunchKernelGGL(token_logprob_lanes_kernel<16>, dim3(static_cast<unsigned>((a.rows + kRows - 1) / kRows)),
                       dim3(kLpThreads), 0, s, a);
  } else if (a.cols <= kTokenLogprobWaveCols) {
    constexpr int kRows = kLpThreads / kWave;
    hipLaunchKernelGGL(token_logprob_lanes_kernel<kWave>, dim3(static_cast<unsigned>((a.rows + kRows - 1) / kRows)),
                       dim3(kLpThreads), 0, s, a);
  } else if (a.cols <= kSampleNarrowCols) {
    hipLaunchKernelGGL(token_logprob_block_kernel<256>, dim3(static_cast<unsigned>(a.rows)), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(token_logprob_block_kernel<1024>, dim3(static_cast<unsigned>(a.rows)), dim3(1024), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace pz
