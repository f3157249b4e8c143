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
//             row_core.h orders them); counted in integers (the register forms fold the lane counts,
//             at most 1024 in all, as exact small floats through the DPP folds); 0 is the column greedy
//             sampling picks;
//   S       = sum_c exp(l_c - max) with __expf (a -inf column gives exactly 0);
//   logprob = (l_t - max) - logf(S): the target's weight is never formed, so a target 160 below the
//             maximum gives about -160 and a -inf target gives -inf.
// S is summed in row_core.h's SUMMATION ORDER, a function of V only.
//
// logits rows may be strided (row stride >= V, unit column stride); targets, logprob and rank take any
// element stride. Loads are 4-byte and coalesced (a 27-column row is not 16-B aligned), the workgroup
// forms issue kSampleLoads of them before their uses, as the sampler does.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch:
//   token_logprob_lanes_kernel<16>  18 VGPRs, 0 B LDS     token_logprob_block_kernel<256>   31 VGPRs, 48 B LDS
//   token_logprob_lanes_kernel<64>  32 VGPRs, 0 B LDS     token_logprob_block_kernel<1024>  29 VGPRs, 192 B LDS
#include "row_core.h"

namespace pz {
namespace {

PZ_DEV int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

struct OpOrBits {
  PZ_DEV float operator()(float a, float b) const { return __int_as_float(__float_as_int(a) | __float_as_int(b)); }
};

// the rank rule: does column c with logit l stand before the target ti with logit lt?
PZ_DEV int lp_before(float l, int c, float lt, int ti) { return (l > lt || (l == lt && c < ti)) ? 1 : 0; }

PZ_DEV void lp_store(const TokenLogprobArgs& a, int64_t row, bool valid, float lt, float mx, float s, int rank) {
  a.logprob[row * a.logprob_stride] = valid ? (lt - mx) - logf(s) : __int_as_float(0x7FC00000);
  if (a.rank != nullptr) a.rank[row * a.rank_stride] = valid ? rank : -1;
}

template <int G>
__global__ void __launch_bounds__(kRowThreads) token_logprob_lanes_kernel(TokenLogprobArgs a) {
  LaneRow<G> r(a.rows);
  const int V = a.cols;
  const int64_t t = a.targets[r.row * a.targets_stride];
  const bool valid = t >= 0 && t < V;
  const int ti = valid ? static_cast<int>(t) : -1;

  float ltb = 0.f;
  const float mx = r.load(a.logits + r.row * a.ld, V, [&](int, int c, float l) {
    if (c == ti) ltb = l;
  });
  const float lt = group_reduce<G>(ltb, OpOrBits{});  // one lane holds the bits, the others 0
  int cnt = 0;
  const float s = r.sum_exp(V, mx, [&](int, int c, float l) { cnt += lp_before(l, c, lt, ti); });
  const int rank = static_cast<int>(group_reduce<G>(static_cast<float>(cnt), OpAdd{}));
  if (r.live && r.lane == 0) lp_store(a, r.row, valid, lt, mx, s, rank);
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
    cnt += lp_before(l, c, lt, ti);
  });
  const int wcnt = wave_sum_i(cnt);
  if (lane == 0) red_c[wave] = wcnt;
  mx = block_max<NT>(mx, red_m);
  const int rank = wave_sum_i(lane < kWaves ? red_c[lane] : 0);

  float s = 0.f;
  for_strided(x, tid, NT, V, [&](int, float l) { s += __expf(l - mx); });
  wave_sums_put(s, red_s);
  __syncthreads();
  if (wave == 0) {
    s = wave_sums_fold<NT>(red_s);
    if (lane == 0) lp_store(a, row, valid, lt, mx, s, rank);
  }
}

}  // namespace

hipError_t token_logprob(const TokenLogprobArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.cols <= 0 || a.cols > kSampleMaxCols) return hipErrorInvalidValue;
  return launch_row_forms(token_logprob_lanes_kernel<16>, token_logprob_lanes_kernel<kWave>, token_logprob_block_kernel<256>,
                          token_logprob_block_kernel<1024>, a, s);
}

}  // namespace pz
