// pz::sample_rows — draw one token per row from fp32 logits, on the device: the head of the
// generation loop (engine/predictor.py: FusedPredictor.generate). Greedy (temperature 0) or
// temperature / top-k / min-p / top-p (nucleus) sampling by inverse CDF with a counter-based uniform, so a (seed, row, step)
// names its draw and the host can reproduce it (ops/functional.py: sample_uniform,
// sample_rows_reference).
//
// One workgroup owns a row (4 waves up to 8192 columns, 16 beyond: a function of V only);
// workgroups never talk to each other (no tickets, no global atomics, no global scratch). Per row
// (steps 1-3c are sample_core.h's sample_row, which the one-launch generation kernel of
// generate_resident.hip calls too):
//
//  1. max: every thread folds key(l_c) << 32 | ~c over its columns (key = the order-preserving
//     uint32 image of the fp32 bits, -0 read as +0), shuffles, then the wave results through LDS:
//     the row maximum and the lowest index holding it. temperature == 0 stops here.
//  2. top-k threshold (0 < top_k < V): an exact radix select on the keys, digits of 12, 10 and 10
//     bits from the top, each pass an LDS histogram of the columns that match the digits found so
//     far and a suffix scan over the bins (row_core.h: pick_digit; 12 bits first: sign, exponent and 3
//     mantissa bits spread logits of one octave over 8 bins: short same-address LDS atomics). Integer
//     arithmetic only: the k-th largest key comes out exactly, columns with key >= it are kept
//     (ties at the threshold all stay).
//  2b. min-p (0 < min_p < 1) drops the kept columns with w_c < min_p; top-p (0 < top_p < 1) then keeps
//     the columns whose strictly-more-likely columns hold less than top_p of the mass that is left:
//     the same radix select with mass where top-k counts columns (digits of 11, 11 and 10 bits, 64-bit
//     integer LDS adds of floor(w_c * 2^32): no float atomics, the same bits every time; sample_core.h:
//     nucleus_key). Ties at the threshold all stay, the maximum always stays.
//  3. weights w_c = exp((l_c - max) / T) on kept columns, 0 elsewhere, recomputed where needed (the
//     same instructions give the same bits). The row is cut into chunks of 64 consecutive columns
//     and into 64 segments of `segch` = ceil(chunks / 64) consecutive chunks.
//     SUMMATION ORDER (a function of V only; which wave sums a segment does not enter):
//       a. segment sum: lane l adds its column of each of the segment's chunks in chunk order
//          (segch - 1 additions), then the 64 lane sums fold as pz_common.h's wave_sum tree (6 levels);
//       b. the 64 segment sums are scanned (Hillis-Steele over lanes, 6 levels; a level that adds the
//          exact zero of an empty segment does not round): P_s, and S = P_63;
//       c. the walk starts at R = P_(s-1) for the first segment s with P_s > u * S and visits chunks
//          in order: an inclusive lane scan of the chunk's weights (6 levels) gives the prefix
//          R + incl_l; the first kept lane whose prefix exceeds u * S is the token, else R += the
//          chunk total (one addition per chunk).
//     Longest chain of dependent rounding additions: (segch - 1) + 6 + min(6, ceil(log2(chunks)))
//     for P, plus segch + 6 for the walk = 2 * ceil(V / 4096) + 11 + min(6, ceil(log2(ceil(V / 64))))
//     <= V / 64 + 16 for every V (13 at V <= 64, 19 at V = 4096, 49 at V = 65536).
//     P and the walk's running sum associate differently, so the walk may reach the end of segment
//     s a rounding short of u * S; it then simply goes on into the next chunks, and a walk that runs
//     off the row takes the last kept column.
//  4. the token goes to seq[row, pos] (one ordinary 8-byte store by lane 0), done[row] is set when
//     it equals stop_token; a row already done writes stop_token and touches nothing else.
//
// A row's token depends on its logits, row0 + row, key and the scalars only: not on the row count.
// Loads are 4-byte and coalesced, issued kSampleLoads at a time before their use (a row is read by one
// workgroup, so it is the loads in flight, not bandwidth, that set the time of a pass).
//
// Every width is built twice: <NT, false> for calls without top-p / min-p (the instructions of the
// kernel before those options existed) and <NT, true> for calls with either: a call without the
// options must cost what it cost before, and one kernel with a run-time branch measured 0.2 us more
// at V = 4096. Resources (hipcc -O3
// --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), all with 16,912 B of LDS and no scratch:
//   <256, false> 92 VGPRs   <256, true> 90 VGPRs   <1024, false> 78 VGPRs   <1024, true> 81 VGPRs
#include "sample_core.h"

namespace pz {
namespace {

constexpr int kWideFrom = kSampleNarrowCols;  // columns beyond which a row gets 16 waves instead of 4

// kNucleus: the call has top_p < 1 or min_p > 0 (sample_core.h)
template <int NT, bool kNucleus>
__global__ void __launch_bounds__(NT) sample_rows_kernel(SampleArgs a) {
  __shared__ SampleScratch sm;
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  int64_t* out = a.seq + static_cast<int64_t>(row) * a.seq_ld + a.pos;
  if (a.done[row] != 0) {  // block-uniform
    if (tid == 0) *out = a.stop_token;
    return;
  }
  const float* __restrict__ x = a.logits + static_cast<int64_t>(row) * a.cols;
  const int token = sample_row<NT, kNucleus>(x, a.cols, a.temperature, a.top_k, a.top_p, a.min_p, a.row0 + static_cast<uint32_t>(row), a.key, sm);
  if (tid == 0) {
    *out = token;
    if (token == a.stop_token) a.done[row] = 1;
  }
}

}  // namespace

hipError_t sample_rows(const SampleArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.cols <= 0 || a.cols > kSampleMaxCols) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(a.rows));
  const bool nucleus = a.top_p < 1.f || a.min_p > 0.f;
  if (a.cols > kWideFrom) {
    if (nucleus)
      hipLaunchKernelGGL((sample_rows_kernel<1024, true>), grid, dim3(1024), 0, s, a);
    else
      hipLaunchKernelGGL((sample_rows_kernel<1024, false>), grid, dim3(1024), 0, s, a);
  } else {
    if (nucleus)
      hipLaunchKernelGGL((sample_rows_kernel<256, true>), grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((sample_rows_kernel<256, false>), grid, dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace pz
