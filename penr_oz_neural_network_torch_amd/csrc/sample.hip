// pz::sample_rows — draw one token per row from fp32 logits, on the device: the head of the
// generation loop (engine/predictor.py: FusedPredictor.generate). Greedy (temperature 0) or
// temperature / top-k sampling by inverse CDF with a counter-based uniform, so a (seed, row, step)
// names its draw and the host can reproduce it (ops/functional.py: sample_uniform,
// sample_rows_reference).
//
// One workgroup owns a row (4 waves up to 8192 columns, 16 beyond: a function of V only);
// workgroups never talk to each other (no tickets, no global atomics, no global scratch). Per row:
//
//  1. max: every thread folds key(l_c) << 32 | ~c over its columns (key = the order-preserving
//     uint32 image of the fp32 bits, -0 read as +0), shuffles, then the wave results through LDS:
//     the row maximum and the lowest index holding it. temperature == 0 stops here.
//  2. top-k threshold (0 < top_k < V): an exact radix select on the keys, digits of 12, 10 and 10
//     bits from the top, each pass an LDS histogram of the columns that match the digits found so
//     far and a suffix scan over the bins (12 bits first: sign, exponent and 3 mantissa bits spread
//     logits of one octave over 8 bins, which keeps same-address LDS atomics short). Integer
//     arithmetic only: the k-th largest key comes out exactly, columns with key >= it are kept
//     (ties at the threshold all stay).
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
// Loads are 4-byte and coalesced, issued kLoads at a time before their use (a row is read by one
// workgroup, so it is the loads in flight, not bandwidth, that set the time of a pass).
#include "pz_common.h"
#include "pz_kernels.h"

namespace pz {
namespace {

constexpr int kSegments = 64;      // one per lane of the selecting wave
constexpr int kMaxWaves = 16;
constexpr int kLoads = 16;         // loads in flight per thread
constexpr int kWideFrom = 8192;    // columns beyond which a row gets 16 waves instead of 4
constexpr int kDigits = 3;         // key digits from the top: 12, 10 and 10 bits
constexpr int kMaxBins = 1 << 12;
constexpr int kBins = 1 << 10;

// order-preserving image of a float: a > b (as floats, -0 == +0) <=> okey(a) > okey(b)
PZ_DEV uint32_t okey(float x) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PZ_DEV float okey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

template <typename T>
PZ_DEV T scan_incl(T v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const T t = __shfl_up(v, d, kWave);
    if (lane >= d) v += t;
  }
  return v;
}

// f(c, x[c]) for c = first, first + stride, ... < n (any order-free fold): kLoads loads, then their uses
template <class F>
PZ_DEV void for_strided(const float* __restrict__ x, int first, int stride, int n, F f) {
  int c = first;
  for (; static_cast<int64_t>(c) + static_cast<int64_t>(kLoads - 1) * stride < n; c += kLoads * stride) {
    float v[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) v[k] = x[c + k * stride];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) f(c + k * stride, v[k]);
  }
  for (; c < n; c += stride) f(c, x[c]);
}

struct Weigher {
  float mx, temperature;
  uint32_t thr;
  PZ_DEV float operator()(float l, bool& kept) const {
    kept = okey(l) >= thr;
    return kept ? __expf((l - mx) / temperature) : 0.f;
  }
};

template <int NT>
__global__ void __launch_bounds__(NT) sample_rows_kernel(SampleArgs a) {
  constexpr int kWaves = NT / kWave;
  static_assert(NT % kWave == 0 && kWaves <= kMaxWaves && kBins % NT == 0 && kMaxBins % NT == 0, "block shape");
  __shared__ unsigned long long best_w[kMaxWaves];
  __shared__ int hist[kMaxBins];
  __shared__ int wtot[kMaxWaves];
  __shared__ int sel[2];
  __shared__ int lastk_w[kMaxWaves];
  __shared__ float segsum[kSegments];

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int row = blockIdx.x;
  const int V = a.cols;
  int64_t* out = a.seq + static_cast<int64_t>(row) * a.seq_ld + a.pos;
  if (a.done[row] != 0) {  // block-uniform
    if (tid == 0) *out = a.stop_token;
    return;
  }
  const float* __restrict__ x = a.logits + static_cast<int64_t>(row) * V;

  // 1. row maximum and the lowest index among the maxima
  unsigned long long best = 0ull;
  for_strided(x, tid, NT, V, [&](int c, float l) {
    const unsigned long long p = (static_cast<unsigned long long>(okey(l)) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(c));
    best = p > best ? p : best;
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(best, o, kWave);
    best = t > best ? t : best;
  }
  if (lane == 0) best_w[wave] = best;
  __syncthreads();
  best = best_w[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) best = best_w[w] > best ? best_w[w] : best;
  const uint32_t kmax = static_cast<uint32_t>(best >> 32);
  const int argmax = static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(best));

  int token = argmax;
  if (a.temperature > 0.f) {
    // 2. the k-th largest key, exactly
    uint32_t thr = 0u;
    if (a.top_k > 0 && a.top_k < V) {
      uint32_t prefix = 0u, mask = 0u;
      int krem = a.top_k;
#pragma unroll
      for (int d = 0; d < kDigits; ++d) {
        const int shift = d == 0 ? 20 : d == 1 ? 10 : 0, bins = d == 0 ? kMaxBins : kBins, per = bins / NT;
        for (int b = tid; b < bins; b += NT) hist[b] = 0;
        __syncthreads();
        for_strided(x, tid, NT, V, [&](int, float l) {
          const uint32_t k = okey(l);
          if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & (bins - 1)], 1);
        });
        __syncthreads();
        // thread t owns the `per` bins below bins - t * per, descending: a prefix scan over the threads is
        // a suffix count over the digits
        const int top = bins - 1 - tid * per;
        int mine = 0;
        for (int j = 0; j < per; ++j) mine += hist[top - j];
        int incl = scan_incl(mine, lane);
        if (lane == kWave - 1) wtot[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += wtot[w];
        int run = incl - mine;
        if (run < krem && krem <= incl) {  // exactly one thread: it holds the digit of the k-th largest
          for (int j = 0; j < per; ++j) {
            const int h = hist[top - j];
            if (run + h >= krem) {
              sel[0] = top - j;
              sel[1] = krem - run;
              break;
            }
            run += h;
          }
        }
        __syncthreads();
        prefix |= static_cast<uint32_t>(sel[0]) << shift;
        mask |= static_cast<uint32_t>(bins - 1) << shift;
        krem = sel[1];
      }
      thr = prefix;
    }

    // 3a. segment sums
    const Weigher weigh{okey_inv(kmax), a.temperature, thr};
    const int chunks = (V + kWave - 1) / kWave;
    const int segch = (chunks + kSegments - 1) / kSegments;
    // a wave owns kOwn consecutive segments and walks them side by side, kStep chunks of each per round
    // (kLoads loads in flight); every (segment, lane) sum still adds its chunks in chunk order
    constexpr int kOwn = kSegments / kWaves, kStep = kLoads / kOwn;
    static_assert(kOwn * kWaves == kSegments && kStep * kOwn == kLoads, "segments per wave");
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
      if (lane == 0) segsum[wave * kOwn + k] = total;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lastk = max(lastk, __shfl_xor(lastk, o, kWave));
    if (lane == 0) lastk_w[wave] = lastk;
    __syncthreads();
    if (wave != 0) return;  // (no barrier below)

    // 3b. segment prefixes and the draw
    const float P = scan_incl(segsum[lane], lane);
    const float S = __shfl(P, kWave - 1, kWave);
    const float u = static_cast<float>(mix32((a.row0 + static_cast<uint32_t>(row)) ^ a.key) >> 8) * 0x1p-24f;
    const float target = u * S;
    token = lastk_w[0];  // the last kept column: where a walk that runs off the row ends
#pragma unroll
    for (int w = 1; w < kWaves; ++w) token = max(token, lastk_w[w]);
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
  if (a.cols > kWideFrom)
    hipLaunchKernelGGL(sample_rows_kernel<1024>, grid, dim3(1024), 0, s, a);
  else
    hipLaunchKernelGGL(sample_rows_kernel<256>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace pz
