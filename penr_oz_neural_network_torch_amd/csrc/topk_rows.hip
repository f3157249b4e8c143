// pz::topk_rows — the k most likely columns of every row of fp32 logits and their log-probabilities, on
// the device: the head of classify() and of top_logprobs in score() / generate() (engine/predictor.py;
// the host rule is ops/functional.py: topk_rows_reference). 1 <= k <= min(V, kTopkMaxK = 64).
//
// Per row: idx[j] is the column of rank j under token_logprob.hip's rule, rank(t) = #{c : l_c > l_t} +
// #{c < t : l_c == l_t} (-0 == +0): descending logit, then ascending column, also across ties at the k-th
// place. The selection compares okey() images (row_core.h) and column numbers only: integers, exact.
// logprob[j] = (l_idx[j] - max) - logf(S), with max and S = sum_c __expf(l_c - max) formed by the code that
// forms them in token_logprob.hip (row_core.h: LaneRow, block_max, the wave sums and their SUMMATION ORDER),
// so logprob[:, j] has the bits of pz::token_logprob(logits, idx[:, j]). The winner's logit is
// okey_inv(its key): the logit itself except that -0 comes back as +0, which changes no bit of the result
// (with max != 0 the difference absorbs it; with max == +-0 and logf(S) != 0 the final subtraction does;
// logf(S) == 0 has one column at the maximum, itself the winner, and -0 - -0 == +0 - -0 == +0).
//
// The form is chosen by V alone (a row's bits never depend on the row count or on its neighbours):
//
//   V <= 64    16 LANES PER ROW (one DPP row), 16 rows per 256-thread workgroup; V <= 1024 WAVE PER ROW,
//              4 rows per workgroup. The row is read once into registers (lane l holds the columns l,
//              l + G, ...: at most 4 / 16). k rounds of cross-lane arg-max over (key << 32 | ~column);
//              the owner of a round's winner stores it, clears its bit in the lane's mask of live
//              registers and renews its own best. No LDS, no barriers.
//   V >  1024  WORKGROUP PER ROW, 256 threads up to 8192 columns, 1024 beyond:
//              1. maximum, and the histogram of the keys' top 12 bits (LDS integer atomics);
//              2. S, and the histogram of the next 10 bits among the keys that match so far; 3. the last
//                 10 bits: `thr` is the k-th largest key exactly, `need` >= 1 of the columns at thr are
//                 wanted besides the k - need columns above it (the radix select of the sampler:
//                 row_core.h's pick_digit);
//              4. wave w walks its contiguous share of the row's 64-column chunks in column order: a
//                 column above thr takes the next free candidate slot (one LDS integer counter: arrival
//                 order), the columns at thr are counted per wave;
//              5. the waves whose share begins before the need-th column at thr walk it again, in column
//                 order, and put the tied column of ordinal o < need into slot (k - need) + o: the ties
//                 taken are the lowest-index ones whatever the arrival order (a row of equal logits has
//                 V of them);
//              6. one wave ranks the k candidates by counting (key, then column) and stores each at its
//                 rank, so the arrival order of step 4 never shows.
//              The row is read five times (the later reads come from the caches); steps 4 and 5 issue
//              coalesced 4-byte loads, step 4 kTkLoads of them before their uses.
//
// logits rows may be strided (row stride >= V, unit column stride); idx and logprob rows may be strided
// (row stride >= k, unit column stride). No global scratch, no float atomics, nothing leaves the workgroup.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch:
//   topk_rows_lanes_kernel<16>  26 VGPRs, 0 B LDS     topk_rows_block_kernel<256>   42 VGPRs, 16,972 B LDS
//   topk_rows_lanes_kernel<64>  52 VGPRs, 0 B LDS     topk_rows_block_kernel<1024>  51 VGPRs, 17,164 B LDS
#include "row_core.h"

namespace pz {
namespace {

constexpr int kTkLoads = 8;  // chunk loads in flight per lane in the compaction walk

template <int G>
__global__ void __launch_bounds__(kRowThreads) topk_rows_lanes_kernel(TopkRowsArgs a) {
  constexpr int kPer = LaneRow<G>::kPer;
  LaneRow<G> r(a.rows);
  const int V = a.cols, lane = r.lane;

  uint32_t alive = 0u;  // bit k: column k * G + lane exists and has not been taken
  const float mx = r.load(a.logits + r.row * a.ld, V, [&](int k, int, float) { alive |= 1u << k; });
  const float lse = logf(r.sum_exp(V, mx, [](int, int, float) {}));

  auto lane_best = [&]() {  // (0: nothing left)
    unsigned long long b = 0ull;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (k * G < V) {
        const unsigned long long p = ((alive >> k) & 1u) ? pack_col(r.v[k], k * G + lane) : 0ull;
        b = p > b ? p : b;
      }
    return b;
  };
  int* __restrict__ idx = a.idx + r.row * a.idx_ld;
  float* __restrict__ logprob = a.logprob + r.row * a.logprob_ld;
  unsigned long long mine = lane_best();
  for (int j = 0; j < a.k; ++j) {
    const unsigned long long win = group_max_u64<G>(mine);
    const int c = packed_col(win);
    if (win == mine && win != 0ull) {  // the one lane that holds column c
      alive &= ~(1u << (c / G));
      if (r.live) {
        idx[j] = c;
        logprob[j] = (okey_inv(packed_key(win)) - mx) - lse;
      }
      mine = lane_best();
    }
  }
}

template <int NT>
__global__ void __launch_bounds__(NT) topk_rows_block_kernel(TopkRowsArgs a) {
  constexpr int kWaves = NT / kWave;
  static_assert(NT % kWave == 0 && kBins % NT == 0 && kMaxBins % NT == 0, "block shape");
  __shared__ int hist[kMaxBins];
  __shared__ float red_m[kWaves];
  __shared__ float red_s[kWaves];
  __shared__ int wtot[kWaves];
  __shared__ int tie_w[kWaves];
  __shared__ int sel[2];
  __shared__ int count;
  __shared__ uint32_t cand_key[kTopkMaxK];
  __shared__ int cand_col[kTopkMaxK];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int V = a.cols, K = a.k;
  const float* __restrict__ x = a.logits + row * a.ld;
  uint32_t prefix = 0u, mask = 0u;
  int krem = K;

  // 1. the maximum; the top 12 bits
  for (int b = tid; b < kMaxBins; b += NT) hist[b] = 0;
  if (tid == 0) {
    count = 0;
    sel[0] = 0;
    sel[1] = 1;  // (a row whose keys no thread's bins account for cannot be: k <= V; stay defined anyway)
  }
  __syncthreads();
  float mx = -INFINITY;
  for_strided(x, tid, NT, V, [&](int, float l) {
    mx = fmaxf(mx, l);
    atomicAdd(&hist[okey(l) >> 20], 1);
  });
  mx = block_max<NT>(mx, red_m);  // (its barrier completes the histogram)
  pick_digit<NT>(hist, wtot, sel, 20, kMaxBins, prefix, mask, krem);

  // 2. S; the next 10 bits
  for (int b = tid; b < kBins; b += NT) hist[b] = 0;
  __syncthreads();
  float s = 0.f;
  for_strided(x, tid, NT, V, [&](int, float l) {
    s += __expf(l - mx);
    const uint32_t key = okey(l);
    if ((key & mask) == prefix) atomicAdd(&hist[(key >> 10) & (kBins - 1)], 1);
  });
  wave_sums_put(s, red_s);
  __syncthreads();
  pick_digit<NT>(hist, wtot, sel, 10, kBins, prefix, mask, krem);

  // 3. the last 10 bits
  for (int b = tid; b < kBins; b += NT) hist[b] = 0;
  __syncthreads();
  for_strided(x, tid, NT, V, [&](int, float l) {
    const uint32_t key = okey(l);
    if ((key & mask) == prefix) atomicAdd(&hist[key & (kBins - 1)], 1);
  });
  __syncthreads();
  pick_digit<NT>(hist, wtot, sel, 0, kBins, prefix, mask, krem);
  const uint32_t thr = prefix;
  const int need = min(max(krem, 1), K), above = K - need;  // (1 <= krem <= K by construction)

  // 4. the columns above thr, in arrival order; the columns at thr, counted per wave
  const int chunks = (V + kWave - 1) / kWave, cpw = (chunks + kWaves - 1) / kWaves;
  const int ch0 = wave * cpw, ch1 = min(chunks, ch0 + cpw);
  int ties = 0;
  for (int ch = ch0; ch < ch1; ch += kTkLoads) {
    float l[kTkLoads];
#pragma unroll
    for (int u = 0; u < kTkLoads; ++u) {
      const int c = (ch + u) * kWave + lane;
      l[u] = (ch + u < ch1 && c < V) ? x[c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kTkLoads; ++u) {
      const int c = (ch + u) * kWave + lane;
      const bool ok = ch + u < ch1 && c < V;
      const uint32_t key = okey(l[u]);
      if (ok && key > thr) {
        const int pos = atomicAdd(&count, 1);
        if (pos < above) {  // (always: exactly `above` keys exceed thr)
          cand_key[pos] = key;
          cand_col[pos] = c;
        }
      }
      ties += __popcll(__ballot(ok && key == thr));
    }
  }
  if (lane == 0) tie_w[wave] = ties;
  __syncthreads();

  // 5. the first `need` columns at thr, by column number
  int before = 0;
  for (int w = 0; w < wave; ++w) before += tie_w[w];
  for (int ch = ch0; ch < ch1 && before < need; ++ch) {  // (wave-uniform)
    const int c = ch * kWave + lane;
    const bool tie = c < V && okey(x[c < V ? c : 0]) == thr;
    const unsigned long long m = __ballot(tie);
    const int ord = before + __popcll(m & ((1ull << lane) - 1ull));
    if (tie && ord < need) {
      cand_key[above + ord] = thr;
      cand_col[above + ord] = c;
    }
    before += __popcll(m);
  }
  __syncthreads();

  // 6. every candidate to its rank
  if (wave == 0) {
    const float lse = logf(wave_sums_fold<NT>(red_s));
    if (lane < K) {
      const uint32_t key = cand_key[lane];
      const int col = cand_col[lane];
      int rank = 0;
      for (int i = 0; i < K; ++i) {
        const uint32_t ki = cand_key[i];
        rank += (ki > key || (ki == key && cand_col[i] < col)) ? 1 : 0;
      }
      a.idx[row * a.idx_ld + rank] = col;
      a.logprob[row * a.logprob_ld + rank] = (okey_inv(key) - mx) - lse;
    }
  }
}

}  // namespace

hipError_t topk_rows(const TopkRowsArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.cols <= 0 || a.cols > kSampleMaxCols || a.k < 1 || a.k > kTopkMaxK || a.k > a.cols) return hipErrorInvalidValue;
  return launch_row_forms(topk_rows_lanes_kernel<16>, topk_rows_lanes_kernel<kWave>, topk_rows_block_kernel<256>,
                          topk_rows_block_kernel<1024>, a, s);
}

}  // namespace pz
