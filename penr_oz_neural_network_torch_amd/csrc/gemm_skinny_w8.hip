// Weight-only quantised skinny-batch GEMM for inference:
//     out[M,N] = act(scale[n] * (x[M,K] @ W8[K,N]) + bias[n]),   1 <= M <= 16.
//
// x is bf16, W8 is OCP e4m3 in the layers' natural [in, out] layout (N-contiguous) with one
// power-of-two scale per output column (quant_cols.hip), accumulation is fp32. The sibling of
// gemm_skinny.hip with half its weight bytes; the same contract, restated where the numbers differ:
//
//  * every lane loads 8 B of one W8 row straight to registers (8 columns, so the accumulator count
//    per bucket is the bf16 kernel's); a batch of 16 such loads (8 / 2 in the buckets with 64 / 128
//    accumulators) is issued back to back into one set of a ring of register sets (2 sets; 8 in
//    the 16-row bucket, whose batches are small), and the following batches are issued before the
//    current one is consumed: two or more batches are in flight per lane, and no register is
//    copied between sets. W8 never passes through LDS.
//  * a wave is 16 column lanes x 4 K lanes: one load instruction reads whole 128-B lines of 4 rows.
//    A 256-thread workgroup covers a strip of 128 columns and 16 K-rows per load.
//  * e4m3 -> fp32 by v_cvt_pk_f32_fp8 (two values per instruction); a bf16 x e4m3 product has at
//    most 12 significant bits and is exact in fp32, the sum is fp32 FMAs.
//  * x (<= 16 rows) is staged once per workgroup into LDS, transposed to [k][m]; the row count is a
//    compile-time bucket MB (1, 2, 4, 8, 16); rows >= M are zeros in LDS and are neither folded
//    across workgroups nor stored.
//  * K is split across the 16 K lanes of a workgroup and across workgroups (skinny_w8_plan: a
//    function of K and N only). A lane sums the rows congruent to its K lane modulo 16 in rising
//    order whatever the bucket; the 16 lane sums of each output go through LDS and are added in lane
//    order; the workgroups' fp32 slabs are folded in slice order by the last arriver of the strip's
//    ticket (pz_common.h det_ticket; write-through stores and loads, the loads of all of a
//    thread's outputs issued together, each output summed as det_fold does). No float atomics: a call is bit-reproducible, and
//    row r of a 16-row call equals that row sent alone.
//  * the folding workgroup multiplies by scale[col] (exact: a power of two), adds the fp32 bias,
//    applies act_fwd and stores bf16 / fp32.
//
// Eligibility (skinny_w8_eligible; anything else is refused on the host, never launched): W8's row
// bytes and leading dimension are multiples of 16 B and its base is 16-B aligned — the bf16
// kernel's rule in bytes, i.e. N % 16 == 0 here (the 8-B loads alone would need half of it; a
// 128-column strip then never ends inside a lane pair). x, out, scale and bias need only their
// natural alignment.
// K rows past the end are never read (load_batch clamps the row and zeroes the value).
#include <algorithm>

#include "pz_common.h"
#include "pz_launch.h"

namespace pz {

namespace {

constexpr int kThreads = 256;
constexpr int kColLanes = 16;                      // lanes of a wave along N
constexpr int kRowLanes = kThreads / kColLanes;    // K-rows a workgroup covers per load: 16
constexpr int kVec = 8;                            // columns per lane: one 8-B load
constexpr int kCols = kColLanes * kVec;            // strip width: 128 columns = one 128-B line per row
constexpr int kBatchRows = 256;                    // the plan's granule of a K slice: 16 rows per lane
constexpr int kFoldRows = 4;                       // output rows folded through LDS per round
constexpr int kMaxSlice = 1024;                    // K rows of x one workgroup stages
constexpr int kTargetGroups = 512;                 // ~2 workgroups per CU on a 256-CU chip

template <int MB>
struct W8Shape {
  static constexpr int kRound = MB < kFoldRows ? MB : kFoldRows;
  static constexpr int kRounds = MB / kRound;
  static constexpr int kOutPerRound = (kRound * kCols + kThreads - 1) / kThreads;
  static constexpr int kXsBytes = kMaxSlice * MB * 2;
  static constexpr int kRedBytes = kRowLanes * kRound * kCols * 4;
  // a ring of kSets register sets of kU loads each lives beside the MB * 8 accumulators; kSets - 1
  // batches are in flight while one is consumed: 256 B of W8 per lane in the ring (128 B with 64 or
  // 128 accumulators; 4-load batches in two sets spill in the 16-row bucket, 2-load batches in
  // eight sets do not). Which rows a lane sums, and in what order, is the same for every bucket
  static constexpr int kU = MB * kVec >= 128 ? 2 : MB * kVec >= 64 ? 8 : 16;
  static constexpr int kSets = MB * kVec >= 128 ? 8 : 2;
  static constexpr int kRows = kRowLanes * kU;     // K-rows per batch: 256, 128 or 32 (all divide kBatchRows)
  static constexpr int kLds = kXsBytes > kRedBytes ? kXsBytes : kRedBytes;
};

PZ_DEV void unpack_e4m3(const u32x2_t& r, float (&w)[kVec]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(r[i]), false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(r[i]), true);
    w[4 * i] = lo[0];
    w[4 * i + 1] = lo[1];
    w[4 * i + 2] = hi[0];
    w[4 * i + 3] = hi[1];
  }
}

// one batch: U W8 vectors of this lane, rows row0 + u * kRowLanes (row0 includes the lane's K lane).
// A row past the slice reads row k1 - 1 instead and drops the value: no out-of-bounds read and no
// branch, so a partial batch's loads still issue back to back.
template <int U>
PZ_DEV void load_batch(u32x2_t (&w)[U], const uint8_t* wp, int64_t ldw, int row0, int k1) {
#pragma unroll
  for (int u = 0; u < U; ++u)
    w[u] = *reinterpret_cast<const u32x2_t*>(wp + static_cast<int64_t>(min(row0 + u * kRowLanes, k1 - 1)) * ldw);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (row0 + u * kRowLanes >= k1) w[u] = u32x2_t{0u, 0u};
}

// the MB bf16 values of one staged x row: 16-B LDS reads where a row has that many bytes
template <int MB>
PZ_DEV void load_x(const uint16_t* xr, float (&xf)[MB]) {
  if constexpr (MB >= 8) {
#pragma unroll
    for (int i = 0; i < MB / 8; ++i) {
      const u32x4_t r = reinterpret_cast<const u32x4_t*>(xr)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xf[i * 8 + 2 * j] = __uint_as_float(r[j] << 16);
        xf[i * 8 + 2 * j + 1] = __uint_as_float(r[j] & 0xFFFF0000u);
      }
    }
  } else {
#pragma unroll
    for (int m = 0; m < MB; ++m) xf[m] = bf2f(xr[m]);
  }
}

template <int MB, int U>
PZ_DEV void consume_batch(const u32x2_t (&w)[U], const uint16_t* xs, int lrow0, float (&acc)[MB][kVec]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float wf[kVec], xf[MB];
    unpack_e4m3(w[u], wf);
    load_x<MB>(xs + (lrow0 + u * kRowLanes) * MB, xf);
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int j = 0; j < kVec; ++j) acc[m][j] = fmaf(xf[m], wf[j], acc[m][j]);
  }
}

template <int MB>
__global__ void __launch_bounds__(kThreads, 2) gemm_skinny_w8_kernel(const SkinnyW8Args a, const int slices, const int slice_len) {
  using S = W8Shape<MB>;
  constexpr int VEC = kVec, CW = kCols;
  __shared__ __attribute__((aligned(16))) char smem[S::kLds];
  uint16_t* xs = reinterpret_cast<uint16_t*>(smem);  // [slice rows, padded to whole batches][MB]
  float* red = reinterpret_cast<float*>(smem);       // [kRowLanes][kRound][CW], after the K loop
  PZ_LDS int* flag = (PZ_LDS int*)(smem);             // the ticket's verdict, after the sums left LDS

  const int tid = threadIdx.x;
  const int strip = blockIdx.x, slice = blockIdx.y;
  const int k0 = slice * slice_len;
  const int k1 = min(a.K, k0 + slice_len);
  constexpr int U = S::kU, BR = S::kRows;
  const int batches = (k1 - k0 + BR - 1) / BR;
  const int col_lane = tid & (kColLanes - 1);
  const int row_lane = tid / kColLanes;         // 0..15: wave * 4 + K lane of the wave
  const int col0 = strip * CW + col_lane * VEC;
  // N is a multiple of 16: a lane's 8 columns are wholly inside or outside; outside lanes stream
  // column 0 of W8 (always valid) and their sums are dropped by the epilogue's column guard
  const uint8_t* wp = a.w8 + (col0 < a.N ? col0 : 0);

  // the first NS - 1 W8 batches are in flight before x is staged
  constexpr int NS = S::kSets;
  u32x2_t w[NS][U];
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < batches) load_batch<U>(w[s], wp, a.ldw, k0 + s * BR + row_lane, k1);

  // stage x[0..M)[k0..k1) -> xs[k - k0][m], zeros for m >= M and k >= k1
  {
    const uint16_t* x = static_cast<const uint16_t*>(a.x);
    const int rows_pad = batches * BR;
    const bool vec_ok = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (a.ldx * 2) % 16 == 0;
    const int nvec = rows_pad / 8, total = nvec * MB;
    // 8 k of one row per item; the loads of four items are issued before the first is written (a
    // 1024-row slice of 16 rows is 8 items per thread)
    constexpr int SU = 4;
    for (int i0 = tid; i0 < total; i0 += kThreads * SU) {
      u32x4_t r[SU];
#pragma unroll
      for (int s = 0; s < SU; ++s) {
        const int i = i0 + s * kThreads;
        r[s] = u32x4_t{0u, 0u, 0u, 0u};
        if (i >= total) continue;
        const int m = i / nvec, k = k0 + (i - m * nvec) * 8;
        if (m >= a.M) continue;
        if (vec_ok && k + 8 <= k1) {
          r[s] = *reinterpret_cast<const u32x4_t*>(x + static_cast<int64_t>(m) * a.ldx + k);
        } else {
          uint16_t v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = k + j < k1 ? x[static_cast<int64_t>(m) * a.ldx + k + j] : uint16_t(0);
          __builtin_memcpy(&r[s], v, 16);
        }
      }
#pragma unroll
      for (int s = 0; s < SU; ++s) {
        const int i = i0 + s * kThreads;
        if (i >= total) continue;
        const int m = i / nvec, kk = (i - m * nvec) * 8;
        uint16_t v[8];
        __builtin_memcpy(v, &r[s], 16);
#pragma unroll
        for (int j = 0; j < 8; ++j) xs[(kk + j) * MB + m] = v[j];
      }
    }
  }
  __syncthreads();

  float acc[MB][VEC];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[m][j] = 0.f;

  // the ring: set s holds batch b0 + s; batch b + NS - 1 is issued into the set consumed last,
  // then batch b is consumed (the loop is unrolled over the ring, so every set index is static and
  // no register is copied)
  for (int b0 = 0; b0 < batches; b0 += NS) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int b = b0 + s;
      if (b >= batches) break;
      if (b + NS - 1 < batches) load_batch<U>(w[(s + NS - 1) % NS], wp, a.ldw, k0 + (b + NS - 1) * BR + row_lane, k1);
      consume_batch<MB, U>(w[s], xs, b * BR + row_lane, acc);
    }
  }

  // the 16 K-lane sums of each output go through LDS and are added in lane order
  float res[S::kRounds][S::kOutPerRound];
#pragma unroll
  for (int h = 0; h < S::kRounds; ++h) {
    __syncthreads();  // xs (first round) / the previous round's sums are no longer read
#pragma unroll
    for (int mm = 0; mm < S::kRound; ++mm) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) red[(row_lane * S::kRound + mm) * CW + col_lane * VEC + j] = acc[h * S::kRound + mm][j];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < S::kOutPerRound; ++i) {
      const int o = tid + i * kThreads;
      float s = 0.f;
      if (o < S::kRound * CW) {
#pragma unroll
        for (int p = 0; p < kRowLanes; ++p) s += red[p * S::kRound * CW + o];
      }
      res[h][i] = s;
    }
  }

  // across workgroups: fp32 slabs [strip][slice][MB][CW], folded in slice order by the last arriver
  if (slices > 1) {
    float* slab = a.ws + (static_cast<int64_t>(strip) * slices + slice) * (MB * CW);
#pragma unroll
    for (int h = 0; h < S::kRounds; ++h)
#pragma unroll
      for (int i = 0; i < S::kOutPerRound; ++i) {
        const int o = tid + i * kThreads;
        if (o < S::kRound * CW && h * S::kRound + o / CW < a.M) st_wt(slab + h * S::kRound * CW + o, res[h][i]);
      }
    if (!det_ticket(a.tickets + strip, slices, flag)) return;
    // every output of this thread sums its slab column in slice order; the write-through loads of
    // CH slices of ALL its outputs are issued together (a load round trip per output and chunk, one
    // after the other, was the tail of the wide buckets). A slice past the end re-reads the last
    // one and is not added.
    const float* first = a.ws + static_cast<int64_t>(strip) * slices * (MB * CW);
    constexpr int NOUT = S::kRounds * S::kOutPerRound;
    constexpr int CH = NOUT <= 2 ? 16 : 8;
    bool live[NOUT];
#pragma unroll
    for (int h = 0; h < S::kRounds; ++h)
#pragma unroll
      for (int i = 0; i < S::kOutPerRound; ++i) {
        const int o = tid + i * kThreads;
        live[h * S::kOutPerRound + i] = o < S::kRound * CW && h * S::kRound + o / CW < a.M;
        res[h][i] = 0.f;
      }
    for (int r0 = 0; r0 < slices; r0 += CH) {
      float v[NOUT][CH];
#pragma unroll
      for (int h = 0; h < S::kRounds; ++h)
#pragma unroll
        for (int i = 0; i < S::kOutPerRound; ++i) {
          const int idx = h * S::kOutPerRound + i;
          if (!live[idx]) continue;
          const float* col = first + h * S::kRound * CW + tid + i * kThreads;
#pragma unroll
          for (int k = 0; k < CH; ++k) v[idx][k] = ld_wt(col + static_cast<int64_t>(min(r0 + k, slices - 1)) * (MB * CW));
        }
#pragma unroll
      for (int h = 0; h < S::kRounds; ++h)
#pragma unroll
        for (int i = 0; i < S::kOutPerRound; ++i) {
          const int idx = h * S::kOutPerRound + i;
          if (!live[idx]) continue;
#pragma unroll
          for (int k = 0; k < CH; ++k) res[h][i] = r0 + k < slices ? res[h][i] + v[idx][k] : res[h][i];
        }
    }
  }

  // epilogue: column scale (exact), bias (fp32), activation, store
#pragma unroll
  for (int h = 0; h < S::kRounds; ++h)
#pragma unroll
    for (int i = 0; i < S::kOutPerRound; ++i) {
      const int o = tid + i * kThreads;
      const int m = h * S::kRound + o / CW, col = strip * CW + o % CW;
      if (o >= S::kRound * CW || m >= a.M || col >= a.N) continue;
      float v = res[h][i] * a.scale[col];
      if (a.bias != nullptr) v += a.bias[col];
      v = act_fwd(v, a.act);
      const int64_t off = static_cast<int64_t>(m) * a.ldo + col;
      if (a.out_dtype == DT_BF16) static_cast<uint16_t*>(a.out)[off] = f2bf(v);
      else static_cast<float*>(a.out)[off] = v;
    }
}

hipError_t launch(const SkinnyW8Args& a, const SkinnyPlan& p, hipStream_t s) {
  const dim3 grid(p.strips, p.slices), block(kThreads);
  switch (skinny_bucket(a.M)) {
    case 1: hipLaunchKernelGGL((gemm_skinny_w8_kernel<1>), grid, block, 0, s, a, p.slices, p.slice_len); break;
    case 2: hipLaunchKernelGGL((gemm_skinny_w8_kernel<2>), grid, block, 0, s, a, p.slices, p.slice_len); break;
    case 4: hipLaunchKernelGGL((gemm_skinny_w8_kernel<4>), grid, block, 0, s, a, p.slices, p.slice_len); break;
    case 8: hipLaunchKernelGGL((gemm_skinny_w8_kernel<8>), grid, block, 0, s, a, p.slices, p.slice_len); break;
    default: hipLaunchKernelGGL((gemm_skinny_w8_kernel<16>), grid, block, 0, s, a, p.slices, p.slice_len); break;
  }
  return hipGetLastError();
}

}  // namespace

SkinnyPlan skinny_w8_plan(int K, int N) {
  SkinnyPlan p{};
  p.strip_cols = kCols;
  p.strips = (N + kCols - 1) / kCols;
  int want = (kTargetGroups + p.strips - 1) / p.strips;                 // fill the chip ...
  want = std::min(want, (K + kBatchRows - 1) / kBatchRows);             // ... with at least one granule each
  want = std::max(want, (K + kMaxSlice - 1) / kMaxSlice);               // a slice's x fits the LDS stage
  const int len = ((K + want - 1) / want + kBatchRows - 1) / kBatchRows * kBatchRows;
  p.slice_len = len;
  p.slices = (K + len - 1) / len;                                       // no empty slice
  return p;
}

bool skinny_w8_eligible(const SkinnyW8Args& a) {
  if (a.in_dtype != DT_BF16) return false;
  if (a.out_dtype != DT_BF16 && a.out_dtype != DT_F32) return false;
  if (a.M < 1 || a.M > 16 || a.K < 1 || a.N < 1) return false;
  if (a.act < ACT_NONE || a.act > ACT_TANH) return false;
  if (a.x == nullptr || a.w8 == nullptr || a.scale == nullptr || a.out == nullptr) return false;
  if (a.N % 16 != 0 || a.ldw % 16 != 0 || a.ldw < a.N) return false;
  if (reinterpret_cast<uintptr_t>(a.w8) % 16 != 0) return false;
  if (a.ldx < a.K || a.ldo < a.N) return false;
  const int64_t eo = a.out_dtype == DT_BF16 ? 2 : 4;
  if (reinterpret_cast<uintptr_t>(a.x) % 2 != 0 || reinterpret_cast<uintptr_t>(a.out) % eo != 0) return false;
  if (reinterpret_cast<uintptr_t>(a.scale) % 4 != 0) return false;
  if (a.bias != nullptr && reinterpret_cast<uintptr_t>(a.bias) % 4 != 0) return false;
  return true;
}

int64_t skinny_w8_ws_floats(const SkinnyW8Args& a) {
  const SkinnyPlan p = skinny_w8_plan(a.K, a.N);
  if (p.slices <= 1) return 0;
  return static_cast<int64_t>(p.strips) * p.slices * skinny_bucket(a.M) * p.strip_cols;
}

hipError_t gemm_skinny_w8(const SkinnyW8Args& a, hipStream_t s) {
  if (!skinny_w8_eligible(a)) return hipErrorInvalidValue;
  const SkinnyPlan p = skinny_w8_plan(a.K, a.N);
  if (p.slices > 1 && (a.ws == nullptr || a.tickets == nullptr)) return hipErrorInvalidValue;
  return launch(a, p, s);
}

}  // namespace pz
