// Skinny-batch forward GEMM for inference: out[M,N] = act(x[M,K] @ W[K,N] + bias), 1 <= M <= 16.
//
// W is in the layers' natural [in, out] layout (N-contiguous), bf16 or fp32 (x has W's type), fp32
// accumulation. The kernel is a weight stream: at these M a GEMM is bound by reading W once, so
//
//  * every lane loads 16 B of one W row straight to registers (8 bf16 / 4 fp32 columns); a batch
//    of 8 such loads (4 / 2 in the buckets with 64 / 128 accumulators) is issued back to back and the next
//    batch is issued before the current one is consumed (two register sets), so two batches are in
//    flight per lane. W never passes through LDS.
//  * a wave is 8 column lanes x 8 K lanes: one load instruction reads whole 128-B lines of 8 rows.
//    A 256-thread workgroup covers a strip of kColLanes * VEC columns and 32 K-rows per load.
//  * x (<= 16 rows) is staged once per workgroup into LDS, transposed to [k][m], so the MB values
//    a lane needs for its K-row are one or two 16-B LDS reads (broadcast among the column lanes).
//  * the row count is a compile-time bucket MB (1, 2, 4, 8, 16): MB * VEC fp32 accumulators stay
//    in registers; rows >= M are zeros in LDS and are neither folded across workgroups nor stored.
//  * K is split across the K lanes of a wave, the waves of a workgroup, and across workgroups
//    (skinny_plan: a function of K, N and the dtype only). Partial sums are combined in a fixed
//    order: lane pairs by one DPP row rotate, the 16 pair sums of a workgroup through LDS in pair
//    order, the workgroups' fp32 slabs in slice order by the last arriver of the strip's ticket
//    (pz_common.h det_ticket: write-through stores, every wave drained, one agent-scope ticket;
//    write-through loads). No float atomics: a call is bit-reproducible, and because neither the
//    plan nor any summation order depends on M, row r of a 16-row call equals that row sent alone.
//  * the folding workgroup adds the fp32 bias, applies act_fwd (pz_common.h) and stores bf16 / fp32.
//
// Eligibility (skinny_eligible; anything else is refused on the host, never launched): W's row
// bytes and leading dimension are multiples of 16 B and its base is 16-B aligned; x, out and bias
// need only their natural alignment (x rows are staged by 16-B loads when they allow it, by
// element loads otherwise). K rows past the end are never read (load_batch clamps the row).
#include <algorithm>

#include "pz_common.h"
#include "pz_launch.h"

namespace pz {

namespace {

constexpr int kThreads = 256;
constexpr int kColLanes = 8;                       // lanes of a wave along N
constexpr int kRowLanes = kThreads / kColLanes;    // K-rows a workgroup covers per load: 32
constexpr int kLoads = 8;                          // 16-B loads per lane and batch (Shape::kU: 4 in the wide buckets)
constexpr int kBatchRows = kRowLanes * kLoads;     // 256: the plan's granule of a K slice
constexpr int kPairs = kRowLanes / 2;              // partial sums per output after the DPP stage: 16
constexpr int kFoldRows = 8;                       // output rows folded through LDS per round
constexpr int kTargetGroups = 512;                 // ~2 workgroups per CU on a 256-CU chip

template <typename T> struct Elem;
template <> struct Elem<uint16_t> { static constexpr int kVec = 8; static constexpr int kMaxSlice = 1024; };
template <> struct Elem<float> { static constexpr int kVec = 4; static constexpr int kMaxSlice = 512; };

template <typename T> PZ_DEV void unpack(const u32x4_t& r, float (&w)[Elem<T>::kVec]);
template <> PZ_DEV void unpack<uint16_t>(const u32x4_t& r, float (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[2 * i] = __uint_as_float(r[i] << 16);
    w[2 * i + 1] = __uint_as_float(r[i] & 0xFFFF0000u);
  }
}
template <> PZ_DEV void unpack<float>(const u32x4_t& r, float (&w)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = __uint_as_float(r[i]);
}

template <typename T, int MB>
struct Shape {
  static constexpr int kVec = Elem<T>::kVec;
  static constexpr int kCols = kColLanes * kVec;            // strip width: 64 bf16 / 32 fp32 columns
  static constexpr int kRound = MB < kFoldRows ? MB : kFoldRows;
  static constexpr int kRounds = MB / kRound;
  static constexpr int kOutPerRound = (kRound * kCols + kThreads - 1) / kThreads;
  static constexpr int kXsBytes = Elem<T>::kMaxSlice * MB * static_cast<int>(sizeof(T));
  static constexpr int kRedBytes = kPairs * kRound * kCols * 4;
  // loads per lane and batch: two sets of them live beside the MB * VEC accumulators, so the wide
  // buckets (VALU-bound anyway) take fewer (64 accumulators: 4, 128: 2) to stay clear of spills;
  // which rows a lane sums, and in what order, is the same
  static constexpr int kU = MB * kVec >= 128 ? kLoads / 4 : MB * kVec >= 64 ? kLoads / 2 : kLoads;
  static constexpr int kRows = kRowLanes * kU;              // K-rows per batch
  static constexpr int kLds = kXsBytes > kRedBytes ? kXsBytes : kRedBytes;
};

// one batch: U W vectors of this lane, rows row0 + u * kRowLanes (row0 includes the lane's K lane).
// A row past the slice reads row k1 - 1 instead and drops the value: no out-of-bounds read and no
// branch, so a partial batch's loads still issue back to back (one min and four selects per load).
template <int U>
PZ_DEV void load_batch(u32x4_t (&w)[U], const char* wp, int64_t ldw_bytes, int row0, int k1) {
#pragma unroll
  for (int u = 0; u < U; ++u)
    w[u] = *reinterpret_cast<const u32x4_t*>(wp + static_cast<int64_t>(min(row0 + u * kRowLanes, k1 - 1)) * ldw_bytes);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (row0 + u * kRowLanes >= k1) w[u] = u32x4_t{0u, 0u, 0u, 0u};
}

// the MB values of one staged x row: 16-B LDS reads where a row has that many bytes
template <typename T, int MB>
PZ_DEV void load_x(const T* xr, float (&xf)[MB]) {
  constexpr int VEC = Elem<T>::kVec;
  if constexpr (MB >= VEC) {
#pragma unroll
    for (int i = 0; i < MB / VEC; ++i) {
      float part[VEC];
      unpack<T>(reinterpret_cast<const u32x4_t*>(xr)[i], part);
#pragma unroll
      for (int j = 0; j < VEC; ++j) xf[i * VEC + j] = part[j];
    }
  } else {
#pragma unroll
    for (int m = 0; m < MB; ++m) xf[m] = to_f<T>(xr[m]);
  }
}

template <typename T, int MB, int U>
PZ_DEV void consume_batch(const u32x4_t (&w)[U], const T* xs, int lrow0, float (&acc)[MB][Elem<T>::kVec]) {
  constexpr int VEC = Elem<T>::kVec;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float wf[VEC], xf[MB];
    unpack<T>(w[u], wf);
    load_x<T, MB>(xs + (lrow0 + u * kRowLanes) * MB, xf);
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[m][j] = fmaf(xf[m], wf[j], acc[m][j]);
  }
}

template <typename T, int MB>
__global__ void __launch_bounds__(kThreads, 2) gemm_skinny_kernel(const SkinnyArgs a, const int slices, const int slice_len) {
  using S = Shape<T, MB>;
  constexpr int VEC = S::kVec, CW = S::kCols;
  __shared__ __attribute__((aligned(16))) char smem[S::kLds];
  T* xs = reinterpret_cast<T*>(smem);          // [slice rows, padded to whole batches][MB]
  float* red = reinterpret_cast<float*>(smem); // [kPairs][kRound][CW], after the K loop
  PZ_LDS int* flag = (PZ_LDS int*)(smem);       // the ticket's verdict, after the sums left LDS

  const int tid = threadIdx.x;
  const int strip = blockIdx.x, slice = blockIdx.y;
  const int k0 = slice * slice_len;
  const int k1 = min(a.K, k0 + slice_len);
  constexpr int U = S::kU, BR = S::kRows;
  const int batches = (k1 - k0 + BR - 1) / BR;
  const int col_lane = tid & (kColLanes - 1);
  const int row_lane = tid / kColLanes;         // 0..31: wave * 8 + K lane of the wave
  const int col0 = strip * CW + col_lane * VEC;
  // N is a multiple of VEC: a lane's vector is wholly inside or outside; outside lanes stream
  // column 0 of W (always valid) and their sums are dropped by the epilogue's column guard
  const char* wp = static_cast<const char*>(a.w) + static_cast<int64_t>(col0 < a.N ? col0 : 0) * sizeof(T);
  const int64_t ldw_bytes = a.ldw * static_cast<int64_t>(sizeof(T));

  // first W batch in flight before x is staged
  u32x4_t wa[U], wb[U];
  load_batch<U>(wa, wp, ldw_bytes, k0 + row_lane, k1);

  // stage x[0..M)[k0..k1) -> xs[k - k0][m], zeros for m >= M and k >= k1
  {
    const T* x = static_cast<const T*>(a.x);
    const int rows_pad = batches * BR;
    const bool vec_ok = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (a.ldx * sizeof(T)) % 16 == 0;
    const int nvec = rows_pad / VEC;
    for (int i = tid; i < nvec * MB; i += kThreads) {
      const int m = i / nvec, kk = (i - m * nvec) * VEC;
      const int k = k0 + kk;
      T v[VEC];
      if (m < a.M && vec_ok && k + VEC <= k1) {
        const u32x4_t r = *reinterpret_cast<const u32x4_t*>(x + static_cast<int64_t>(m) * a.ldx + k);
        __builtin_memcpy(v, &r, 16);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          v[j] = (m < a.M && k + j < k1) ? x[static_cast<int64_t>(m) * a.ldx + k + j] : T(0);
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) xs[(kk + j) * MB + m] = v[j];
    }
  }
  __syncthreads();

  float acc[MB][VEC];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[m][j] = 0.f;

  for (int b = 0; b < batches; ++b) {
    const int next = k0 + (b + 1) * BR;
    const bool more = b + 1 < batches;
    if (more) {  // the next batch is in flight while this one is consumed
      load_batch<U>(wb, wp, ldw_bytes, next + row_lane, k1);
    }
    consume_batch<T, MB, U>(wa, xs, b * BR + row_lane, acc);
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) wa[u] = wb[u];
    }
  }

  // K lanes 2j and 2j+1 of a wave sit 8 lanes apart in one DPP row: one row rotate pairs them;
  // the 16 pair sums of each output then go through LDS and are summed in pair order
  float res[S::kRounds][S::kOutPerRound];
  const int pair = row_lane >> 1;
#pragma unroll
  for (int h = 0; h < S::kRounds; ++h) {
    __syncthreads();  // xs (first round) / the previous round's sums are no longer read
#pragma unroll
    for (int mm = 0; mm < S::kRound; ++mm) {
      float v[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float t = acc[h * S::kRound + mm][j];
        v[j] = t + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), 0x128, 0xF, 0xF, false));
      }
      if ((row_lane & 1) == 0) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) red[(pair * S::kRound + mm) * CW + col_lane * VEC + j] = v[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < S::kOutPerRound; ++i) {
      const int o = tid + i * kThreads;
      float s = 0.f;
      if (o < S::kRound * CW) {
#pragma unroll
        for (int p = 0; p < kPairs; ++p) s += red[p * S::kRound * CW + o];
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
    const float* first = a.ws + static_cast<int64_t>(strip) * slices * (MB * CW);
#pragma unroll
    for (int h = 0; h < S::kRounds; ++h)
#pragma unroll
      for (int i = 0; i < S::kOutPerRound; ++i) {
        const int o = tid + i * kThreads;
        if (o < S::kRound * CW && h * S::kRound + o / CW < a.M)
          res[h][i] = det_fold(first + h * S::kRound * CW + o, MB * CW, 0, slices, 0);
      }
  }

  // epilogue: bias (fp32), activation, store
#pragma unroll
  for (int h = 0; h < S::kRounds; ++h)
#pragma unroll
    for (int i = 0; i < S::kOutPerRound; ++i) {
      const int o = tid + i * kThreads;
      const int m = h * S::kRound + o / CW, col = strip * CW + o % CW;
      if (o >= S::kRound * CW || m >= a.M || col >= a.N) continue;
      float v = res[h][i];
      if (a.bias != nullptr) v += a.bias[col];
      v = act_fwd(v, a.act);
      const int64_t off = static_cast<int64_t>(m) * a.ldo + col;
      if (a.out_dtype == DT_BF16) static_cast<uint16_t*>(a.out)[off] = f2bf(v);
      else static_cast<float*>(a.out)[off] = v;
    }
}

template <typename T>
hipError_t launch(const SkinnyArgs& a, const SkinnyPlan& p, hipStream_t s) {
  const dim3 grid(p.strips, p.slices), block(kThreads);
  switch (skinny_bucket(a.M)) {
    case 1: hipLaunchKernelGGL((gemm_skinny_kernel<T, 1>), grid, block, 0, s, a, p.slices, p.slice_len); break;
    case 2: hipLaunchKernelGGL((gemm_skinny_kernel<T, 2>), grid, block, 0, s, a, p.slices, p.slice_len); break;
    case 4: hipLaunchKernelGGL((gemm_skinny_kernel<T, 4>), grid, block, 0, s, a, p.slices, p.slice_len); break;
    case 8: hipLaunchKernelGGL((gemm_skinny_kernel<T, 8>), grid, block, 0, s, a, p.slices, p.slice_len); break;
    default: hipLaunchKernelGGL((gemm_skinny_kernel<T, 16>), grid, block, 0, s, a, p.slices, p.slice_len); break;
  }
  return hipGetLastError();
}

int elem_size(int dtype) { return dtype == DT_BF16 ? 2 : 4; }

}  // namespace

int skinny_bucket(int M) {
  int b = 1;
  while (b < M) b *= 2;
  return b;
}

SkinnyPlan skinny_plan(int K, int N, int dtype) {
  const int vec = 16 / elem_size(dtype);
  const int max_slice = dtype == DT_BF16 ? Elem<uint16_t>::kMaxSlice : Elem<float>::kMaxSlice;
  SkinnyPlan p{};
  p.strip_cols = kColLanes * vec;
  p.strips = (N + p.strip_cols - 1) / p.strip_cols;
  int want = (kTargetGroups + p.strips - 1) / p.strips;                 // fill the chip ...
  want = std::min(want, (K + kBatchRows - 1) / kBatchRows);             // ... with at least one batch each
  want = std::max(want, (K + max_slice - 1) / max_slice);               // a slice's x fits the LDS stage
  const int len = ((K + want - 1) / want + kBatchRows - 1) / kBatchRows * kBatchRows;
  p.slice_len = len;
  p.slices = (K + len - 1) / len;                                       // no empty slice
  return p;
}

bool skinny_eligible(const SkinnyArgs& a) {
  if (a.in_dtype != DT_BF16 && a.in_dtype != DT_F32) return false;
  if (a.out_dtype != DT_BF16 && a.out_dtype != DT_F32) return false;
  if (a.M < 1 || a.M > 16 || a.K < 1 || a.N < 1) return false;
  if (a.act < ACT_NONE || a.act > ACT_TANH) return false;
  const int64_t es = elem_size(a.in_dtype), eo = elem_size(a.out_dtype);
  if ((a.N * es) % 16 != 0 || (a.ldw * es) % 16 != 0 || a.ldw < a.N) return false;
  if (reinterpret_cast<uintptr_t>(a.w) % 16 != 0) return false;
  if (a.ldx < a.K || a.ldo < a.N) return false;
  if (reinterpret_cast<uintptr_t>(a.x) % es != 0 || reinterpret_cast<uintptr_t>(a.out) % eo != 0) return false;
  if (a.bias != nullptr && reinterpret_cast<uintptr_t>(a.bias) % 4 != 0) return false;
  return true;
}

int64_t skinny_ws_floats(const SkinnyArgs& a) {
  const SkinnyPlan p = skinny_plan(a.K, a.N, a.in_dtype);
  if (p.slices <= 1) return 0;
  return static_cast<int64_t>(p.strips) * p.slices * skinny_bucket(a.M) * p.strip_cols;
}

hipError_t gemm_skinny(const SkinnyArgs& a, hipStream_t s) {
  if (!skinny_eligible(a)) return hipErrorInvalidValue;
  const SkinnyPlan p = skinny_plan(a.K, a.N, a.in_dtype);
  if (p.slices > 1 && (a.ws == nullptr || a.tickets == nullptr)) return hipErrorInvalidValue;
  return a.in_dtype == DT_BF16 ? launch<uint16_t>(a, p, s) : launch<float>(a, p, s);
}

}  // namespace pz
