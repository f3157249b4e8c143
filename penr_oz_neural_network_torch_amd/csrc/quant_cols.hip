// Column quantiser of the weight-only inference path: W [K][N] fp32 (the layers' natural [in, out]
// layout) -> W8 [K][N] OCP e4m3 in the same layout (no transpose) + scale[N] fp32.
//
// One POWER-OF-TWO scale per output column, derived in integer arithmetic on the exponent of the
// column's amax = max_k |W[k][n]| = m * 2^x, m in [0.5, 1):
//
//     e = x - 9 if m <= 0.875 else x - 8      (the smallest e with amax <= 448 * 2^e; 448 = 0.875 * 2^9)
//     e = max(e, -126)                        (scale stays a normal fp32; only amax < 2^-118 meets it)
//     scale[n] = 2^e, 1 for an all-zero column;   W8[k][n] = e4m3_rne(clamp(W[k][n] * 2^-e, +-448))
//
// Multiplying by 2^-e is exact, so W8 * scale is W rounded to 4 significant bits on its column's
// exponent grid and is exactly representable in bf16.
//
// Two launches in stream order: (1) column amax — per-thread maxima over a 64-column x 256-row
// block, folded through LDS, one atomicMax per column and block on the bits of the non-negative
// float (max is order-independent); (2) quantise — 8 columns per lane (two 16-B loads, four packed
// conversions, one 8-B store) where the operands allow it, element-wise otherwise, so any K, N and
// alignment is accepted. The lanes of row 0 publish the scales.
#include "pz_common.h"
#include "pz_kernels.h"

namespace pz {
namespace {

constexpr float kE4m3Max = 448.f;
constexpr int kAmaxCols = 64, kAmaxRows = 256;

// exponent e of the column scale from the bits of amax (> 0, finite)
PZ_DEV int scale_exp(float amax) {
  const uint32_t b = __float_as_uint(amax);
  const int x = static_cast<int>(b >> 23) - 126;  // frexp exponent (subnormal amax: clamped below anyway)
  const int e = x - 9 + ((b & 0x7FFFFFu) > 0x600000u ? 1 : 0);  // mantissa above 1.75 = m above 0.875
  return e < -126 ? -126 : e;
}
PZ_DEV float pow2(int e) { return __uint_as_float(static_cast<uint32_t>(e + 127) << 23); }  // -126 <= e <= 127

__global__ void __launch_bounds__(256) col_amax_kernel(const float* __restrict__ w, int64_t ldw, int K, int N, float* amax) {
  __shared__ float part[4][kAmaxCols];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int n = blockIdx.x * kAmaxCols + tx;
  const int k0 = blockIdx.y * kAmaxRows, k1 = min(K, k0 + kAmaxRows);
  float m = 0.f;
  if (n < N)
    for (int k = k0 + ty; k < k1; k += 4) m = fmaxf(m, fabsf(w[static_cast<int64_t>(k) * ldw + n]));
  part[ty][tx] = m;
  __syncthreads();
  if (ty == 0 && n < N) {
    m = fmaxf(fmaxf(part[0][tx], part[1][tx]), fmaxf(part[2][tx], part[3][tx]));
    if (m > 0.f) atomicMax(reinterpret_cast<unsigned int*>(amax + n), __float_as_uint(m));
  }
}

// VEC8: N % 8 == 0, 16-B aligned W rows, 8-B aligned W8 rows
template <bool VEC8>
__global__ void __launch_bounds__(256) quantize_cols_kernel(const float* __restrict__ w, int64_t ldw, int K, int N,
                                                            uint8_t* __restrict__ out, int64_t ldo,
                                                            const float* __restrict__ amax, float* __restrict__ scale) {
  constexpr int V = VEC8 ? 8 : 1;
  const int64_t per_row = N / V, total = static_cast<int64_t>(K) * per_row;
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * 256) {
    const int r = static_cast<int>(i / per_row), c = static_cast<int>(i - r * per_row) * V;
    float v[V], q[V];
    if constexpr (VEC8) {
      const float4 a0 = *reinterpret_cast<const float4*>(w + static_cast<int64_t>(r) * ldw + c);
      const float4 a1 = *reinterpret_cast<const float4*>(w + static_cast<int64_t>(r) * ldw + c + 4);
      v[0] = a0.x; v[1] = a0.y; v[2] = a0.z; v[3] = a0.w; v[4] = a1.x; v[5] = a1.y; v[6] = a1.z; v[7] = a1.w;
    } else {
      v[0] = w[static_cast<int64_t>(r) * ldw + c];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float am = amax[c + j];
      const int e = am > 0.f ? scale_exp(am) : 0;
      if (r == 0) scale[c + j] = pow2(e);
      q[j] = fminf(fmaxf(v[j] * pow2(-e), -kE4m3Max), kE4m3Max);  // exact multiply: -e <= 126
    }
    if constexpr (VEC8) {
      int lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
      lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], lo, true);
      int hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], 0, false);
      hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], hi, true);
      *reinterpret_cast<uint2*>(out + static_cast<int64_t>(r) * ldo + c) =
          make_uint2(static_cast<uint32_t>(lo), static_cast<uint32_t>(hi));
    } else {
      out[static_cast<int64_t>(r) * ldo + c] = static_cast<uint8_t>(__builtin_amdgcn_cvt_pk_fp8_f32(q[0], 0.f, 0, false) & 0xFF);
    }
  }
}

}  // namespace

hipError_t quantize_cols(const float* w, int64_t ldw, int K, int N, uint8_t* out, int64_t ldo, float* scale,
                         float* amax, hipStream_t s) {
  if (K <= 0 || N <= 0) return hipSuccess;
  if (ldw < N || ldo < N) return hipErrorInvalidValue;
  hipLaunchKernelGGL(col_amax_kernel, dim3((N + kAmaxCols - 1) / kAmaxCols, (K + kAmaxRows - 1) / kAmaxRows), dim3(256), 0,
                     s, w, ldw, K, N, amax);
  const bool vec8 = N % 8 == 0 && ldw % 4 == 0 && ldo % 8 == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(out) & 7) == 0;
  const int64_t work = static_cast<int64_t>(K) * (vec8 ? N / 8 : N);
  const int64_t blocks = (work + 256 * 4 - 1) / (256 * 4);  // ~4 items per thread
  const int grid = static_cast<int>(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
  if (vec8) hipLaunchKernelGGL(quantize_cols_kernel<true>, dim3(grid), dim3(256), 0, s, w, ldw, K, N, out, ldo, amax, scale);
  else hipLaunchKernelGGL(quantize_cols_kernel<false>, dim3(grid), dim3(256), 0, s, w, ldw, K, N, out, ldo, amax, scale);
  return hipGetLastError();
}

}  // namespace pz
