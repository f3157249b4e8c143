// Host-side launch API of the pz HIP kernels. Plain C++ (no torch headers) so the kernel
// translation units compile fast; bindings.cpp adapts torch tensors to these calls.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pz_types.h"

namespace pz {

enum DType : int { DT_BF16 = 0, DT_F32 = 1, DT_F64 = 2, DT_FP8 = 3 };

enum EpiMode : int {
  EPI_STORE = 0,  // C = alpha*AB (+bias)                      [+ optional colsum of C]
  EPI_FWD = 1,    // C = epi_fwd(alpha*AB + bias)               (fused dropout/act/dropout)
  EPI_BWD = 2,    // C = epi_bwd(alpha*AB, aux)                 [+ optional colsum of C]
  EPI_OPT = 3,    // C is NOT stored: g = alpha*AB is the gradient of the fp32 weight p[M][N] and the
                  // optimizer update of p (GemmOpt) runs in the epilogue (fp32 output, MFMA path)
};

// EPI_OPT: the weight-gradient GEMM applies the update of the weight whose gradient it produces
// (single process: nothing has to be reduced first) — the fp32 gradient is never written to
// memory nor read back by a separate optimizer pass (8 B/param of HBM traffic and one launch per
// weight saved), and the update leaves the step's tail. Numerics are those of optimizer_step
// (torch.optim.Adam single-tensor / the reference's SGD). Element (m, n) of every array below is
// at m * ldc + n (the weight's own [in, out] layout, the dW GEMM's C).
struct GemmOpt {
  float* params;          // fp32 master weight
  float* exp_avg;         // Adam moments (nullptr: SGD)
  float* exp_avg_sq;
  void* shadow;           // low-precision GEMM copy written after the update (nullptr: none)
  int shadow_dtype;       // DT_BF16 or DT_F32
  int adam;
  double* stats;          // this weight's 4 accumulators: sum(dw), sum(dw^2), sum(w), sum(w^2)
  float* amax;            // optional: max |w_new| (fp8 weight scaling)
  const double* hp;       // graph-replayed steps: {lr, bias_c1, bias_c2_sqrt, -} of epoch *epoch_ptr
  const int* epoch_ptr;
  int stats_every;        // as OptArgs::stats_every
  float lr, beta1, beta2, eps, bias_c1, bias_c2_sqrt;
  float grad_scale;       // 1 / world
  float l2x2;             // 2 * l2 (the L2 term's gradient, weights only)
};

// C[M][N] = op(A) · op(B); row-major C with leading dim ldc.
//  a_kc: A stored [M][K] (K contiguous) if true, else [K][M]
//  b_kc: B stored [N][K] (K contiguous) if true, else [K][N]
struct GemmArgs {
  const void* A;
  const void* B;
  void* C;
  int M, N, K;
  int64_t lda, ldb, ldc;
  int a_kc, b_kc;
  int in_dtype;   // DType of A and B
  int out_dtype;  // DType of C
  float alpha;
  int accumulate;  // C += result (beta = 1)
  const float* bias;  // [N] fp32 or null (EPI_STORE / EPI_FWD)
  const void* aux;    // EPI_BWD: stored stage output y, [M][ldaux], dtype aux_dtype
  int64_t ldaux;
  int aux_dtype;
  float* colsum;      // [N] fp32: atomically accumulates column sums of the final C values
  // fp64 models (generic / wide paths only): the bias and the column sums in the master precision
  // (used instead of bias / colsum when set) — the fp64 fused engine stays exact to fp64 rounding
  const double* bias64;
  double* colsum64;
  // deterministic column sums (pz_common.h det_colsum; bf16 LDS-staged epilogues): per-tile partial
  // rows [ceil(M / BM) + groups][N] and per-column-strip tickets; null = float atomics
  float* cs_ws;
  int* cs_tickets;
  int epi_mode;
  EpiSpec epi;
  int64_t idx_ld;     // logical row stride used for dropout element indices (usually N)
  int force_generic;  // testing: bypass the MFMA path
  // ReLU bitmask, bit (n & 7) of byte mask_off(m, n) = (y[m][n] > 0), tile-blocked: 256 x 256
  // element blocks of 8 KiB (256 rows of 32 B), block (m / 256, n / 256) at byte
  // ((m / 256) * ldmask / 32 + n / 256) * 8192 — a [roundup(M, 256), ldmask] uint8 tensor with
  // ldmask = 32 * ceil(N / 256). One 256 x 256 tile's bits are one contiguous 8 KiB run: the
  // forward epilogue writes it as 512-B runs per store pass (a row-major [M][N/8] mask scattered
  // them as 32-B row segments over 256 rows), and the dX epilogue's 8-B reads stay inside it.
  // EPI_FWD writes it (from the final stage output); EPI_BWD with act == RELU reads it INSTEAD of
  // aux: 1/16 of the bytes of re-reading the stored bf16 activation. MFMA path only.
  uint8_t* mask;
  int64_t ldmask;
  // fp8 (e4m3) operands: A/B hold e4m3 bytes; the products are dequantised by the device-side
  // per-tensor factors *scale_a * *scale_b (nullptr = 1) on top of alpha
  const float* scale_a;
  const float* scale_b;
  int a_fmt;  // fp8 A operand format: 0 = e4m3, 1 = e5m2 (gradients of the dX GEMM)
  int b_fmt;  // fp8 B operand format: 1 = e5m2 only for the weight-gradient GEMM X8ᵀ · dZ8
  // EPI_FWD extra output: e4m3 copy of C, out8[m*ldout8 + n] = sat(C * *out8_qscale), and the
  // running max |C| (atomicMax into *amax, which the caller zeroes) for delayed scaling
  uint8_t* out8;
  int64_t ldout8;
  int out8_fmt;  // 0: e4m3 (EPI_FWD activations), 1: e5m2 (EPI_BWD: dZ for the next fp8 dW GEMM)
  const float* out8_qscale;
  float* amax;
  // split-K (set by the launcher, gemm_split()): K is cut into split_k slices computed by
  // separate workgroups; every slice stores its fp32 partial tile into ws, and the LAST slice to
  // arrive at a tile (per-tile counter) sums the others and runs the epilogue
  int split_k;
  float* ws;       // [tiles * split_k][BM * BN] fp32
  int* counters;   // [tiles], zero; reset by the last arriver
  GemmOpt opt;     // EPI_OPT only
  uint64_t* dbg;   // diagnostic phase stamps (tools/gemm_stamps.hip builds only); nullptr otherwise
  // epilogue stores of whole tiles (C, the ReLU bitmask, the fp8 copy) as write-through `sc1`
  // buffer stores (set by the launcher, PZ_GEMM_WT): a kernel boundary writes back every line a
  // kernel left dirty in the XCD L2s (~B / 6 TB/s for B dirty bytes, MI355X_MICROARCH "boundary"),
  // and a GEMM that stores 64 MB of output leaves the L2s full of them
  int store_wt;
  int prio;  // s_setprio(1) around the ping-pong MFMA blocks (set by the launcher, PZ_GEMM_PRIO)
  // persistent stream-K engine (gemm_sk.hip): workgroups = CUs it may occupy (0 = every CU; the
  // trainer lowers it while RCCL channels hold CUs), engine 0 = default choice, 1 = the tiled
  // kernels of gemm_mfma.hip, 2 = stream-K (8-wave ping-pong loop), 3 = stream-K on the 4-wave lab loop
  int cus;
  int engine;
};

// The functions below that decide something (sk_eligible, sk_default, deterministic, gemm_split,
// gemm_split_ws_floats, gemm_pair_split, gemm_path) are defined inline in gemm_dispatch.h, beside
// gemm_choose: a caller includes that header.
// persistent stream-K engine: eligibility, workspace (fp32 floats for the partial-tile slabs of a
// `cus`-workgroup launch; 0 = none needed) and launch over one or two problems of one layout and
// epilogue kind (the second one's tiles follow the first's; equal K)
bool sk_eligible(const GemmArgs& p);
int64_t sk_ws_floats(const GemmArgs* probs, int n);
int sk_tickets(const GemmArgs* probs, int n);  // per-tile ticket counters needed
int sk_device_cus();  // the CU count the engine plans with (gemm_sk_plan.h sk_plan's device_cus)
hipError_t gemm_sk(const GemmArgs* probs, int n, float* ws, int* counters, hipStream_t stream);
bool sk_default();  // PZ_GEMM_SK: the engine gemm() picks for eligible shapes
// PZ_DETERMINISTIC (default 1): bias-gradient column sums of the bf16 GEMM epilogues and heads are
// folded in a fixed order (pz_common.h det_colsum) instead of float atomics
bool deterministic();

// split-K plan for the MFMA path: 1 = none. Workspace floats needed: gemm_split_ws_floats().
int gemm_split(const GemmArgs& args);
int64_t gemm_split_ws_floats(const GemmArgs& args);

// returns hipSuccess or an error; chooses the MFMA path when the shape allows
hipError_t gemm(const GemmArgs& args, hipStream_t stream);
// two weight-gradient-layout GEMMs (A, B M/N-contiguous; plain stores; equal K; whole 256-tiles)
// in one launch. gemm_pair_split: the pair's split-K factor (set it as split_k of both, with
// gemm_split_ws_floats-sized workspaces for that factor), 0 = the pair is not eligible
int gemm_pair_split(const GemmArgs& a, const GemmArgs& b);
hipError_t gemm_pair(const GemmArgs& a, const GemmArgs& b, hipStream_t stream);
// exposed for tests / benchmarks: which path gemm() would take
int gemm_path(const GemmArgs& args);  // 0 = generic VALU, 1 = MFMA bf16 / fp8, 2 = MFMA fp32 / fp64

// The GEMM kernel this thread launched last. Every launcher writes it next to its launch, so it
// cannot disagree with what ran (gemm_choose, gemm_dispatch.h, predicts it): family "generic", "wide",
// "mfma" (the tiled kernels), "w4" (gemm_w4.h), "sk" (stream-K) or "pair"; the kernel's VAR number
// (0 where the family has none), output tile, epilogue kind (gemm_dispatch.h EK_*; 0 = EK_ANY where
// the family has none) and split-K factor
struct GemmLaunch {
  const char* family;
  int var, bm, bn, ek, split;
};
inline thread_local GemmLaunch gemm_last = {"none", 0, 0, 0, 0, 1};

// Skinny-batch forward GEMM of the inference path (gemm_skinny.hip): out[M][N] = act(x[M][K] ·
// W[K][N] + bias), 1 <= M <= 16, W N-contiguous, x of W's type (bf16 / fp32), fp32 accumulation.
// A separate op: gemm() never selects it.
struct SkinnyArgs {
  const void* x;      // [M][ldx]
  const void* w;      // [K][ldw]
  void* out;          // [M][ldo]
  const float* bias;  // [N] fp32 or null
  int M, N, K;
  int64_t ldx, ldw, ldo;  // elements
  int in_dtype;       // DT_BF16 or DT_F32 (x and W)
  int out_dtype;      // DT_BF16 or DT_F32
  int act;            // Act, applied after the bias
  float* ws;          // skinny_ws_floats() fp32 partial slabs (slices > 1)
  int* tickets;       // [strips], zero; reset by each strip's last arriver
};
struct SkinnyPlan {
  int strips;      // column strips of strip_cols columns (grid.x)
  int strip_cols;
  int slices;      // K slices over workgroups (grid.y)
  int slice_len;   // K rows per slice
};
SkinnyPlan skinny_plan(int K, int N, int dtype);  // never a function of M
int skinny_bucket(int M);                         // compile-time row count the call runs with: 1, 2, 4, 8, 16
bool skinny_eligible(const SkinnyArgs& a);
int64_t skinny_ws_floats(const SkinnyArgs& a);
hipError_t gemm_skinny(const SkinnyArgs& a, hipStream_t stream);  // hipErrorInvalidValue: not eligible, nothing launched

// Weight-only quantised skinny GEMM (gemm_skinny_w8.hip): out[M][N] = act(scale[n] * (x[M][K] ·
// W8[K][N]) + bias[n]), 1 <= M <= 16, x bf16, W8 OCP e4m3 bytes (N-contiguous), scale a power of
// two per output column (quant_cols.hip), fp32 accumulation. A separate op: neither gemm() nor
// gemm_skinny() ever selects it. Eligible: W8's row bytes and leading dimension multiples of 16 B,
// its base 16-B aligned; everything else at its natural alignment.
struct SkinnyW8Args {
  const void* x;       // [M][ldx] bf16
  const uint8_t* w8;   // [K][ldw] e4m3
  const float* scale;  // [N] fp32, powers of two
  void* out;           // [M][ldo]
  const float* bias;   // [N] fp32 or null
  int M, N, K;
  int64_t ldx, ldw, ldo;  // elements
  int in_dtype;        // x: DT_BF16 (anything else is refused)
  int out_dtype;       // DT_BF16 or DT_F32
  int act;             // Act, applied after scale and bias
  float* ws;           // skinny_w8_ws_floats() fp32 partial slabs (slices > 1)
  int* tickets;        // [strips], zero; reset by each strip's last arriver
};
SkinnyPlan skinny_w8_plan(int K, int N);  // never a function of M
bool skinny_w8_eligible(const SkinnyW8Args& a);
int64_t skinny_w8_ws_floats(const SkinnyW8Args& a);
hipError_t gemm_skinny_w8(const SkinnyW8Args& a, hipStream_t stream);  // hipErrorInvalidValue: not eligible, nothing launched

}  // namespace pz
