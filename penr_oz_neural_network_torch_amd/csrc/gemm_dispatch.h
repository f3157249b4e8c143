// Which kernel runs a GEMM: the whole decision, as host arithmetic on shapes, strides, alignments
// and flags. Plain C++17, no device code and no HIP call (tests/native/gemm_choose.cpp builds it
// with the host compiler alone). gemm_choose / gemm_pair_choose return what gemm_last will hold
// after the launch; kTiled lists every instantiated tiled kernel, and gemm_mfma.hip builds its
// launchers from that list, so a choice without a row cannot launch.
#pragma once

#include <cstdlib>
#include <cstring>

#include "pz_launch.h"

namespace pz {

// Compile-time epilogue kinds. The generic epilogue (EK_ANY) carries every transform — sigmoid /
// tanh with IEEE reciprocals, both dropout forms, aux-tile derivatives — unrolled over the tile's
// rows: ~20k instructions, and it measured ~5 us per tile of instruction-fetch stalls with EVERY
// transform switched off (tools/gemm_stamps.hip: stage-math phase 8.6 us in EPI_FWD with nothing
// enabled vs 3.3 us in EPI_STORE). The MLP's stages use three shapes, each specialised to only the
// code it runs (host: epi_kind()):
//   EK_STORE    alpha * acc -> bf16 (weight gradients)
//   EK_RELU     EPI_FWD with act NONE / RELU: bias, dropout pre / post, ReLU bitmask, fp8 copy
//   EK_BWD_MASK EPI_BWD through a ReLU stage from its bitmask: dropout scales, column sums, e5m2 copy
constexpr int EK_ANY = 0, EK_STORE = 1, EK_RELU = 2, EK_BWD_MASK = 3;
// Fixed forward stages (EPI_FWD, no colsum, not drop_all): the activation and both dropout flags
// are compile-time, so a row is ONE straight-line pass — no per-row flag branches, no untaken hash
// copies. EK_RELU with every transform switched off still ran ~1,400 more VALU instructions per
// wave and tile than the plain store (its 6.3k-instruction stage-math section: 3.6k I-cache
// misses per launch vs 0.6k; profiles/r3_epilogue_fixed_kinds.txt). The MLP's three stage
// shapes: linear -> ReLU -> dropout (first hidden stage), linear -> dropout -> ReLU -> dropout
// (later hidden stages), linear -> dropout (the logits).
constexpr int EK_F_RELU_POST = 4, EK_F_RELU_PREPOST = 5, EK_F_PRE = 6;
constexpr bool ek_fixed(int ek) { return ek >= EK_F_RELU_POST && ek <= EK_F_PRE; }
constexpr int kSkF32 = 100;  // stream-K engine: epilogue code of the fp32-output store path

// ------------------------------------------------------------------------------------ knobs
// VAR 40 for the bf16 dX layout and VAR 43 for the long-K plain fp8 forward (gemm_w4.h);
// PZ_GEMM_W4=0 keeps those GEMMs on VAR 30 / VAR 15, 16 (A/B)
inline bool w4_default() {
  static const bool on = [] {
    const char* e = getenv("PZ_GEMM_W4");
    return e == nullptr || atoi(e) != 0;
  }();
  return on;
}

inline bool sk_default() {
  static const bool on = [] {
    const char* e = getenv("PZ_GEMM_SK");
    return e != nullptr && atoi(e) != 0;
  }();
  return on;
}

inline bool deterministic() {
  static const bool on = [] {
    const char* e = getenv("PZ_DETERMINISTIC");
    return e == nullptr || atoi(e) != 0;
  }();
  return on;
}

struct GemmKnobs {
  bool w4, sk;
};
inline GemmKnobs gemm_knobs() { return {w4_default(), sk_default()}; }

// ------------------------------------------------------------------------------------ shared terms
constexpr int kFillTiles = 240;  // ~ CU count: a config below this leaves CUs idle
constexpr int kGemmBK = 32;      // K depth of one bf16 MFMA K block

inline int tiles(const GemmArgs& p, int bm, int bn) { return ((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); }
inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// buffer-addressed LDS-DMA takes 32-bit byte offsets: every staged byte of an operand of `eb`-byte
// elements must lie within 4 GiB of its base
constexpr int64_t k4GiB = int64_t(1) << 32;
inline int64_t a_bytes(const GemmArgs& p, int eb) { return (p.a_kc ? static_cast<int64_t>(p.M) : static_cast<int64_t>(p.K)) * p.lda * eb; }
inline int64_t b_bytes(const GemmArgs& p, int eb) { return (p.b_kc ? static_cast<int64_t>(p.N) : static_cast<int64_t>(p.K)) * p.ldb * eb; }
inline bool buffer_addressable(const GemmArgs& p, int eb = 2) { return a_bytes(p, eb) < k4GiB && b_bytes(p, eb) < k4GiB; }

// which specialised epilogue (EK_*) covers these arguments
inline int epi_kind(const GemmArgs& p) {
  if (p.out_dtype != DT_BF16 || p.accumulate) return EK_ANY;
  if (p.epi_mode == EPI_STORE && p.bias == nullptr && p.colsum == nullptr && p.mask == nullptr && p.out8 == nullptr)
    return EK_STORE;
  if (p.epi_mode == EPI_FWD && (p.epi.act == ACT_NONE || p.epi.act == ACT_RELU) && p.colsum == nullptr) {
    const EpiSpec& e = p.epi;
    const bool relu = e.act == ACT_RELU;
    if (!e.drop_all) {
      if (relu && !e.drop_pre && e.drop_post) return EK_F_RELU_POST;
      if (relu && e.drop_pre && e.drop_post) return EK_F_RELU_PREPOST;
      if (!relu && e.drop_pre && !e.drop_post) return EK_F_PRE;
    }
    return EK_RELU;
  }
  if (p.epi_mode == EPI_BWD && p.mask != nullptr && p.epi.act == ACT_RELU) return EK_BWD_MASK;
  return EK_ANY;
}

// One row per instantiated stream-K kernel: operand layout, type of C, the engine's epilogue code.
// gemm_sk.hip instantiates exactly these and launches from this list, and sk_takes answers from it,
// so a GEMM the engine is chosen for has a kernel.
struct SkKey {
  int a_kc, b_kc;
  int out;  // DType of C
  int ek;   // EK_*, or kSkF32
};
inline constexpr SkKey kSk[] = {
    // forward X · W[in, out]
    {1, 0, DT_BF16, EK_STORE}, {1, 0, DT_BF16, EK_RELU}, {1, 0, DT_BF16, EK_F_RELU_POST},
    {1, 0, DT_BF16, EK_F_RELU_PREPOST}, {1, 0, DT_BF16, EK_F_PRE}, {1, 0, DT_BF16, EK_ANY},
    // dX = dZ · Wᵀ
    {1, 1, DT_BF16, EK_STORE}, {1, 1, DT_BF16, EK_BWD_MASK}, {1, 1, DT_BF16, EK_ANY},
    // dW = Xᵀ · dZ
    {0, 0, DT_BF16, EK_STORE}, {0, 0, DT_F32, kSkF32},
};
constexpr int kNumSk = sizeof(kSk) / sizeof(kSk[0]);

// the row of kSk that is the kernel of epilogue code ek for p's layout and output type; -1: none
inline int sk_row(const GemmArgs& p, int ek) {
  for (int i = 0; i < kNumSk; ++i) {
    const SkKey& k = kSk[i];
    if (k.a_kc == (p.a_kc != 0) && k.b_kc == (p.b_kc != 0) && k.out == p.out_dtype && k.ek == ek) return i;
  }
  return -1;
}

// the epilogue code the stream-K engine would run arguments of kind ek = epi_kind(p) with: ek
// itself, kSkF32 for an fp32 C (weight gradients: plain stores only), -1 where its epilogues
// cannot do what p asks
inline int sk_epilogue(const GemmArgs& p, int ek) {
  if (p.out_dtype == DT_F32)
    return (p.epi_mode != EPI_STORE || p.mask != nullptr || p.out8 != nullptr || p.colsum != nullptr) ? -1 : kSkF32;
  if (p.out_dtype != DT_BF16 || p.accumulate) return -1;
  if (p.epi_mode == EPI_STORE) return p.out8 != nullptr ? -1 : ek;
  if (p.epi_mode == EPI_FWD) return ek;
  if (p.epi_mode != EPI_BWD) return -1;
  if (p.mask != nullptr) return p.epi.act == ACT_RELU ? ek : -1;
  if (p.aux == nullptr || p.aux_dtype != DT_BF16 || p.ldaux % 8 != 0 || !aligned16(p.aux)) return -1;
  return ek;
}

// the stream-K engine's epilogue code for p, -1 where it has no kernel of that code in p's layout
// (kSk): those GEMMs stay on the tiled kernels
inline int sk_takes(const GemmArgs& p, int ek) {
  const int code = sk_epilogue(p, ek);
  return code >= 0 && sk_row(p, code) >= 0 ? code : -1;
}

// ------------------------------------------------------------------------------------ eligibility
// VAR 14: X8ᵀ (e4m3) · dZ8 (e5m2); fp8_eligible asks for GEMMs with both operands M/N-contiguous
inline bool fp8_dw_eligible(const GemmArgs& p) {
  if (p.a_fmt != 0 || p.b_fmt != 1 || p.epi_mode != EPI_STORE || p.accumulate) return false;
  if (p.bias != nullptr || p.colsum != nullptr || p.mask != nullptr || p.out8 != nullptr || p.aux != nullptr) return false;
  if (p.M % 256 != 0 || p.N % 256 != 0 || p.K % 64 != 0 || p.K < 64) return false;
  if (p.lda % 16 != 0 || p.ldb % 16 != 0 || p.ldc % 8 != 0) return false;
  if (!aligned16(p.A) || !aligned16(p.B) || !aligned16(p.C)) return false;
  return buffer_addressable(p, 1);  // buffer-addressed staging
}

inline bool fp8_eligible(const GemmArgs& p) {
  if (p.force_generic || p.in_dtype != DT_FP8 || p.out_dtype != DT_BF16) return false;
  if (p.bias64 != nullptr || p.colsum64 != nullptr) return false;
  if (!p.a_kc && !p.b_kc) return fp8_dw_eligible(p);
  if (p.b_fmt != 0) return false;
  if (p.a_kc && !p.b_kc) {  // VAR 15: forward on the [in, out] e4m3 weights
    if (p.a_fmt != 0 || p.epi_mode == EPI_BWD || p.accumulate || p.N % 256 != 0) return false;
    if (b_bytes(p, 1) >= k4GiB) return false;  // buffer-addressed B
  } else if (!p.a_kc || p.accumulate) {
    return false;
  }
  if (p.M < 64 || p.N < 64 || p.K < 64 || p.K % 64 != 0) return false;
  if (p.N % 8 != 0 || p.ldc % 8 != 0 || p.lda % 16 != 0 || p.ldb % 16 != 0) return false;
  if (!aligned16(p.A) || !aligned16(p.B) || !aligned16(p.C)) return false;
  if (p.idx_ld % 2 != 0) return false;
  if (p.bias != nullptr && !aligned16(p.bias)) return false;
  // e4m3 x e4m3: forward stages; e5m2 (A, gradients) x e4m3 (B): backward dX stages only
  if ((p.a_fmt == 1) != (p.epi_mode == EPI_BWD)) return false;
  if (p.out8 != nullptr && p.out8_fmt != (p.epi_mode == EPI_BWD ? 1 : 0)) return false;
  if (p.epi_mode == EPI_BWD && p.mask == nullptr &&
      (p.aux == nullptr || p.aux_dtype != DT_BF16 || p.ldaux % 8 != 0 || !aligned16(p.aux)))
    return false;
  if (p.mask != nullptr && (p.ldmask % 32 != 0 || (reinterpret_cast<uintptr_t>(p.mask) & 7) != 0)) return false;
  if (p.out8 != nullptr && (p.ldout8 % 8 != 0 || (reinterpret_cast<uintptr_t>(p.out8) & 7) != 0 ||
                            p.out8_qscale == nullptr))
    return false;
  return true;
}

inline bool mfma_eligible(const GemmArgs& p) {
  if (p.in_dtype == DT_FP8) return fp8_eligible(p);
  if (p.force_generic || p.in_dtype != DT_BF16) return false;
  if (p.bias64 != nullptr || p.colsum64 != nullptr) return false;  // fp64 models: wide / generic paths
  if (p.out_dtype != DT_BF16 && p.out_dtype != DT_F32) return false;
  if (p.M < 64 || p.N < 64 || p.K < kGemmBK || p.K % kGemmBK != 0) return false;
  if (p.N % 8 != 0 || p.ldc % 8 != 0) return false;
  if (!aligned16(p.A) || !aligned16(p.B) || !aligned16(p.C)) return false;
  if (p.lda % 8 != 0 || p.ldb % 8 != 0) return false;
  if (!p.a_kc && p.M % 8 != 0) return false;
  if (p.idx_ld % 2 != 0) return false;  // 4-element epilogue groups start at even element indices
  // fused stage epilogues: bf16 output only; accumulate: fp32 output only
  if (p.out_dtype == DT_F32 && p.epi_mode != EPI_STORE && p.epi_mode != EPI_OPT) return false;
  if (p.epi_mode == EPI_OPT) {  // fused optimizer update: plain gradient tiles, 16-B state vectors
    if (p.out_dtype != DT_F32 || p.bias != nullptr || p.colsum != nullptr || p.accumulate || p.mask != nullptr ||
        p.out8 != nullptr || p.ldc % 4 != 0 || p.opt.params == nullptr || !aligned16(p.opt.params))
      return false;
    if (p.opt.adam && (!aligned16(p.opt.exp_avg) || !aligned16(p.opt.exp_avg_sq))) return false;
    if (p.opt.shadow != nullptr &&
        (reinterpret_cast<uintptr_t>(p.opt.shadow) & (p.opt.shadow_dtype == DT_BF16 ? 7 : 15)) != 0)
      return false;
  }
  if (p.out_dtype == DT_BF16 && p.accumulate) return false;
  if (p.bias != nullptr && !aligned16(p.bias)) return false;
  if (p.out8 != nullptr && (p.out_dtype != DT_BF16 || p.out8_fmt != (p.epi_mode == EPI_BWD ? 1 : 0) ||
                            (p.epi_mode != EPI_BWD && p.epi_mode != EPI_FWD) || p.ldout8 % 8 != 0 ||
                            (reinterpret_cast<uintptr_t>(p.out8) & 7) != 0 || p.out8_qscale == nullptr))
    return false;
  if (p.mask != nullptr) {
    if (p.out_dtype != DT_BF16 || p.ldmask % 32 != 0 || (reinterpret_cast<uintptr_t>(p.mask) & 7) != 0) return false;
    if (p.epi_mode == EPI_BWD ? p.epi.act != ACT_RELU : p.epi_mode != EPI_FWD) return false;
    return true;
  }
  if (p.epi_mode == EPI_BWD) {
    if (p.aux == nullptr || p.ldaux % 8 != 0 || !aligned16(p.aux)) return false;
    if (p.aux_dtype != DT_BF16) return false;
  }
  return true;
}

// gemm_wide.hip: fp32 / fp64 operands on the matrix cores; tiny problems (one partial tile, e.g. the
// reference's 9x9 tic-tac-toe layers) stay on the generic VALU tile, which wastes fewer lanes
inline bool wide_eligible(const GemmArgs& p) {
  if (p.force_generic || (p.in_dtype != DT_F32 && p.in_dtype != DT_F64)) return false;
  if (p.mask != nullptr || p.out8 != nullptr || p.split_k > 1 || p.epi_mode == EPI_OPT) return false;
  return static_cast<int64_t>(p.M) * p.N >= 64 * 64 && p.K >= 16;
}

// the persistent stream-K engine (gemm_sk.hip): whole 256 x 256 tiles, 64-deep K steps
inline bool sk_eligible(const GemmArgs& p) {
  if (p.force_generic || p.in_dtype != DT_BF16 || (p.out_dtype != DT_BF16 && p.out_dtype != DT_F32)) return false;
  if (p.bias64 != nullptr || p.colsum64 != nullptr) return false;
  if (p.engine == 3) return false;  // (round-5 lab loop: tools/gemm_w4_lab.hip)
  if (p.M <= 0 || p.N <= 0 || p.M % 256 != 0 || p.N % 256 != 0 || p.K % 64 != 0 || p.K < 2 * 64) return false;
  if (!p.a_kc && p.b_kc) return false;  // (no MLP GEMM has this layout)
  if (!aligned16(p.A) || !aligned16(p.B) || (p.C != nullptr && !aligned16(p.C))) return false;
  if (p.lda % 8 != 0 || p.ldb % 8 != 0 || p.ldc % 8 != 0 || p.idx_ld % 2 != 0) return false;
  if (p.bias != nullptr && !aligned16(p.bias)) return false;
  if (!buffer_addressable(p)) return false;  // buffer-addressed staging
  if (p.mask != nullptr && (p.ldmask % 32 != 0 || !aligned16(p.mask))) return false;
  if (p.out8 != nullptr && (p.out8_fmt != (p.epi_mode == EPI_BWD ? 1 : 0) || p.ldout8 % 8 != 0 ||
                            (reinterpret_cast<uintptr_t>(p.out8) & 7) != 0 || p.out8_qscale == nullptr))
    return false;
  return sk_takes(p, epi_kind(p)) >= 0;
}

// the shape conditions of every 4-wave variant (gemm_w4.h): whole 256 x 256 tiles that fill the
// CUs, no split-K, at least 2 K steps of `step` elements, buffer-addressable operands (their
// extents in bytes)
inline bool w4_shape_ok(const GemmArgs& p, int step, int64_t a_bytes, int64_t b_bytes) {
  if (p.split_k > 1 || p.M % 256 || p.N % 256 || p.K % step || p.K < 2 * step) return false;
  if (tiles(p, 256, 256) < kFillTiles) return false;
  return a_bytes < k4GiB && b_bytes < k4GiB;
}

// dX-layout bf16 GEMMs VAR 40 takes: a backward-mask or plain-store epilogue
inline bool w4_eligible(const GemmArgs& p, int ek) {
  if (!p.a_kc || !p.b_kc || p.in_dtype != DT_BF16 || p.out_dtype != DT_BF16 || p.accumulate) return false;
  if (ek != EK_BWD_MASK && ek != EK_STORE) return false;
  return w4_shape_ok(p, 64, a_bytes(p, 2), b_bytes(p, 2));
}

// the fp8 forward GEMMs VAR 43 takes (e4m3 x e4m3 [in, out] weights)
inline bool w4f8_fwd_eligible(const GemmArgs& p, int ek) {
  if (!p.a_kc || p.b_kc || p.in_dtype != DT_FP8 || p.a_fmt != 0 || p.b_fmt != 0 || p.out_dtype != DT_BF16 ||
      p.accumulate || p.epi_mode == EPI_BWD)
    return false;
  if (!ek_fixed(ek) && ek != EK_RELU && ek != EK_STORE) return false;
  return w4_shape_ok(p, 128, a_bytes(p, 1), b_bytes(p, 1));
}

// (measured, not kept: 128x128 tiles, two workgroups per CU, instead of split-K 256x256 for
// skinny shapes — fwd [8192,1024] K=4096 950 vs 855 TFLOP/s alone, the mlp4 step 0.9% slower)
// 64-deep ring steps (VAR 30: 2 x 64 KiB slots, one MFMA interval = 64 MFMAs per wave, the
// staging waves fetch whole 128-B lines of K-contiguous rows) for layouts with an M/N-contiguous
// operand: fwd [8192,4096]x[4096,4096] +6%, dW +4%, fwd K=1024 +4% (tools/gemm_lab, same box).
// Both operands K-contiguous (dX) stay on the 32-deep ring: the BK64 form spills there (-11%).
inline bool use_bk64(const GemmArgs& p, bool buf) {
  const int split = p.split_k > 1 ? p.split_k : 1;
  // VAR 30 stages K-contiguous operands without a row clamp: full 256-row tiles only (which
  // also frees the K-contiguous x K-contiguous dX GEMMs from a scratch spill: +5..6%, lab)
  const bool full = (!p.a_kc || p.M % 256 == 0) && (!p.b_kc || p.N % 256 == 0);
  return buf && full && p.K % 64 == 0 && (p.K / 64) % split == 0;
}

// Fixed-kind bf16 forward GEMMs with too few 256x256 tiles to fill the CUs (the logits GEMM,
// [8192, 1024] at K = 4096) run as 256x128 tiles on the 64-deep ring WITHOUT split-K: the
// deterministic split-K fold's slab round trip and the split tile's heavier epilogue cost more
// than the narrower tile's extra LDS traffic. r5 same box: fused fwd_L3 885-949 vs 830-841 TF/s,
// mlp4 step 1.111-1.113 vs 1.130-1.138 ms (profiles/r5_ab_w128_fixed.txt). (r2, before the
// fixed epilogue kinds and the deterministic fold: the generic-epilogue 256x128 form lost in-step.)
inline bool w128_fixed(const GemmArgs& p) {
  if (p.in_dtype != DT_BF16 || p.out_dtype != DT_BF16 || !p.a_kc || p.b_kc || p.accumulate) return false;
  if (p.M % 256 || p.N % 128 || !ek_fixed(epi_kind(p))) return false;
  return tiles(p, 256, 256) < kFillTiles && tiles(p, 256, 128) >= kFillTiles;
}

// fp8 GEMMs with at least two 256x256 tiles per CU and no split-K run as 256x128 tiles on 4-wave
// workgroups, two per CU (VAR 16 / 17): one workgroup's epilogue beside the other's main loop
inline bool f8_two_wg(const GemmArgs& p) {
  return p.split_k <= 1 && tiles(p, 256, 256) >= 2 * kFillTiles && p.N % 128 == 0;
}

// ------------------------------------------------------------------------------------ split-K plans
inline int gemm_split(const GemmArgs& p) {
  // fp8 skinny shapes run better as 128x128 tiles (measured: split-K 256x256 -4%); the fp8
  // weight-gradient GEMM (both operands M/N-contiguous, 256-tiles only) splits like bf16
  // (and the N-contiguous-weight fp8 forward, VAR 15: 256x256 tiles only)
  const bool f8_dw = p.in_dtype == DT_FP8 && !p.b_kc;
  if ((p.in_dtype == DT_FP8 && !f8_dw) || !mfma_eligible(p)) return 1;
  if (w128_fixed(p)) return 1;
  const int t256 = tiles(p, 256, 256);
  if (t256 >= kFillTiles) return 1;
  // (fixed-kind forwards: 256x128 tiles instead, w128_fixed above; the generic-epilogue kinds
  // keep the split — r2: 1008 vs 881 TF/s alone but the mlp4 step slower,
  // profiles/r2_lab_skinny_fwd.txt)
  const int nk = p.K / (p.in_dtype == DT_FP8 ? 64 : kGemmBK);
  for (int sp : {2, 4, 8})
    if (t256 * sp >= kFillTiles && nk % sp == 0 && nk / sp >= 16) return sp;
  return 1;
}

// fp32 floats of the split-K slabs of a GEMM that runs `split` slices: one 256 x 256 slab per
// tile and slice
inline int64_t split_ws_floats(const GemmArgs& p, int split) {
  return split <= 1 ? 0 : static_cast<int64_t>(tiles(p, 256, 256)) * split * 256 * 256;
}
inline int64_t gemm_split_ws_floats(const GemmArgs& p) { return split_ws_floats(p, gemm_split(p)); }

// gemm_pair: both GEMMs in the weight-gradient layout (A and B M/N-contiguous), plain stores of
// whole 256 x 256 tiles, one K; returns the split-K factor of the pair, or 0 if it cannot be paired
inline int gemm_pair_split(const GemmArgs& a, const GemmArgs& b) {
  for (const GemmArgs* q : {&a, &b}) {
    const GemmArgs& p = *q;
    if (p.a_kc || p.b_kc || p.epi_mode != EPI_STORE || p.accumulate || p.force_generic) return 0;
    if (p.bias || p.colsum || p.mask || p.out8 || p.aux || p.bias64 || p.colsum64) return 0;
    if (p.M % 256 || p.N % 256 || p.K % 64 || !mfma_eligible(p)) return 0;
    if (p.in_dtype != DT_FP8 && (!buffer_addressable(p) || epi_kind(p) != (p.out_dtype == DT_BF16 ? EK_STORE : EK_ANY)))
      return 0;
  }
  if (a.K != b.K || a.in_dtype != b.in_dtype || a.out_dtype != b.out_dtype || a.a_fmt != b.a_fmt ||
      a.b_fmt != b.b_fmt)
    return 0;
  if (a.in_dtype == DT_FP8 && a.out_dtype != DT_BF16) return 0;
  const int t256 = tiles(a, 256, 256) + tiles(b, 256, 256);
  const int nk = a.K / 64;
  for (int sp : {1, 2, 4, 8})
    if (t256 * sp >= kFillTiles && nk % sp == 0 && nk / sp >= 16) return sp;
  return nk % 8 == 0 && nk / 8 >= 16 ? 8 : 1;
}

// ------------------------------------------------------------------------------------ the choice
inline bool family_is(const GemmLaunch& c, const char* family) { return std::strcmp(c.family, family) == 0; }
constexpr GemmLaunch kNoKernel = {"none", 0, 0, 0, 0, 1};  // no kernel runs these arguments: gemm() refuses them

// bf16 operands on the tiled kernels of gemm_mfma.hip / gemm_w4.h (mfma_eligible; split_k planned)
inline GemmLaunch choose_bf16(const GemmArgs& p, const GemmKnobs& k) {
  const int split = p.split_k > 1 ? p.split_k : 1;
  const int ek = epi_kind(p);
  // buffer-addressed LDS-DMA (VAR 6; +2..12% on the step's shapes, tools/gemm_lab); operands that
  // reach past 4 GiB take flat addresses (VAR 0)
  const bool buf = buffer_addressable(p);
  const int var32 = buf ? 6 : 0;
  const bool bk64 = use_bk64(p, buf);
  // 256x256 tiles: the MLP's three GEMM layouts on the 64-deep ring, each with its stage's
  // specialised epilogue: forward X·W (K-contiguous x N-contiguous), dX = dZ·Wᵀ (both
  // K-contiguous), dW = Xᵀ·dZ (both M/N-contiguous); anything else takes the generic epilogue
  const bool fwd = p.a_kc && !p.b_kc, dx = p.a_kc && p.b_kc, dw = !p.a_kc && !p.b_kc;
  const bool ek30 = (fwd && (ek_fixed(ek) || ek == EK_RELU)) || (dx && ek == EK_BWD_MASK) || (dw && ek == EK_STORE);
  const GemmLaunch t256 = bk64 ? GemmLaunch{"mfma", 30, 256, 256, ek30 ? ek : EK_ANY, split}
                               : GemmLaunch{"mfma", var32, 256, 256, EK_ANY, split};
  if (split > 1) return t256;  // slabs sized for 256x256
  if (k.w4 && w4_eligible(p, ek)) return {"w4", 40, 256, 256, ek, 1};
  if (tiles(p, 256, 256) >= kFillTiles) return t256;
  if (tiles(p, 256, 128) >= kFillTiles) {
    // (no ReLU-stage form of this config: w128_fixed takes the fixed kinds only)
    if (bk64 && w128_fixed(p)) return {"mfma", 30, 256, 128, ek, 1};
    return {"mfma", bk64 ? 30 : var32, 256, 128, EK_ANY, 1};
  }
  return {"mfma", var32, 128, 128, EK_ANY, 1};
}

// fp8 operands (fp8_eligible; split_k planned)
inline GemmLaunch choose_fp8(const GemmArgs& p, const GemmKnobs& k) {
  const int split = p.split_k > 1 ? p.split_k : 1;
  if (!p.a_kc && !p.b_kc)  // e4m3 x e5m2 weight gradient (fp8_eligible: full 256-tiles, buffer-addressable,
                          // plain store)
    return {"mfma", 14, 256, 256, EK_STORE, split};
  const int ek = epi_kind(p);
  // forward layout: the fixed stages and the ReLU stage have their own kinds, else the generic epilogue
  const int ek_fwd = ek_fixed(ek) || ek == EK_RELU ? ek : EK_ANY;
  // VAR 43: the fp8 forward on the 4-wave LDS-DMA schedule, plain stores at K >= 2048 (at K = 1,024 it
  // ties VAR 16). With the fused stage epilogues the 32x32 accumulator layout's 128-column wave rows
  // (16 four-column groups per lane: values, column sums, bias) spill 66-213 VGPRs — the fused fp8 dX
  // (VAR 42, tools/gemm_w4_lab_ops.h) ran 144 vs 106 us in the mlp8192 step (profiles/r6_gemm_w4.txt) —
  // so the trainer's fused fp8 GEMMs stay on VAR 9 / 15-17
  if (k.w4 && ek == EK_STORE && p.K >= 2048 && w4f8_fwd_eligible(p, ek)) return {"w4", 43, 256, 256, EK_STORE, 1};
  if (f8_two_wg(p)) {
    if (p.a_kc && !p.b_kc) return {"mfma", 16, 256, 128, ek_fwd, 1};
    if (p.a_kc && p.b_kc && p.a_fmt == 1) return {"mfma", 17, 256, 128, ek == EK_BWD_MASK ? ek : EK_ANY, 1};
  }
  // e4m3 X x e4m3 W[in, out] (fp8_eligible: N % 256 — B's transposed image rows are whole 256-B
  // tiles, swz_mn8 — buffer-addressable B; split-K when the tiles do not fill the CUs, gemm_split)
  if (p.a_kc && !p.b_kc) return {"mfma", 15, 256, 256, ek_fwd, split};
  // (measured, not kept: buffer-addressed staging, VAR 10 / 11; the 64-deep ring, VAR 12 / 13,
  // within noise of the 32-deep one, profiles/r2_ab_fp8_bk64.txt)
  const int tile = tiles(p, 256, 256) >= kFillTiles || split > 1 ? 256 : 128;
  if (p.a_fmt == 1)  // e5m2 x e4m3 (backward dX)
    return {"mfma", 9, tile, tile, ek == EK_BWD_MASK ? ek : EK_ANY, split};
  // (VAR 8 forms: the fixed kinds run the generic ReLU-stage kind)
  return {"mfma", 8, tile, tile, ek_fixed(ek) || ek == EK_RELU ? EK_RELU : EK_ANY, split};
}

// The kernel gemm() launches for p (split_k as the caller planned it: gemm_split, or none), in
// gemm_last's terms; family "none" where gemm() refuses
inline GemmLaunch gemm_choose(const GemmArgs& p, const GemmKnobs& k) {
  // the persistent stream-K engine: asked for (engine 2 / 3), or the default engine with PZ_GEMM_SK
  // or a CU budget, wherever it is eligible (engine 1: the tiled kernels)
  if ((p.engine >= 2 || (p.engine == 0 && (k.sk || p.cus > 0))) && sk_eligible(p))
    return {"sk", 0, 256, 256, sk_takes(p, epi_kind(p)), 1};
  if (mfma_eligible(p)) return p.in_dtype == DT_FP8 ? choose_fp8(p, k) : choose_bf16(p, k);
  if (p.epi_mode == EPI_OPT) return kNoKernel;  // the fused update: bf16 MFMA path only
  if (wide_eligible(p)) return {"wide", 0, 128, 128, 0, 1};
  // bitmask / e4m3 epilogues and e4m3 operands exist on the MFMA path only
  if (p.mask != nullptr || p.out8 != nullptr || p.in_dtype == DT_FP8) return kNoKernel;
  return {"generic", 0, 64, 64, 0, 1};
}

// which path the tiled engine would take: 0 = generic VALU, 1 = MFMA bf16 / fp8, 2 = MFMA fp32 / fp64
inline int gemm_path(const GemmArgs& p) {
  GemmArgs q = p;
  q.engine = 1;
  const GemmLaunch c = gemm_choose(q, GemmKnobs{true, false});
  return family_is(c, "mfma") || family_is(c, "w4") ? 1 : family_is(c, "wide") ? 2 : 0;
}

// the kernel gemm_pair() launches for (a, b) with the split gemm_pair_split plans; "none": not a pair
inline GemmLaunch gemm_pair_choose(const GemmArgs& a, const GemmArgs& b) {
  const int split = gemm_pair_split(a, b);
  if (split == 0) return kNoKernel;
  if (a.in_dtype == DT_FP8) return {"pair", 14, 256, 256, EK_STORE, split};
  return {"pair", 30, 256, 256, a.out_dtype == DT_BF16 ? EK_STORE : EK_ANY, split};
}

// ------------------------------------------------------------------------------------ the kernels
// One row per instantiated kernel (or per family of one kernel in several operand layouts):
// gemm_mfma.hip instantiates exactly these.
enum : int { L_DW = 1, L_TN = 2, L_FWD = 4, L_DX = 8, L_ALL = 15 };  // bit 2 * a_kc + b_kc
struct TiledKey {
  int bm, bn, wm, wn;  // output tile, wave grid
  int var, ek;
  int out;      // DType of C
  int layouts;  // L_* the row is built for
};

inline constexpr TiledKey kTiled[] = {
    // bf16 operands, generic epilogue, every layout, bf16 and fp32 C: the 64-deep ring (30), the
    // 32-deep ring buffer-addressed (6) and flat (0)
    {256, 256, 2, 4, 30, EK_ANY, DT_BF16, L_ALL}, {256, 256, 2, 4, 30, EK_ANY, DT_F32, L_ALL},
    {256, 256, 2, 4, 6, EK_ANY, DT_BF16, L_ALL},  {256, 256, 2, 4, 6, EK_ANY, DT_F32, L_ALL},
    {256, 256, 2, 4, 0, EK_ANY, DT_BF16, L_ALL},  {256, 256, 2, 4, 0, EK_ANY, DT_F32, L_ALL},
    {256, 128, 4, 2, 30, EK_ANY, DT_BF16, L_ALL}, {256, 128, 4, 2, 30, EK_ANY, DT_F32, L_ALL},
    {256, 128, 4, 2, 6, EK_ANY, DT_BF16, L_ALL},  {256, 128, 4, 2, 6, EK_ANY, DT_F32, L_ALL},
    {256, 128, 4, 2, 0, EK_ANY, DT_BF16, L_ALL},  {256, 128, 4, 2, 0, EK_ANY, DT_F32, L_ALL},
    {128, 128, 2, 2, 6, EK_ANY, DT_BF16, L_ALL},  {128, 128, 2, 2, 6, EK_ANY, DT_F32, L_ALL},
    {128, 128, 2, 2, 0, EK_ANY, DT_BF16, L_ALL},  {128, 128, 2, 2, 0, EK_ANY, DT_F32, L_ALL},
    // VAR 30, 256x256: each MLP layout's specialised epilogues
    {256, 256, 2, 4, 30, EK_RELU, DT_BF16, L_FWD},
    {256, 256, 2, 4, 30, EK_F_RELU_POST, DT_BF16, L_FWD},
    {256, 256, 2, 4, 30, EK_F_RELU_PREPOST, DT_BF16, L_FWD},
    {256, 256, 2, 4, 30, EK_F_PRE, DT_BF16, L_FWD},
    {256, 256, 2, 4, 30, EK_BWD_MASK, DT_BF16, L_DX},
    {256, 256, 2, 4, 30, EK_STORE, DT_BF16, L_DW},
    // VAR 30, 256x128: the fixed-kind forwards (w128_fixed)
    {256, 128, 4, 2, 30, EK_F_RELU_POST, DT_BF16, L_FWD},
    {256, 128, 4, 2, 30, EK_F_RELU_PREPOST, DT_BF16, L_FWD},
    {256, 128, 4, 2, 30, EK_F_PRE, DT_BF16, L_FWD},
    // fp8 weight gradient
    {256, 256, 2, 4, 14, EK_STORE, DT_BF16, L_DW},
    // fp8 forward on the [in, out] weights: 256x256 (15) and two 4-wave workgroups per CU (16)
    {256, 256, 2, 4, 15, EK_ANY, DT_BF16, L_FWD},
    {256, 256, 2, 4, 15, EK_RELU, DT_BF16, L_FWD},
    {256, 256, 2, 4, 15, EK_F_RELU_POST, DT_BF16, L_FWD},
    {256, 256, 2, 4, 15, EK_F_RELU_PREPOST, DT_BF16, L_FWD},
    {256, 256, 2, 4, 15, EK_F_PRE, DT_BF16, L_FWD},
    {256, 128, 2, 2, 16, EK_ANY, DT_BF16, L_FWD},
    {256, 128, 2, 2, 16, EK_RELU, DT_BF16, L_FWD},
    {256, 128, 2, 2, 16, EK_F_RELU_POST, DT_BF16, L_FWD},
    {256, 128, 2, 2, 16, EK_F_RELU_PREPOST, DT_BF16, L_FWD},
    {256, 128, 2, 2, 16, EK_F_PRE, DT_BF16, L_FWD},
    // fp8 dX (e5m2 x e4m3): two workgroups per CU (17), 256x256 / 128x128 (9)
    {256, 128, 2, 2, 17, EK_ANY, DT_BF16, L_DX},
    {256, 128, 2, 2, 17, EK_BWD_MASK, DT_BF16, L_DX},
    {256, 256, 2, 4, 9, EK_ANY, DT_BF16, L_DX},
    {256, 256, 2, 4, 9, EK_BWD_MASK, DT_BF16, L_DX},
    {128, 128, 2, 2, 9, EK_ANY, DT_BF16, L_DX},
    {128, 128, 2, 2, 9, EK_BWD_MASK, DT_BF16, L_DX},
    // e4m3 x e4m3, both K-contiguous
    {256, 256, 2, 4, 8, EK_ANY, DT_BF16, L_DX},
    {256, 256, 2, 4, 8, EK_RELU, DT_BF16, L_DX},
    {128, 128, 2, 2, 8, EK_ANY, DT_BF16, L_DX},
    {128, 128, 2, 2, 8, EK_RELU, DT_BF16, L_DX},
    // the 4-wave schedule (gemm_w4.h): VAR 40 = W4Bf16, VAR 43 = W4F8Fwd
    {256, 256, 2, 2, 40, EK_STORE, DT_BF16, L_DX},
    {256, 256, 2, 2, 40, EK_BWD_MASK, DT_BF16, L_DX},
    {256, 256, 2, 2, 43, EK_STORE, DT_BF16, L_FWD},
};
constexpr int kNumTiled = sizeof(kTiled) / sizeof(kTiled[0]);

// gemm_pair's kernels (gemm_mfma_pair_kernel)
inline constexpr TiledKey kPair[] = {
    {256, 256, 2, 4, 14, EK_STORE, DT_BF16, L_DW},
    {256, 256, 2, 4, 30, EK_STORE, DT_BF16, L_DW},
    {256, 256, 2, 4, 30, EK_ANY, DT_F32, L_DW},
};
constexpr int kNumPair = sizeof(kPair) / sizeof(kPair[0]);

inline int layout_index(const GemmArgs& p) { return 2 * (p.a_kc != 0) + (p.b_kc != 0); }

// the row of `keys` that is the kernel of choice c for p's output type and layout; -1: none
template <int N>
int find_row(const TiledKey (&keys)[N], const GemmLaunch& c, const GemmArgs& p) {
  const int lay = 1 << layout_index(p);
  for (int i = 0; i < N; ++i) {
    const TiledKey& k = keys[i];
    if (k.var == c.var && k.ek == c.ek && k.bm == c.bm && k.bn == c.bn && k.out == p.out_dtype && (k.layouts & lay))
      return i;
  }
  return -1;
}

}  // namespace pz
