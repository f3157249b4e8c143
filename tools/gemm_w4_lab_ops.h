// Operand traits of the 4-wave schedule (csrc/gemm_w4.h: w4_kernel<Ops, EK>) that were measured but
// are not dispatched by the library. Included by tools/gemm_w4_lab.hip and tools/gemm_w4f8_lab.hip
// after gemm_mfma.hip.
#pragma once

namespace pz {
namespace {

// VAR 41 — bf16 with B M/N-contiguous ([K][N], the forward's weights): its K-step slot is
// [64 k][256 n] (512-B rows, swz_mn), one DMA = 2 k-rows, fragments by transposing
// ds_read_b64_tr_b16 reads (frag_mn). Measured: fwd_L2 1,278 vs 1,286 TF/s (VAR 30), fwd_L1 926 vs
// 944, same box (profiles/r6_gemm_w4.txt)
struct W4Bf16Fwd : W4Bf16 {
  static constexpr int VAR = 41, NB = 4, B_ROWS = 2;
  static constexpr bool B_KC = false;
  // B lane offsets: k-row lane / 32 of a 2-row piece, 16-B column chunk lane % 32 XOR swz_mn(k-row),
  // whose bits 0-1 and 3 vary with the piece (4 classes; class c stands for piece (c & 1) + 4 (c >> 1))
  static PZ_DEV int b_class(int i) { return (i & 1) + 2 * (i >> 2); }
  static PZ_DEV uint32_t b_lane(int c, int lane, uint32_t ldb) {
    const int kr = 2 * ((c & 1) + 4 * (c >> 1)) + (lane >> 5);
    return ((lane >> 5) * ldb + (((lane & 31) ^ swz_mn(kr)) * 8)) * 2u;
  }
  static PZ_DEV Frag frag_b(const PZ_LDS char* t, int kh, int col0, int f, int lane) {
    return frag_mn<256>(t, col0 + f * 16, 8 * (lane >> 4) + 32 * kh, lane);
  }
};

// VAR 42 — the fp8 policy's dX GEMM (e5m2 dZ x e4m3 W, both K-contiguous). Lab (tools/gemm_w4f8_lab.hip,
// plain store, same box, TF/s median): dX [8192,8192] K=1024 1,584 vs 1,341 (VAR 17), [8192,4096]
// K=4096 2,479 vs 1,743. Not dispatched: with the fused backward epilogue the 32x32 accumulator
// layout spills (144 vs 106 us in the mlp8192 step, profiles/r6_gemm_w4.txt)
struct W4F8Dx : W4F8Fwd {
  static constexpr int VAR = 42;
  static constexpr bool B_KC = true, FWD_ONLY = false;
  static PZ_DEV void mma(Acc& c, Frag b, Frag a) {  // blgp = A's format: e5m2 = 1
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b, a, c, 0, 1, 0, 127, 0, 127);
  }
};

// the dX GEMMs VAR 42 takes: e5m2 x e4m3, both K-contiguous
inline bool w4f8_eligible(const GemmArgs& p, int ek) {
  if (!p.a_kc || !p.b_kc || p.in_dtype != DT_FP8 || p.a_fmt != 1 || p.b_fmt != 0 || p.out_dtype != DT_BF16 ||
      p.accumulate)
    return false;
  if (ek != EK_BWD_MASK && ek != EK_ANY && ek != EK_STORE) return false;
  return w4_shape_ok(p, 128, static_cast<int64_t>(p.M) * p.lda, static_cast<int64_t>(p.N) * p.ldb);
}

}  // namespace
}  // namespace pz
