// The 4-wave LDS-DMA GEMM schedule: hipBLASLt's gfx950 dX kernel
// (Custom_Cijk_Alik_Bljk_..._MT256x256x64, disassembled in round 6: profiles/r6_hipblaslt_kernels.txt),
// written once for this library's LDS-DMA and epilogues and instantiated per operand format.
// Included by gemm_mfma.hip inside namespace pz::(anonymous).
//
//   * 256 x 256 tiles, 4 waves (one per SIMD), 128 x 128 per wave: T x T accumulator tiles = 256
//     AGPRs (bf16: 8 x 8 of 16x16x32; fp8: 4 x 4 of 32x32x64), mfma(B, A) so the Lay16 / Lay32
//     epilogue layouts apply (gemm_epilogue.h).
//   * TWO 64-KiB LDS buffers, one 128-byte K step each ([256][128 B] A then B, swz_kc<64>; an
//     M/N-contiguous B: [k][256 elements]), filled by buffer_load ... lds: one DMA = 1 KiB.
//   * Fragments of BOTH k-halves of step t are in registers before its second half's MFMAs (sets
//     S0 / S1, 2T fragments each), so buffer t&1 is free for step t+2's DMAs from the middle of
//     iteration t on. The two k-halves are T*T MFMAs each:
//       phase 1: MFMAs S0 rows 0..T/2-1 + the 2T S1 reads (step t)       B1: lgkmcnt(0) + barrier
//       phase 2-3: MFMAs S0 rows T/2..T-1, S1 rows 0..T/2-1 + 12 DMAs (step t+2)
//       B2: vmcnt(12) (step t+1 landed) + barrier
//       phase 4: MFMAs S1 rows T/2..T-1 + the 2T S0 reads (step t+1) + 4 DMAs (step t+2)
//     The last two iterations are compile-time copies without DMAs (no wasted loads, no per-DMA
//     branches: a per-piece guard inside the unrolled phases cost 11% in the lab).
//   * The 128 KiB of LDS then hold the epilogue's tile image (epilogue_lds: the library's own
//     epilogue code — column sums, e5m2 copy, ReLU bitmask).
// What differs between formats is an operand-traits struct `Ops`:
//   VAR, EB (element bytes), T, B_KC, FWD_ONLY (epilogue_lds), Frag, Acc, Lay;
//   frag_k(slot, row, kh, lane): the lane's part (tile row `row`) of a K-contiguous operand's fragment;
//   mma(acc, b, a); alpha(p): the epilogue's factor;
//   NB, b_class(i): B's per-lane DMA offsets and the one piece i (0..7) of a K step uses;
//   M/N-contiguous B only: B_ROWS (k-rows per 1-KiB piece), b_lane(c, lane, ldb), frag_b(slot, kh, col0, f, lane).
// The library dispatches W4Bf16 (VAR 40) and W4F8Fwd (VAR 43) below, for the GEMMs that w4_eligible /
// w4f8_fwd_eligible (gemm_dispatch.h) accept; the measured, undispatched
// VAR 41 / 42 live in tools/gemm_w4_lab_ops.h.
namespace w4cfg {
constexpr int kW4M = 256, kW4N = 256, kW4T = 256;
constexpr int kStepB = 128;               // bytes of a K-contiguous row per K step
constexpr int kTB = kW4M * kStepB * 2;    // one K-step buffer: A + B, 64 KiB
constexpr int kD4 = 4;                    // DMA pieces issued in phase 4 (the other 12 in phases 2-3)
constexpr int kD23 = 16 - kD4;
}  // namespace w4cfg

template <class Ops, int EK>
__global__ void __launch_bounds__(w4cfg::kW4T) __attribute__((amdgpu_waves_per_eu(1, 1)))
w4_kernel(const GemmArgs p) {
  using namespace w4cfg;
  using Frag = typename Ops::Frag;
  constexpr int T = Ops::T, EB = Ops::EB;
  constexpr bool B_KC = Ops::B_KC;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PZ_LDS char* smem = (PZ_LDS char*)(smem_raw);
  const int tiles_m = p.M / kW4M, tiles_n = p.N / kW4N;
  int tm, tn, tile_id, slice;
  tile_coords(xcd_remap(blockIdx.x, gridDim.x), tiles_m, tiles_n, 1, tm, tn, tile_id, slice);
  const int m0 = tm * kW4M, n0 = tn * kW4N;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const i32x4_t rs_a = buf_rsrc(p.A), rs_b = buf_rsrc(p.B);
  // DMA lanes of a K-contiguous operand: row lane/8 of an 8-row piece, 16-B chunk lane%8; the chunk
  // swizzle of slot row r is (r >> 1) & 7, which for the piece's base row (a multiple of 8) differs
  // between even and odd pieces by 4 — hence two lane offsets per operand
  const int prow = lane >> 3;
  const int pch0 = (lane & 7) ^ swz_kc<64>(prow), pch1 = (lane & 7) ^ swz_kc<64>(prow + 8);
  const uint32_t lda = static_cast<uint32_t>(p.lda), ldb = static_cast<uint32_t>(p.ldb);
  const uint32_t va0 = (prow * lda + pch0 * (16 / EB)) * EB, va1 = (prow * lda + pch1 * (16 / EB)) * EB;
  uint32_t vb[Ops::NB];
  if constexpr (B_KC) {
    vb[0] = (prow * ldb + pch0 * (16 / EB)) * EB;
    vb[1] = (prow * ldb + pch1 * (16 / EB)) * EB;
  } else {
    static_for<Ops::NB>([&](auto cc) { vb[cc.value] = Ops::b_lane(cc.value, lane, ldb); });
  }
  const uint32_t lds0 = lds_addr(smem);
  const uint32_t abase = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(m0) * lda * EB);
  const uint32_t bbase = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(n0) * (B_KC ? ldb : 1u) * EB);
  // K-step advance of a piece's source: 128 bytes of a K-contiguous row, 128 / EB rows of an
  // M/N-contiguous operand
  const uint32_t bstep = __builtin_amdgcn_readfirstlane(B_KC ? static_cast<uint32_t>(kStepB) : (kStepB / EB) * ldb * EB);
  // piece d (16 per wave and K step): operand d / 8, 1 KiB at (wave * 8 + d % 8) KiB of the slot
  // (K-contiguous: rows 8 (wave * 8 + d % 8) .. + 8; M/N-contiguous B: B_ROWS k-rows from B_ROWS times that)
  uint32_t soff[16], dst[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    const int op = d >> 3;
    const uint32_t piece = static_cast<uint32_t>(wave * 8 + (d & 7));
    if constexpr (B_KC)
      soff[d] = __builtin_amdgcn_readfirstlane((op ? bbase : abase) + piece * 8u * (op ? ldb : lda) * EB);
    else
      soff[d] = __builtin_amdgcn_readfirstlane(op ? bbase + piece * Ops::B_ROWS * ldb * EB : abase + piece * 8u * lda * EB);
    dst[d] = __builtin_amdgcn_readfirstlane(lds0 + static_cast<uint32_t>(op * (kTB / 2)) + piece * 1024u);
  }
  auto dma = [&](int kt, int d) __attribute__((always_inline)) {
    if (d < 8)
      blds16<0>(rs_a, (d & 1) ? va1 : va0, soff[d] + static_cast<uint32_t>(kt) * kStepB,
                dst[d] + static_cast<uint32_t>((kt & 1) * kTB));
    else
      blds16<0>(rs_b, vb[Ops::b_class(d & 7)], soff[d] + static_cast<uint32_t>(kt) * bstep,
                dst[d] + static_cast<uint32_t>((kt & 1) * kTB));
  };
  // fragment f of k-half kh: f < T -> B (output columns), else A (output rows); a K-contiguous
  // operand's fragment covers 128 / T tile rows, one per lane modulo that
  auto frag = [&](int buf, int kh, int f) __attribute__((always_inline)) -> Frag {
    const PZ_LDS char* t = smem + buf * kTB + (f < T ? kTB / 2 : 0);
    if constexpr (!B_KC) {
      if (f < T) return Ops::frag_b(t, kh, wn * 128, f, lane);
    }
    const int row = (f < T ? wn : wm) * 128 + (f & (T - 1)) * (128 / T) + (lane & (128 / T - 1));
    return Ops::frag_k(t, row, kh, lane);
  };
  typename Ops::Acc acc[T][T];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j) acc[i][j] = typename Ops::Acc{};
  auto mm = [&](const Frag (&F)[2 * T], int i, int j) __attribute__((always_inline)) {
    Ops::mma(acc[i][j], F[j], F[T + i]);
  };
  Frag S0[2 * T], S1[2 * T];
  const int nk = p.K / (kStepB / EB);  // >= 2 (w4_shape_ok)
#pragma unroll
  for (int d = 0; d < 16; ++d) dma(0, d);
#pragma unroll
  for (int d = 0; d < 16; ++d) dma(1, d);
  wait_vm<16>();
  __syncthreads();
#pragma unroll
  for (int f = 0; f < 2 * T; ++f) S0[f] = frag(0, 0, f);

  // one K step; DMA: step kt+2 goes out (kt + 2 < nk); NEXT: step kt+1's S0 is read in phase 4
  auto step = [&](int kt, auto dmac, auto nextc) __attribute__((always_inline)) {
    constexpr bool DMA = decltype(dmac)::value, NEXT = decltype(nextc)::value;
    constexpr int G = T / 4;  // MFMAs per fragment read in phases 1 and 4
    const int buf = kt & 1;
    __builtin_amdgcn_sched_barrier(0);
    static_for<2 * T>([&](auto gc) {
      constexpr int q = decltype(gc)::value;
#pragma unroll
      for (int m = q * G; m < (q + 1) * G; ++m) mm(S0, m / T, m % T);
      S1[q] = frag(buf, 1, q);
      __builtin_amdgcn_sched_barrier(0);
    });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();  // every wave has both k-halves of step kt: buffer buf is free
    __builtin_amdgcn_sched_barrier(0);
    static_for<T * T>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      if constexpr (c < T * T / 2) mm(S0, T / 2 + c / T, c % T);
      else mm(S1, c / T - T / 2, c % T);
      constexpr int every = T * T / kD23;
      if constexpr (DMA && c % every == every - 1 && c / every < kD23) {
        dma(kt + 2, c / every);
        __builtin_amdgcn_sched_barrier(0);
      }
    });
    if constexpr (NEXT) {
      if constexpr (DMA) wait_vm<kD23>();  // step kt+1 landed; step kt+2's pieces stay in flight
      else wait_vm<0>();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    static_for<2 * T>([&](auto gc) {
      constexpr int q = decltype(gc)::value;
#pragma unroll
      for (int m = q * G; m < (q + 1) * G; ++m) mm(S1, T / 2 + m / T, m % T);
      if constexpr (NEXT) S0[q] = frag(buf ^ 1, 0, q);
      constexpr int every4 = 2 * T / kD4;
      if constexpr (DMA && q % every4 == every4 - 1) dma(kt + 2, kD23 + q / every4);
      __builtin_amdgcn_sched_barrier(0);
    });
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  int kt = 0;
  for (; kt < nk - 2; ++kt) step(kt, T_{}, T_{});
  step(kt, F_{}, T_{});
  step(kt + 1, F_{}, F_{});
  PZ_STAMP(3);
  // (epilogue_lds opens with a barrier: every wave is done with the operand buffers)
  epilogue_lds<kW4M, kW4N, 2, 2, typename Ops::Lay, Ops::FWD_ONLY, EK>(p, acc, smem, m0, n0, wm, wn, lane, Ops::alpha(p));
}

template <class Ops, int EK>
hipError_t launch_w4(const GemmArgs& p, hipStream_t s) {
  return launch_lds<&w4_kernel<Ops, EK>>(p, (p.M / w4cfg::kW4M) * (p.N / w4cfg::kW4N), w4cfg::kW4T, 2 * w4cfg::kTB, s,
                                         {"w4", Ops::VAR, w4cfg::kW4M, w4cfg::kW4N, EK, 1});
}

// VAR 40 — the bf16 dX GEMM (both operands K-contiguous) on v_mfma_f32_16x16x32_bf16.
// tools/gemm_w4_lab.hip (same box, plain store): dX [8192,4096] K=4096 1436 vs 1387 TF/s (VAR 30),
// K=1024 1095 vs 1040; the diagnostics there put the remaining gap to hipBLASLt (1569) in the
// DMA issue itself (no-DMA build 1690 TF/s; L2-resident operands: no change).
struct W4Bf16 {
  static constexpr int VAR = 40, EB = 2, T = 8, NB = 2;
  static constexpr bool B_KC = true, FWD_ONLY = false;
  using Frag = i16x8_t;
  using Acc = f32x4_t;
  using Lay = Lay16<8, 8>;
  static PZ_DEV int b_class(int i) { return i & 1; }
  static PZ_DEV Frag frag_k(const PZ_LDS char* t, int row, int kh, int lane) {
    return frag_kc<64>(t, row, kh * 4 + (lane >> 4));
  }
  static PZ_DEV void mma(Acc& c, Frag b, Frag a) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, b), __builtin_bit_cast(bf16x8_t, a), c, 0, 0, 0);
  }
  static PZ_DEV float alpha(const GemmArgs& p) { return p.alpha; }
};

// VAR 43 — the fp8 forward X8 (e4m3, K-contiguous) x W8 (e4m3 [in, out], N-contiguous) on
// v_mfma_scale_f32_32x32x64_f8f6f4 (unit E8M0 block scales; the per-tensor dequant scales go into
// the epilogue's alpha). A 128-byte K step of fp8 is the bf16 slot geometry; each 64-byte k-half is
// ONE 32x32x64 MFMA per 32x32 tile, 16 MFMAs of 64 cycles — the bf16 kernel's 64 x 16 cycles — so
// the phases, DMA spread and barriers carry over unchanged. B's K-step slot is [128 k][256 B] (one
// DMA = 4 k-rows, swz_mn8<256>), read per 64-k half with the transposing ds_read_b64_tr_b8
// (frag_mn8) — the same natural-layout weight copy VAR 15 / 16 read. Lab (tools/gemm_w4f8_lab.hip,
// plain store, same box, TF/s median): forward [8192,4096] K=4096 2,464 vs 2,262 (VAR 15),
// [8192,8192] K=1024 1,602 vs 1,598 (VAR 16)
struct W4F8Fwd {
  static constexpr int VAR = 43, EB = 1, T = 4, NB = 2, B_ROWS = 4;
  static constexpr bool B_KC = false, FWD_ONLY = true;
  using Frag = i32x8_t;
  using Acc = f32x16_t;
  using Lay = Lay32<4, 4>;
  static PZ_DEV int b_class(int i) { return i & 1; }
  // B lane offsets: k-row lane / 16 of a 4-row piece, 16-B chunk lane % 16 XOR the k-row's swizzle,
  // whose k-row bits vary with the piece's parity c
  static PZ_DEV uint32_t b_lane(int c, int lane, uint32_t ldb) {
    const int kq = lane >> 4;
    return kq * ldb + ((lane & 15) ^ swz_mn8<256>(4 * c + kq)) * 16;
  }
  // lane l holds row l & 31, k bytes [32 (l >> 5), +32) of the half = 16-B chunks 4 kh + 2 (l >> 5) + {0, 1}
  static PZ_DEV Frag frag_k(const PZ_LDS char* t, int row, int kh, int lane) {
    const int c = 4 * kh + 2 * (lane >> 5);
    return cat_frag(frag_kc<64>(t, row, c), frag_kc<64>(t, row, c + 1));
  }
  static PZ_DEV Frag frag_b(const PZ_LDS char* t, int kh, int col0, int f, int lane) {
    return frag_mn8<256>(t + kh * 64 * 256, col0 + f * 32, lane);  // the half's [64 k][256 B] image
  }
  // issued as mfma(B, A): cbsz = B's format, blgp = A's (both e4m3 = 0); E8M0 127 = 1.0
  static PZ_DEV void mma(Acc& c, Frag b, Frag a) {
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b, a, c, 0, 0, 0, 127, 0, 127);
  }
  static PZ_DEV float alpha(const GemmArgs& p) {
    return p.alpha * (p.scale_a != nullptr ? *p.scale_a : 1.f) * (p.scale_b != nullptr ? *p.scale_b : 1.f);
  }
};
