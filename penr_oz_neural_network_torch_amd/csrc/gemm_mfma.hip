// N1 — bf16 MFMA GEMM for gfx950 with fused MLP epilogues.
//
// Replaces the reference's three per-layer matmuls (neural_net_model.py:117 forward `x @ W`, and
// autograd's two `mm` for dX / dW) plus the bias add (:119), activation (:172-184), dropout (:395)
// and bias-gradient column sum that surround them.
//
// Design (CDNA4-first, /opt/skills/guides/cdna_hip_programming.md §5):
//  * 16x16x32 bf16 MFMA (v_mfma_f32_16x16x32_bf16), fp32 accumulation. Operands are issued
//    SWAPPED (mfma(B, A)) so each lane owns 4 consecutive output COLUMNS of one row: the epilogue
//    loads bias / aux and stores C with 8-16 B per lane.
//  * Both operand layouts are first-class. A K-contiguous operand is staged as [rows][32 k]
//    (64-B rows, 16-B chunks XOR-swizzled per 4-row group, read with ds_read_b128); an
//    M/N-contiguous operand (the reference's [in,out] weights in the forward, activations in
//    dW = XᵀdZ) is staged as [32 k][rows] and read with the gfx950 transposing
//    ds_read_b64_tr_b16 — no transpose kernels, no second weight copy.
//  * global->LDS by global_load_lds_dwordx4 (LDS-DMA, 1 KiB per wave-instruction; swizzle on the
//    per-lane SOURCE address + the read, rule 21).
//  * Pipeline: a ring of NS LDS slots, each one 32- or 64-deep K step (the table below). On the
//    32-deep rings loads run NS-1 steps ahead; each step waits with a COUNTED
//    `s_waitcnt vmcnt((NS-2)G)` (G = LDS-DMA instructions per wave per step) so the NS-2 younger
//    steps stay in flight across the raw `s_barrier` — never a vmcnt(0) drain in the loop (guide
//    "Pipelining across barriers", T3/T4). One barrier per step covers both hazards: RAW (every
//    wave's DMA for slot t landed) and WAR (every wave's reads of slot t-1, which the step
//    re-fills, completed: lgkmcnt(0) before the barrier). The 64-deep 2-slot ring (the default
//    for bf16) is described above its loop in gemm_body.
//  * MFMA clusters bracketed by s_setprio(1)/(0) (T5).
//  * XCD-aware bijective block remap (T1) + grouped tile order for L2 reuse.
//  * Tile configs 256x256 (8 waves), 256x128 (8 waves, or 4 waves with 2 blocks/CU), 128x128
//    (4 waves, 2 blocks/CU), chosen per shape so the grid covers the 256 CUs.
//  * The main loop comes in the numbered variants of the table below (template VAR; the number
//    is what gemm_last reports). VAR 40 / 43, the 4-wave schedule, are in gemm_w4.h. VAR numbers
//    in profiles/ that have no row in the table are deleted experiments: their code is in the
//    history up to commit a839ea0.
#include <array>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "pz_common.h"
#include "gemm_dispatch.h"

namespace pz {
namespace {

constexpr int kBK = 32;  // K depth of one MFMA K block (a 64-deep ring slot holds two)

#include "gemm_common.h"  // LDS-DMA, swizzles, fragment reads, tile order (shared with gemm_sk.hip)

// fp8 operand forms: what the bytes of A and B look like in memory
enum F8Form {
  F8_NONE,   // bf16 operands
  F8_KC_KC,  // both K-contiguous ([M][K] x [N][K] bytes)
  F8_KC_MN,  // A K-contiguous, B [K][N] (the e4m3 weights in their natural [in, out] layout)
  F8_MN_MN,  // A [K][M] e4m3, B [K][N] e5m2 (the weight gradient; K = batch rows)
};

// One row per main-loop variant: everything gemm_body does differently for a VAR number.
struct Variant {
  int var;           // the template key and what gemm_last reports
  int bk;            // K depth of a ring slot in 16-bit units (fp8: twice as many K bytes)
  int ns;            // ring slots
  int waves_per_eu;  // 2: 4-wave workgroups sized so that two share a CU
  bool buf;          // stage_kc / stage_mn address through a buffer descriptor, not flat pointers
  bool full_kc;      // K-contiguous operands are staged as full row tiles, without a row clamp
  F8Form f8;
  bool a_e5m2;       // fp8: A holds e5m2 gradients (the backward dX GEMM, EPI_BWD epilogues)
};

// LDS-DMA addressing, measured (tools/gemm_lab, same box): buffer is +6..10% on the M/N-contiguous
// operands, whose k-row addresses otherwise cost 64-bit multiplies every step, and 1.5..5% slower
// on K-contiguous ones (measured, not kept: VAR 25 = buffer for M/N-contiguous only). The
// M/N-contiguous fp8 operands (stage_mn8) are always buffer-addressed, whatever `buf` says.
constexpr Variant kVariants[] = {
    // {var, bk, ns, waves_per_eu, buf, full_kc, f8, a_e5m2}
    // 0: flat DMA on the 4-slot 32-deep ring: operands that reach past 4 GiB from their base
    {0, 32, 4, 1, false, false, F8_NONE, false},
    // 6: buffer DMA on the 4-slot 32-deep ring: what 30 does not take (ragged tiles, K % 64,
    // 128x128 tiles)
    {6, 32, 4, 1, true, false, F8_NONE, false},
    // 7: buffer DMA on a 3-slot 32-deep ring, for 4-wave 256x128 tiles that run TWO workgroups
    // per CU (72 KiB of LDS and <= 256 VGPRs each): one workgroup's epilogue overlaps the other's
    // main loop (the hardware interleaves the two instead of a barrier-phased ping-pong).
    // Measured by tools/gemm_stamps, not dispatched for bf16
    {7, 32, 3, 2, true, false, F8_NONE, false},
    // 8: e4m3 x e4m3, both K-contiguous, v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales:
    // a ring slot holds 64 K-bytes per row (the bf16 slot geometry), one MFMA K-step
    {8, 32, 4, 1, false, false, F8_KC_KC, false},
    // 9: A in e5m2 (bf8: gradients, wide range), B in e4m3 — the backward dX GEMM dZ8 · W8ᵀ of
    // the fp8 policy, with the backward (EPI_BWD) epilogues
    {9, 32, 4, 1, false, false, F8_KC_KC, true},
    // 14: the fp8 weight-gradient GEMM dW = X8ᵀ · dZ8 — e4m3 activations (A) x e5m2 output
    // gradients (B), BOTH M/N-contiguous, staged as k-row images and read with the transposing
    // ds_read_b64_tr_b8 (no transposed copies), bf16 output
    {14, 32, 4, 1, false, false, F8_MN_MN, false},
    // 15: the fp8 forward X8 · W8 with the e4m3 weights in their natural [in, out] layout (B
    // N-contiguous, transposing 8-bit reads) — the same copy the backward dX GEMM reads as its
    // K-contiguous B, so one e4m3 weight copy serves both and no transposed copy is made
    {15, 32, 4, 1, false, false, F8_KC_MN, false},
    // 16 / 17: the fp8 forward (15) / e5m2 x e4m3 dX (9) the way of 7 — 4-wave 256x128 tiles,
    // 3-slot ring (72 KiB), two workgroups per CU: at K = 1024 an fp8 tile's epilogue (the stage
    // math, the e4m3 / e5m2 copies, the bitmask) costs about what its main loop does, and the
    // other workgroup's MFMAs run through it
    {16, 32, 3, 2, false, false, F8_KC_MN, false},
    {17, 32, 3, 2, false, false, F8_KC_KC, true},
    // 30: buffer DMA on a 2-slot 64-deep ring (two 64 KiB slots: one MFMA interval = 64 MFMAs per
    // wave, half the barriers per FLOP of the 32-deep ring), the bf16 default. Full row tiles of
    // the K-contiguous operands only (use_bk64 checks M % BM, N % BN)
    {30, 64, 2, 1, true, true, F8_NONE, false},
};

constexpr Variant variant(int var) {
  for (const Variant& v : kVariants)
    if (v.var == var) return v;
  return {-1, 32, 4, 1, false, false, F8_NONE, false};  // no row: gemm_body refuses to compile
}

template <int BM, int BN, int WM, int WN, int NS_ = 4, int BK_ = 32>
struct Cfg {
  static constexpr int BK = BK_;
  // ring depth in 32-deep K slots. Measured on the step's GEMMs: 5 slots for 256x256 (160 KiB)
  // and 6 for 256x128 are 2-4% SLOWER than 4 (the DMA stream is throughput-, not latency-bound),
  // and 5 slots for 128x128 drop it to one workgroup per CU (-20%).
  static constexpr int NS = NS_;
  static constexpr int NW = WM * WN;
  static constexpr int NT = NW * 64;
  static constexpr int WTM = BM / WM;
  static constexpr int WTN = BN / WN;
  static constexpr int TM = WTM / 16;
  static constexpr int TN = WTN / 16;
  static constexpr int A_BYTES = BM * BK * 2;
  static constexpr int B_BYTES = BN * BK * 2;
  static constexpr int SLOT_BYTES = A_BYTES + B_BYTES;
  static constexpr int LDS_BYTES = NS * SLOT_BYTES;  // the epilogues' BM x BN bf16 C image fits the ring
  static constexpr int GA = A_BYTES / 1024 / NW;  // LDS-DMA instructions per wave per slot
  static constexpr int GB = B_BYTES / 1024 / NW;
  static constexpr int G = GA + GB;
  static_assert(TM >= 1 && TN >= 1, "wave tile must hold at least one 16x16 MFMA tile");
  static_assert(GA >= 1 && GB >= 1 && GA * 1024 * NW == A_BYTES && GB * 1024 * NW == B_BYTES, "stage split");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  static_assert(BM * BN * 2 <= LDS_BYTES, "epilogue_lds keeps the tile's bf16 C image in the ring");
};


template <int RB, int NW, int KROWS>
PZ_DEV void stage_mn8(int64_t ld16, int col0, int k0, PZ_LDS char* tile, int wave, int lane, i32x4_t rs) {
  constexpr int CHUNKS = RB / 16;
  constexpr int ROWS_PER = 1024 / RB;
  constexpr int INSTR = (KROWS * RB) / (1024 * NW);
  static_assert(INSTR >= 1 && INSTR * 1024 * NW == KROWS * RB, "fp8 M/N-contiguous stage split");
#pragma unroll
  for (int i = 0; i < INSTR; ++i) {
    const int kbase = (wave * INSTR + i) * ROWS_PER;
    const int kr = kbase + lane / CHUNKS;
    const int chunk = (lane % CHUNKS) ^ swz_mn8<RB>(kr);
    const uint32_t voff = (static_cast<uint32_t>(kr) * static_cast<uint32_t>(ld16)) * 2u +
                          static_cast<uint32_t>(col0 + chunk * 16);
    blds16<0>(rs, voff, __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(k0) * static_cast<uint32_t>(ld16) * 2u),
              lds_addr(tile + kbase * RB));
  }
}


// fp32-output store epilogue (dW / plain GEMMs): alpha, bias, optional accumulate, 16-B stores.
// The fused stage epilogues only exist for bf16 outputs (epilogue_lds); mfma_eligible routes
// anything else to the generic kernel.
template <typename OutT, typename AuxT>
PZ_DEV f32x4_t epi_apply(const GemmArgs& p, f32x4_t a, f32x4_t bias4, int m, int n, OutT* __restrict__ Cp,
                         const AuxT* __restrict__ aux) {
  (void)aux;
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = a[r] * p.alpha + bias4[r];
  OutT* dst = Cp + static_cast<int64_t>(m) * p.ldc + n;
  if (p.accumulate) {
    float old[4];
    load4<OutT>(dst, old);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += old[r];
  }
  store4<OutT>(dst, v);
  return f32x4_t{v[0], v[1], v[2], v[3]};
}


#include "gemm_epilogue.h"

// EPI_OPT: the tile's accumulators are a block of the weight gradient g = alpha*AB; instead of
// storing it (and a separate optimizer pass reading it back), apply the optimizer update of the
// weight right here (GemmOpt). Each lane owns 4 consecutive columns of one row per fragment
// (acc[i][j]: m = lane & 15, n = 4*(lane >> 4)), so p / m / v move as 16-B vectors like the fp32
// C store they replace. The per-tile statistics (update-ratio sums, sum(w^2), amax) are reduced
// in LDS and leave as one atomic per accumulator.
template <class C, class Acc>
PZ_DEV void epilogue_opt(const GemmArgs& p, Acc& acc, PZ_LDS char* smem, int m0, int n0, int wm, int wn, int lane) {
  const GemmOpt& o = p.opt;
  float lr = o.lr, bc1 = o.bias_c1, bc2s = o.bias_c2_sqrt;
  int epoch = -1;
  if (o.epoch_ptr != nullptr) epoch = *o.epoch_ptr;
  if (o.hp != nullptr) {  // graph-replayed step: this epoch's hyper-parameters
    const double* h = o.hp + 4 * static_cast<int64_t>(epoch);
    lr = static_cast<float>(h[0]);
    bc1 = static_cast<float>(h[1]);
    bc2s = static_cast<float>(h[2]);
  }
  const bool full = o.stats_every == 1 || (o.stats_every > 1 && (epoch < 0 || epoch % o.stats_every == 0));
  const float step_size = lr / bc1;
  const bool adam = o.adam != 0;
  const int g4 = 4 * (lane >> 4);
  double st[4] = {0.0, 0.0, 0.0, 0.0};
  float am = 0.f;
  static_for<C::TN>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const int n = n0 + wn * C::WTN + j * 16 + g4;
    static_for<C::TM>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const int m = m0 + wm * C::WTM + i * 16 + (lane & 15);
      if (n < p.N && m < p.M) {
        const int64_t gi = static_cast<int64_t>(m) * p.ldc + n;
        const f32x4_t p0 = *reinterpret_cast<const f32x4_t*>(o.params + gi);
        f32x4_t mm = {0.f, 0.f, 0.f, 0.f}, vv = mm, p1;
        if (adam) {
          mm = *reinterpret_cast<const f32x4_t*>(o.exp_avg + gi);
          vv = *reinterpret_cast<const f32x4_t*>(o.exp_avg_sq + gi);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float graw = acc[i][j][r] * p.alpha;
          float mr = mm[r], vr = vv[r];
          p1[r] = adam ? opt_update<true>(p0[r], graw, o.grad_scale, o.l2x2, lr, step_size, o.beta1, o.beta2, bc2s,
                                          o.eps, mr, vr)
                       : opt_update<false>(p0[r], graw, o.grad_scale, o.l2x2, lr, step_size, 0.f, 0.f, 1.f, 0.f, mr,
                                           vr);
          mm[r] = mr;
          vv[r] = vr;
        }
        if (adam) {
          *reinterpret_cast<f32x4_t*>(o.exp_avg + gi) = mm;
          *reinterpret_cast<f32x4_t*>(o.exp_avg_sq + gi) = vv;
        }
        *reinterpret_cast<f32x4_t*>(o.params + gi) = p1;
        if (o.shadow != nullptr) {
          if (o.shadow_dtype == DT_BF16)
            *reinterpret_cast<u32x2_t*>(static_cast<uint16_t*>(o.shadow) + gi) =
                u32x2_t{pack_bf2(p1[0], p1[1]), pack_bf2(p1[2], p1[3])};
          else
            *reinterpret_cast<f32x4_t*>(static_cast<float*>(o.shadow) + gi) = p1;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          st[3] += static_cast<double>(p1[r]) * p1[r];
          if (full) {
            const double d = static_cast<double>(p1[r] - p0[r]);
            st[0] += d;
            st[1] += d * d;
            st[2] += p1[r];
          }
          am = fmaxf(am, fabsf(p1[r]));
        }
      }
    });
  });
  const bool want_st = o.stats != nullptr, want_am = o.amax != nullptr;
  if (!want_st && !want_am) return;
  constexpr int NW = C::NT / 64;
#pragma unroll
  for (int k = 0; k < 4; ++k) st[k] = wave_sum_d(st[k]);
  am = wave_max(am);
  __syncthreads();  // every wave is past its last ring read: the LDS is free
  PZ_LDS double* part = (PZ_LDS double*)(smem);  // [NW][5]
  const int w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) part[w * 5 + k] = st[k];
    part[w * 5 + 4] = am;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < 5) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) s = k == 4 ? fmax(s, part[q * 5 + 4]) : s + part[q * 5 + k];
    if (k < 4 && want_st && (full || k == 3)) atomicAdd(o.stats + k, s);
    if (k == 4 && want_am)  // non-negative floats order like their bits
      atomicMax(reinterpret_cast<unsigned int*>(o.amax), __float_as_uint(static_cast<float>(s)));
  }
}


// The body of one workgroup: the GEMM `p`, workgroup `wgid` of its (XCD-remapped) grid
template <int BM, int BN, int WM, int WN, bool A_KC, bool B_KC, typename OutT, typename AuxT, int VAR, int EK = EK_ANY>
PZ_DEV void gemm_body(const GemmArgs& p, int wgid) {
  static_assert(EK == EK_ANY || std::is_same<OutT, uint16_t>::value, "specialised epilogues: bf16 output");
  PZ_STAMP(0);
  constexpr Variant V = variant(VAR);
  static_assert(V.var == VAR, "this VAR has no row in kVariants: a deleted experiment (see the header comment)?");
  constexpr int BK = V.bk;
  constexpr int KB = BK / 32;  // 32-deep MFMA K blocks per ring slot
  using C = Cfg<BM, BN, WM, WN, V.ns, BK>;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PZ_LDS char* smem = (PZ_LDS char*)(smem_raw);

  const int tiles_m = (p.M + BM - 1) / BM;
  const int tiles_n = (p.N + BN - 1) / BN;
  const int split = p.split_k > 1 ? p.split_k : 1;
  int tm, tn, tile_id, slice;
  tile_coords(wgid, tiles_m, tiles_n, split, tm, tn, tile_id, slice);
  const int m0 = tm * BM, n0 = tn * BN;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int wm = wave / WN, wn = wave % WN;
  const uint16_t* __restrict__ A = static_cast<const uint16_t*>(p.A);
  const uint16_t* __restrict__ B = static_cast<const uint16_t*>(p.B);

  constexpr bool F8_MN = V.f8 == F8_MN_MN;
  constexpr bool F8_MNB = V.f8 == F8_KC_MN;
  constexpr bool F8 = V.f8 != F8_NONE;  // 32x32 accumulator tiles
  constexpr int F8_FMT_A = V.a_e5m2 ? 1 : 0;  // MFMA format codes: 0 = fp8 e4m3, 1 = bf8 e5m2
  constexpr int F8_FMT_B = F8_MN ? 1 : 0;
  static_assert(!F8 || ((F8_MN ? (!A_KC && !B_KC) : F8_MNB ? (A_KC && !B_KC) : (A_KC && B_KC)) &&
                         std::is_same<OutT, uint16_t>::value),
                "fp8: the operand layouts of the variant's F8Form, bf16 out");
  // (measured, not kept: bf16 on v_mfma_f32_32x32x16_bf16, VAR 41, profiles/r2_ab_mfma_32x32_vs_16x16.txt)
  constexpr int TM8 = C::WTM / 32, TN8 = C::WTN / 32;
  struct Frags16 { i16x8_t a[KB][C::TM]; i16x8_t b[KB][C::TN]; };
  struct Frags8 { i32x8_t a[KB][TM8]; i32x8_t b[KB][TN8]; };  // KB MFMA K-steps of 64 bytes
  using Frags = std::conditional_t<F8, Frags8, Frags16>;
  using AccT = std::conditional_t<F8, f32x16_t[TM8][TN8], f32x4_t[C::TM][C::TN]>;
  AccT acc;
  if constexpr (F8) {
#pragma unroll
    for (int i = 0; i < TM8; ++i)
#pragma unroll
      for (int j = 0; j < TN8; ++j) acc[i][j] = f32x16_t{};
  } else {
#pragma unroll
    for (int i = 0; i < C::TM; ++i)
#pragma unroll
      for (int j = 0; j < C::TN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // GemmArgs::prio = 0 (PZ_GEMM_PRIO=0) drops the s_setprio bracket around the MFMA block at run
  // time (a uniform scalar branch per MFMA block). (measured, not kept: compiled out, VAR 33 —
  // profiles/r4_ab_session.txt: its apparent gain came from run order)
  const bool prio = p.prio != 0;
  auto mfma_step = [&](const Frags& f) {
    if (prio) __builtin_amdgcn_s_setprio(1);
    if constexpr (F8) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int i = 0; i < TM8; ++i)
#pragma unroll
          for (int j = 0; j < TN8; ++j)  // issued as mfma(B, A): cbsz = B's format, blgp = A's;
                                         // E8M0 block scales 127 = 1.0
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(f.b[kb][j], f.a[kb][i], acc[i][j], F8_FMT_B,
                                                                         F8_FMT_A, 0, 127, 0, 127);
    } else {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int i = 0; i < C::TM; ++i)
#pragma unroll
          for (int j = 0; j < C::TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, f.b[kb][j]),
                                                                __builtin_bit_cast(bf16x8_t, f.a[kb][i]), acc[i][j], 0, 0, 0);
    }
    if (prio) __builtin_amdgcn_s_setprio(0);
  };
  auto read_frags = [&](int slot, Frags& f) {
    const PZ_LDS char* ta = smem + slot * C::SLOT_BYTES;
    const PZ_LDS char* tb = ta + C::A_BYTES;
    if constexpr (F8_MNB) {  // A: 16-B chunks of K-contiguous rows; B: transposing 8-bit reads
      const int h2 = 2 * (lane >> 5);
#pragma unroll
      for (int j = 0; j < TN8; ++j) f.b[0][j] = frag_mn8<BN>(tb, wn * C::WTN + j * 32, lane);
#pragma unroll
      for (int i = 0; i < TM8; ++i) {
        const int row = wm * C::WTM + i * 32 + (lane & 31);
        f.a[0][i] = cat_frag(frag_kc<BK>(ta, row, h2), frag_kc<BK>(ta, row, h2 + 1));
      }
    } else if constexpr (F8_MN) {  // transposing 8-bit reads of the [64 k][256 B] images (KB == 1)
#pragma unroll
      for (int j = 0; j < TN8; ++j) f.b[0][j] = frag_mn8<BN>(tb, wn * C::WTN + j * 32, lane);
#pragma unroll
      for (int i = 0; i < TM8; ++i) f.a[0][i] = frag_mn8<BM>(ta, wm * C::WTM + i * 32, lane);
    } else if constexpr (F8) {  // lane l: row l&31, K bytes [32*(l>>5), +32) of K-step kb = 16-B chunks
                                // 4kb + 2h, 4kb + 2h + 1
      const int h2 = 2 * (lane >> 5);
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int j = 0; j < TN8; ++j) {
          const int row = wn * C::WTN + j * 32 + (lane & 31);
          f.b[kb][j] = cat_frag(frag_kc<BK>(tb, row, 4 * kb + h2), frag_kc<BK>(tb, row, 4 * kb + h2 + 1));
        }
#pragma unroll
        for (int i = 0; i < TM8; ++i) {
          const int row = wm * C::WTM + i * 32 + (lane & 31);
          f.a[kb][i] = cat_frag(frag_kc<BK>(ta, row, 4 * kb + h2), frag_kc<BK>(ta, row, 4 * kb + h2 + 1));
        }
      }
    } else {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int j = 0; j < C::TN; ++j) {
          if constexpr (B_KC) f.b[kb][j] = frag_kc<BK>(tb, wn * C::WTN + j * 16 + (lane & 15), (lane >> 4) + 4 * kb);
          else f.b[kb][j] = frag_mn<BN>(tb, wn * C::WTN + j * 16, 8 * (lane >> 4) + 32 * kb, lane);
        }
#pragma unroll
        for (int i = 0; i < C::TM; ++i) {
          if constexpr (A_KC) f.a[kb][i] = frag_kc<BK>(ta, wm * C::WTM + i * 16 + (lane & 15), (lane >> 4) + 4 * kb);
          else f.a[kb][i] = frag_mn<BM>(ta, wm * C::WTM + i * 16, 8 * (lane >> 4) + 32 * kb, lane);
        }
      }
    }
  };
  auto barrier = [] {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  const int nk = p.K / (F8 ? 2 * BK : BK) / split;  // K steps of this slice (fp8: 2 bytes per 16-bit unit)
  const int kt0 = slice * nk;
  const i32x4_t rs_a = buf_rsrc(A), rs_b = buf_rsrc(B);
  // staging works in 16-bit units: an e4m3 row of 64 K-bytes is the same 64-B piece
  const int64_t lda = F8 ? p.lda / 2 : p.lda, ldb = F8 ? p.ldb / 2 : p.ldb;
  // (measured, not kept: DMA issued by waves 0-3 only, twice the instructions each: -2..4%)
  constexpr int NWD = C::NW;
  // TEAM waves (team-local index tw) issue one operand's DMA of a step
  auto stage_a_t = [&](int kt, auto team, int tw) {
    constexpr int TEAM = decltype(team)::value;
    PZ_LDS char* base = smem + (kt % C::NS) * C::SLOT_BYTES;
    if constexpr (F8_MN) stage_mn8<BM, TEAM, 64>(lda, m0, (kt0 + kt) * 64, base, tw, lane, rs_a);
    else if constexpr (A_KC) stage_kc<BM, TEAM, BK, V.buf, V.full_kc>(A, lda, m0, p.M, (kt0 + kt) * BK, base, tw, lane, rs_a);
    else stage_mn<BM, TEAM, BK, V.buf>(A, lda, m0, p.M, (kt0 + kt) * BK, base, tw, lane, rs_a);
  };
  auto stage_b_t = [&](int kt, auto team, int tw) {
    constexpr int TEAM = decltype(team)::value;
    PZ_LDS char* base = smem + (kt % C::NS) * C::SLOT_BYTES + C::A_BYTES;
    if constexpr (F8_MN || F8_MNB) stage_mn8<BN, TEAM, 64>(ldb, n0, (kt0 + kt) * 64, base, tw, lane, rs_b);
    else if constexpr (B_KC) stage_kc<BN, TEAM, BK, V.buf, V.full_kc>(B, ldb, n0, p.N, (kt0 + kt) * BK, base, tw, lane, rs_b);
    else stage_mn<BN, TEAM, BK, V.buf>(B, ldb, n0, p.N, (kt0 + kt) * BK, base, tw, lane, rs_b);
  };
  auto stage_a = [&](int kt) { stage_a_t(kt, std::integral_constant<int, NWD>{}, wave); };
  auto stage_b = [&](int kt) { stage_b_t(kt, std::integral_constant<int, NWD>{}, wave); };
  auto stage = [&](int kt) {
    stage_a(kt);
    stage_b(kt);
  };

  constexpr int NS = C::NS;
  // Measured, not kept: staging K-contiguous operands in PAIRS of steps so both 64-B halves of
  // every 128-B line are requested back to back (halved L1->L2 requests, matched hipBLASLt's
  // request count) ran 2-4% SLOWER than the plain ring.
  if constexpr (BK == 64) {
    // Ping-pong over 64-deep steps in a 2-slot ring: waves 0-3 (G0) issue every DMA of step t+1
    // in their read interval R_t. Interval 2t: G0 R_t | G1 M_{t-1}; interval 2t+1: G0 M_t | G1 R_t.
    // Slot (t+1)%2 was last read by G1 in interval 2t-1, so step t+1 is issued in interval 2t and
    // awaited (vmcnt(0)) at the end of interval 2t+1 by every wave, before G0 reads it in 2t+2.
    // (measured, not kept: waves 4-7 staging B at the head of their MFMA interval, VAR 31,
    // profiles/r5_ab_split_staging.txt)
    static_assert(C::NW == 8, "BK64 ping-pong needs 8 waves");
    const int grp = wave >> 2, tw = wave & 3;
    using T4 = std::integral_constant<int, 4>;
    auto stage_g0 = [&](int kt) {
      stage_a_t(kt, T4{}, tw);
      stage_b_t(kt, T4{}, tw);
    };
    stage(0);
    wait_vm<0>();
    barrier();
    PZ_STAMP(1);
    if (grp == 1) barrier();
    for (int t = 0; t < nk; ++t) {
      if (grp == 0 && t + 1 < nk) stage_g0(t + 1);
      Frags f;
      read_frags(t % 2, f);
      if (grp == 1) wait_vm<0>();  // step t+1 (issued in M_{t-1}) landed before interval 2t+2
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      barrier();
      mfma_step(f);
      if (grp == 0) wait_vm<0>();
      barrier();
    }
    if (grp == 0) barrier();
    PZ_STAMP(2);
  } else {
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nk) stage(s);

  if constexpr (C::NW == 8) {
    // Ping-pong (8 waves = 2 per SIMD). Waves 0-3 and 4-7 sit on the same four SIMDs and run one
    // barrier interval apart: while one wave of a SIMD issues its MFMA block (setprio 1) its
    // partner issues the next step's LDS-DMA + fragment reads into the MFMA gaps. Per wave and
    // step t: R_t = {stage t+NS-1, [group 1: wait until step t+1 landed], read slot t,
    // lgkmcnt(0)} | barrier | M_t = {MFMAs, [group 0: wait until step t+1 landed]} | barrier.
    // Group 0 runs one interval AHEAD, so its wait can sit at the end of its MFMA block (one
    // interval more of DMA latency hidden: +2..6%) and still precede the barrier that opens
    // R_{t+1} for both groups. Hazards: slot t+1 is waited for by every wave before that barrier;
    // slot (t+NS-1)%NS = (t-1)%NS was last read in R_{t-1} and every wave retired those reads
    // (lgkmcnt(0)) before the barrier that precedes R_t of either group.
    const int grp = wave >> 2;
    auto wait_step = [&](int n) { wait_newer<C::G, NS - 2>(n); };
    wait_step(min(nk, NS - 1) - 1);  // step 0 landed
    barrier();
    PZ_STAMP(1);
    if (grp == 1) barrier();
    for (int t = 0; t < nk; ++t) {
      if (t + NS - 1 < nk) stage(t + NS - 1);
      if (grp == 1) wait_step(min(nk - 1, t + NS - 1) - (t + 1));  // step t+1 landed
      Frags f;
      read_frags(t % NS, f);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      barrier();
      mfma_step(f);
      if (grp == 0) wait_step(min(nk - 1, t + NS - 1) - (t + 1));
      barrier();
    }
    if (grp == 0) barrier();
    PZ_STAMP(2);
  } else {
  PZ_STAMP(1);  // (4-wave tiles: before the first wait)
  for (int t = 0; t < nk; ++t) {
    // slot t landed: everything newer than step t (at most NS-2 steps) may stay in flight
    wait_newer<C::G, NS - 2>(min(nk - 1, t + NS - 2) - t);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + NS - 1 < nk) stage(t + NS - 1);
    Frags f;
    read_frags(t % NS, f);
    mfma_step(f);
  }
  PZ_STAMP(2);
  }
  }  // BK

  // ---------------------------------------------------------------- split-K reduction
  // Write-through hand-off (MI355X_MICROARCH "publish-large" / "splitk-seam", hand-off table row
  // 1): every slice stores its fp32 slab with `sc1` (write-through) 16-B buffer stores, drains
  // them (vmcnt(0)), joins a barrier, and ONE lane takes a relaxed agent-scope ticket; the slice
  // whose add returned split-1 sums the other slabs with `sc1` loads (after a barrier its waves
  // join) and runs the epilogue. No release fence (its L2 write-back of every dirty line of the
  // XCD cost ~2.7x the publish, measured 19-23 us of a split-K GEMM's 85-95 us) and no acquire.
  // (measured, not kept: plain stores + agent release / acquire fences, VAR 32)
  if (split > 1) {
    constexpr int CH = F8 ? TM8 * TN8 * 4 : C::TM * C::TN;  // f32x4 chunks per lane
    const int tid = threadIdx.x;
    auto get_chunk = [&](auto cc) -> f32x4_t {
      constexpr int c = decltype(cc)::value;
      if constexpr (F8) {
        constexpr int i = (c / 4) / TN8, j = (c / 4) % TN8, q = 4 * (c % 4);
        return f32x4_t{acc[i][j][q], acc[i][j][q + 1], acc[i][j][q + 2], acc[i][j][q + 3]};
      } else {
        return acc[c / C::TN][c % C::TN];
      }
    };
    static_assert(CH % 8 == 0, "the fold runs 8 chunks at a time");
    constexpr int kSlabBytes = BM * BN * 4;
    // one descriptor per tile's slab group (split x 256 KiB: 32-bit offsets always suffice)
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(p.ws + static_cast<int64_t>(tile_id) * split * (BM * BN), 0,
                                                      split * kSlabBytes, 0x00020000);
    constexpr int kSc1 = 16;  // cache-policy bit sc1
    static_for<CH>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, get_chunk(cc)), rs,
                                             slice * kSlabBytes + (c * C::NT + tid) * 16, 0, kSc1);
    });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    PZ_LDS int* flag = (PZ_LDS int*)(smem);
    if (tid == 0) {
      const int prev = __hip_atomic_fetch_add(p.counters + tile_id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *flag = prev == split - 1;
      if (prev == split - 1) p.counters[tile_id] = 0;  // ready for the next launch
    }
    __syncthreads();
    if (*flag == 0) return;  // block-uniform: another slice finishes this tile
    // The sum order must not depend on which slice arrived last (deterministic results): a fixed
    // pairwise tree ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) whose leaf pairs and subtree
    // pairs are each added in either order — float addition commutes exactly — so the last
    // arriver starts from its own slice in registers and loads only the split - 1 others.
    auto ld = [&](int sl, int c) {
      return __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, sl * kSlabBytes + (c * C::NT + tid) * 16, 0, kSc1));
    };
    const int mate = slice ^ 1, pair2 = (slice ^ 2) & ~1, quad4 = (slice ^ 4) & ~3;
    static_for<CH / 8>([&](auto gc) {  // 8 chunks at a time: bounded temporaries
      static_for<8>([&](auto qc) {
        constexpr int c = 8 * decltype(gc)::value + decltype(qc)::value;
        f32x4_t v = get_chunk(std::integral_constant<int, c>{}) + ld(mate, c);
        if (split >= 4) v = v + (ld(pair2, c) + ld(pair2 + 1, c));
        if (split >= 8) v = v + ((ld(quad4, c) + ld(quad4 + 1, c)) + (ld(quad4 + 2, c) + ld(quad4 + 3, c)));
        if constexpr (F8) {
          constexpr int i = (c / 4) / TN8, j = (c / 4) % TN8, q = 4 * (c % 4);
          acc[i][j][q] = v[0]; acc[i][j][q + 1] = v[1]; acc[i][j][q + 2] = v[2]; acc[i][j][q + 3] = v[3];
        } else {
          acc[c / C::TN][c % C::TN] = v;
        }
      });
      __builtin_amdgcn_sched_barrier(0);
    });
  }

  // ---------------------------------------------------------------- epilogue
  // static_for (not #pragma unroll): the acc array must only ever be indexed by compile-time
  // constants or it is demoted to scratch (guide §5.4 rule 20)
  PZ_STAMP(3);
  OutT* __restrict__ Cp = static_cast<OutT*>(p.C);
  const AuxT* __restrict__ aux = static_cast<const AuxT*>(p.aux);
  const int g4 = 4 * (lane >> 4);
  if constexpr (F8) {
    const float alpha = p.alpha * (p.scale_a != nullptr ? *p.scale_a : 1.f) * (p.scale_b != nullptr ? *p.scale_b : 1.f);
    if constexpr (V.a_e5m2) epilogue_lds<BM, BN, WM, WN, Lay32<TM8, TN8>, false, EK>(p, acc, smem, m0, n0, wm, wn, lane, alpha);
    else epilogue_lds<BM, BN, WM, WN, Lay32<TM8, TN8>, true, EK>(p, acc, smem, m0, n0, wm, wn, lane, alpha);
  } else if constexpr (std::is_same<OutT, uint16_t>::value) {
    epilogue_lds<BM, BN, WM, WN, Lay16<C::TM, C::TN>, false, EK>(p, acc, smem, m0, n0, wm, wn, lane, p.alpha);
  } else if (p.epi_mode == EPI_OPT) {
    epilogue_opt<C>(p, acc, smem, m0, n0, wm, wn, lane);
  } else {
  static_for<C::TN>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const int n = n0 + wn * C::WTN + j * 16 + g4;
    const bool n_ok = n < p.N;
    f32x4_t bias4 = {0.f, 0.f, 0.f, 0.f};
    if (p.bias != nullptr && n_ok) bias4 = *reinterpret_cast<const f32x4_t*>(p.bias + n);
    f32x4_t cs = {0.f, 0.f, 0.f, 0.f};
    static_for<C::TM>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const int m = m0 + wm * C::WTM + i * 16 + (lane & 15);
      if (n_ok && m < p.M) cs += epi_apply<OutT, AuxT>(p, acc[i][j], bias4, m, n, Cp, aux);
    });
    if (p.colsum != nullptr) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = group_sum<16>(cs[r]);
        if ((lane & 15) == 0 && n + r < p.N) atomicAdd(p.colsum + n + r, s);
      }
    }
  });
  }
#ifdef PZ_GEMM_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the tile's stores have left this CU
  __syncthreads();
  PZ_STAMP(4);
#endif
}

template <int BM, int BN, int WM, int WN, bool A_KC, bool B_KC, typename OutT, typename AuxT, int VAR, int EK = EK_ANY>
__global__ void __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(variant(VAR).waves_per_eu)))
gemm_mfma_kernel(const GemmArgs p) {
  gemm_body<BM, BN, WM, WN, A_KC, B_KC, OutT, AuxT, VAR, EK>(p, xcd_remap(blockIdx.x, gridDim.x));
}

#include "gemm_w4.h"  // VAR 40 / 43: the 4-wave LDS-DMA schedule (hipBLASLt's dX kernel)

// Two independent GEMMs of one layout / epilogue kind in ONE launch (gemm_pair): the first nwg0
// remapped workgroup ids run GEMM 0, the rest GEMM 1 — e.g. the two skinny weight-gradient GEMMs
// of a 3-layer MLP (64 tiles each at batch 8192) that alone would each need a 4-way split-K to
// fill the CUs: together they fill them with a 2-way split (or none), half (or none) of the slab
// hand-offs, and one launch instead of two
struct GemmPairArgs {
  GemmArgs p[2];
  int nwg0;
};

template <int BM, int BN, int WM, int WN, bool A_KC, bool B_KC, typename OutT, typename AuxT, int VAR, int EK = EK_ANY>
__global__ void __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(variant(VAR).waves_per_eu)))
gemm_mfma_pair_kernel(const GemmPairArgs g) {
  const int w = xcd_remap(blockIdx.x, gridDim.x);
  const int second = w >= g.nwg0 ? 1 : 0;  // workgroup-uniform
  gemm_body<BM, BN, WM, WN, A_KC, B_KC, OutT, AuxT, VAR, EK>(g.p[second], w - second * g.nwg0);
}

template <int BM, int BN, int WM, int WN, bool A_KC, bool B_KC, typename OutT, typename AuxT, int VAR, int EK = EK_ANY>
hipError_t launch_cfg(const GemmArgs& p, hipStream_t s) {
  using C = Cfg<BM, BN, WM, WN, variant(VAR).ns, variant(VAR).bk>;
  const int split = p.split_k > 1 ? p.split_k : 1;
  return launch_lds<&gemm_mfma_kernel<BM, BN, WM, WN, A_KC, B_KC, OutT, AuxT, VAR, EK>>(
      p, tiles(p, BM, BN) * split, C::NT, C::LDS_BYTES, s, {"mfma", VAR, BM, BN, EK, split});
}

#ifndef PZ_GEMM_LAB  // tools/gemm_lab.hip instantiates only the variants it measures
// The launchers of gemm_dispatch.h's kTiled, row by row and layout by layout (index 2 * a_kc +
// b_kc; null where the row is not built for that layout): every tiled kernel the library holds
using Launcher = hipError_t (*)(const GemmArgs&, hipStream_t);

template <int I, int LAY>
constexpr Launcher tiled_launcher() {
  constexpr TiledKey k = kTiled[I];
  if constexpr (((k.layouts >> LAY) & 1) == 0) {
    return nullptr;
  } else if constexpr (k.var == 40 || k.var == 43) {
    return &launch_w4<std::conditional_t<k.var == 40, W4Bf16, W4F8Fwd>, k.ek>;
  } else {
    using OutT = std::conditional_t<k.out == DT_BF16, uint16_t, float>;
    return &launch_cfg<k.bm, k.bn, k.wm, k.wn, (LAY & 2) != 0, (LAY & 1) != 0, OutT, uint16_t, k.var, k.ek>;
  }
}

template <size_t... I>
constexpr std::array<std::array<Launcher, 4>, sizeof...(I)> tiled_launchers(std::index_sequence<I...>) {
  return {{{tiled_launcher<I, 0>(), tiled_launcher<I, 1>(), tiled_launcher<I, 2>(), tiled_launcher<I, 3>()}...}};
}
constexpr auto kTiledLaunchers = tiled_launchers(std::make_index_sequence<kNumTiled>{});

// launch the kernel `choice` names (gemm_choose); a choice with no row launches nothing
hipError_t launch(const GemmLaunch& choice, const GemmArgs& p, hipStream_t s) {
  const int row = find_row(kTiled, choice, p);
  return row < 0 ? hipErrorInvalidValue : kTiledLaunchers[row][layout_index(p)](p, s);
}

// gemm_pair's kernels: the launchers of gemm_dispatch.h's kPair, row by row
template <typename OutT, int VAR, int EK>
hipError_t launch_pair_cfg(const GemmPairArgs& g, int nwg, hipStream_t s) {
  using C = Cfg<256, 256, 2, 4, variant(VAR).ns, variant(VAR).bk>;
  return launch_lds<&gemm_mfma_pair_kernel<256, 256, 2, 4, false, false, OutT, uint16_t, VAR, EK>>(
      g, nwg, C::NT, C::LDS_BYTES, s, {"pair", VAR, 256, 256, EK, g.p[0].split_k > 1 ? g.p[0].split_k : 1});
}

using PairLauncher = hipError_t (*)(const GemmPairArgs&, int, hipStream_t);
template <size_t... I>
constexpr std::array<PairLauncher, sizeof...(I)> pair_launchers(std::index_sequence<I...>) {
  return {{&launch_pair_cfg<std::conditional_t<kPair[I].out == DT_BF16, uint16_t, float>, kPair[I].var, kPair[I].ek>...}};
}
constexpr auto kPairLaunchers = pair_launchers(std::make_index_sequence<kNumPair>{});

#endif  // PZ_GEMM_LAB
}  // namespace

#ifndef PZ_GEMM_LAB
// whole-tile epilogue stores write through (sc1) instead of leaving dirty L2 lines for the kernel
// boundary's write-back (GemmArgs::store_wt); on by default, PZ_GEMM_WT=0 turns it off. r4 A/B,
// mlp4 step: 1.1112 ms off, 1.1081 on; with PZ_OPT_NT on 1.1023 -> 1.0975
int store_wt_default() {
  static const int on = [] {
    const char* e = getenv("PZ_GEMM_WT");
    return e != nullptr ? atoi(e) : 1;
  }();
  return on;
}

hipError_t gemm_pair(const GemmArgs& a, const GemmArgs& b, hipStream_t s) {
  const GemmLaunch choice = gemm_pair_choose(a, b);
  const int split = choice.split, row = find_row(kPair, choice, a);
  if (row < 0 || a.split_k != split || b.split_k != split) return hipErrorInvalidValue;
  if (split > 1 && (a.ws == nullptr || a.counters == nullptr || b.ws == nullptr || b.counters == nullptr))
    return hipErrorInvalidValue;
  GemmPairArgs g;
  g.p[0] = a;
  g.p[1] = b;
  g.p[0].store_wt = g.p[1].store_wt = store_wt_default();
  g.p[0].prio = g.p[1].prio = 1;
  g.nwg0 = tiles(a, 256, 256) * split;
  return kPairLaunchers[row](g, g.nwg0 + tiles(b, 256, 256) * split, s);
}

// launches the tiled kernel gemm_choose picked for `in` (family "mfma" or "w4")
hipError_t gemm_mfma(const GemmArgs& in, const GemmLaunch& choice, hipStream_t s) {
  GemmArgs p = in;
  p.store_wt = store_wt_default();
  p.prio = 1;
  if (p.split_k > 1 && (p.ws == nullptr || p.counters == nullptr)) return hipErrorInvalidValue;
  return launch(choice, p, s);
}
#endif  // PZ_GEMM_LAB

}  // namespace pz
