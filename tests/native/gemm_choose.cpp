// The GEMM dispatch decision (csrc/gemm_dispatch.h) as a host program: one case per line on stdin,
// the kernel gemm_choose / gemm_pair_choose picks per line on stdout, in gemm_last_kernel()'s
// format, followed for the tiled families by whether the choice has a row in the kernel table.
// Driven by tests/test_gemm_choose_cpu.py under AddressSanitizer + UBSan; no GPU, no HIP call.
//
// A line holds these integers (dtypes as pz::DType, epi_mode as pz::EpiMode, act as pz::Act):
//   pair M N K a_kc b_kc in out aux a_fmt b_fmt epi_mode act drop_pre drop_post drop_all accumulate
//   bias colsum mask auxp out8 no_split force_generic engine cus w4 sk M1 N1
// pair = 1: gemm_pair of (M, N, K) and (M1, N1, K); bias .. out8 say whether that pointer is set.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "gemm_dispatch.h"

namespace {

// non-null, 16-byte aligned, never dereferenced
template <typename T>
T* fake(int n) { return reinterpret_cast<T*>(static_cast<uintptr_t>(0x10000) * (n + 1)); }

// the fields of a line, in order
enum Field {
  F_pair, F_M, F_N, F_K, F_a_kc, F_b_kc, F_in, F_out, F_aux, F_a_fmt, F_b_fmt, F_epi_mode, F_act, F_drop_pre, F_drop_post,
  F_drop_all, F_accumulate, F_bias, F_colsum, F_mask, F_auxp, F_out8, F_no_split, F_force_generic, F_engine, F_cus,
  F_w4, F_sk, F_M1, F_N1, F_COUNT
};
struct Case {
  int v[F_COUNT];
  int operator[](Field f) const { return v[f]; }
};

// contiguous operands, as the binding fills GemmArgs from contiguous tensors
pz::GemmArgs args_of(const Case& c, int M, int N) {
  pz::GemmArgs p{};
  p.A = fake<void>(0);
  p.B = fake<void>(1);
  p.C = fake<void>(2);
  p.M = M;
  p.N = N;
  p.K = c[F_K];
  p.a_kc = c[F_a_kc];
  p.b_kc = c[F_b_kc];
  p.lda = c[F_a_kc] ? c[F_K] : M;
  p.ldb = c[F_b_kc] ? c[F_K] : N;
  p.ldc = N;
  p.in_dtype = c[F_in];
  p.out_dtype = c[F_out];
  p.a_fmt = c[F_a_fmt];
  p.b_fmt = c[F_b_fmt];
  p.alpha = 1.f;
  p.accumulate = c[F_accumulate];
  p.epi_mode = c[F_epi_mode];
  p.epi.act = c[F_act];
  p.epi.drop_pre = c[F_drop_pre];
  p.epi.drop_post = c[F_drop_post];
  p.epi.drop_all = c[F_drop_all];
  p.idx_ld = N;
  p.force_generic = c[F_force_generic];
  p.engine = c[F_engine];
  p.cus = c[F_cus];
  if (c[F_bias]) p.bias = fake<const float>(3);
  if (c[F_colsum]) p.colsum = fake<float>(4);
  if (c[F_auxp]) {
    p.aux = fake<void>(5);
    p.ldaux = N;
    p.aux_dtype = c[F_aux];
  }
  if (c[F_mask]) {
    p.mask = fake<uint8_t>(6);
    p.ldmask = 32 * ((N + 255) / 256);
  }
  if (c[F_out8]) {
    p.out8 = fake<uint8_t>(7);
    p.ldout8 = N;
    p.out8_fmt = c[F_epi_mode] == pz::EPI_BWD ? 1 : 0;
    p.out8_qscale = fake<const float>(8);
  }
  if (c[F_epi_mode] == pz::EPI_OPT) p.opt.params = fake<float>(9);  // SGD: no moments, no shadow
  return p;
}

std::string name_of(const pz::GemmLaunch& g) {
  return std::string(g.family) + "/var" + std::to_string(g.var) + "/" + std::to_string(g.bm) + "x" +
         std::to_string(g.bn) + "/ek" + std::to_string(g.ek) + "/split" + std::to_string(g.split);
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    Case c{};
    for (int& field : c.v)
      if (!(in >> field)) {
        std::fprintf(stderr, "bad case line: %s\n", line.c_str());
        return 2;
      }
    pz::GemmArgs a = args_of(c, c[F_M], c[F_N]);
    if (c[F_pair]) {
      pz::GemmArgs b = args_of(c, c[F_M1], c[F_N1]);
      a.split_k = b.split_k = pz::gemm_pair_split(a, b);
      const pz::GemmLaunch g = pz::gemm_pair_choose(a, b);
      std::printf("%s %s\n", name_of(g).c_str(), pz::find_row(pz::kPair, g, a) >= 0 ? "row" : "norow");
      continue;
    }
    if (!c[F_no_split]) {  // the binding's plan
      const int split = pz::gemm_split(a);
      if (split > 1) a.split_k = split;
    }
    const pz::GemmLaunch g = pz::gemm_choose(a, pz::GemmKnobs{c[F_w4] != 0, c[F_sk] != 0});
    if (pz::family_is(g, "mfma") || pz::family_is(g, "w4"))
      std::printf("%s %s\n", name_of(g).c_str(), pz::find_row(pz::kTiled, g, a) >= 0 ? "row" : "norow");
    else
      std::printf("%s\n", name_of(g).c_str());
  }
  return 0;
}
