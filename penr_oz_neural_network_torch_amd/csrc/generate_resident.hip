// pz::generate_resident — a whole generation request in ONE launch, for models small enough to live
// in a workgroup's LDS (engine/resident.py: resident_plan; FusedPredictor.generate_resident).
//
// Grid: `rows` workgroups of 256 threads, one per row. Workgroups never talk to each other (no
// tickets, no global atomics, no global scratch): a row's tokens depend on its context, row0 + row,
// the seed and the scalars only. Everything below lives in the dynamic LDS region, at the 16-byte
// aligned offsets of the plan (no static LDS, so the region's base is aligned too):
//
//   parameters   linear weights [K][N] in the compute dtype (bf16 or fp32), biases, batchnorm gain /
//                bias / running mean / running variance and the embedding table in fp32. A table
//                that does not fit stays in global memory (plan flag): its L rows are read per token.
//   win          the last L ids as a ring: window position l of step s is win[(s + l) % L], the new
//                token overwrites the oldest id. seq is read once, in the prologue.
//   buf0, buf1   activations in the compute dtype, ping-pong; logits: the last stage's fp32 row
//   sampler      sample_core.h's SampleScratch (16.5 KiB); partial: 256 floats of K-split sums
//
// Prologue: copy the parameters, wrap the context ids as embedding_fwd does, and per batchnorm stage
// 1 / sqrt(var + eps) in fp64 (batchnorm.hip's eval formula), once. Then per step s:
//   embedding   buf0[l][e] = T(table[win[(s + l) % L]][e])
//   flatten     nothing moves: [P][W] is [P / r][W * r] in memory
//   linear      out[p][n] = act(sum_k x[p][k] * w[k][n] + bias[n]), fp32 accumulation by fmaf in k
//               order. Thread t owns output o = p * N + n (consecutive threads read consecutive
//               columns of a W row: no bank conflict; x[p][k] is a broadcast). With O = P * N
//               outputs under 256, S = 256 / roundup(O, 64) thread groups each sum a contiguous
//               range of ceil(K / S) k's into `partial`, and thread o folds the S partial sums in
//               group order: the order is a function of (P, K, N) only. No float atomics anywhere.
//               Hidden stages round to the compute dtype; the last one stays fp32 in `logits`.
//   batchnorm   y = T(act(gain * ((x - mean) * invstd) + bias)) in fp64, in place
//   sampling    sample_row<256> on the LDS logits: the code of sample_rows_kernel<256>, with
//               key = layer_key(seed, s) computed here (ops/functional.py: layer_key); thread 0 stores
//               the token to seq[row][L + s] (a plain 8-byte store) and into the ring.
// A row that draws stop_token sets done[row], fills its remaining positions with it and leaves the
// loop; a row that arrives done writes stop_token everywhere. With logits_out, the threads that
// finish the last stage also store each step's logits to logits_out[row][s][:] (steps a finished row
// does not run are left untouched).
//
// Barriers per token: 1 (embedding) + 2 per split linear stage (1 unsplit) + 1 per batchnorm + the
// sampler's (1 greedy, 2 sampling, + 12 with top-k, + 12 with top-p) + 1 after the token.
//
// Each dtype is built twice: <T, false> for requests without top-p / min-p (sample_row's form that
// ignores them: the instructions and registers of the kernel before those options existed) and
// <T, true> for requests with either. The duplication buys the option-free request its old cost: one
// kernel with a run-time branch measured 2.6 % more per token without the options (206 instead of
// 168 VGPRs, the min-p compare in every weight), and a request with them gives up a third of the
// occupancy (2 instead of 3 waves/SIMD) only where it asks for the select.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   <bf16, false>  168 VGPRs, 0 AGPRs, 106 SGPRs (65 spilled to VGPR lanes), scratch 0, static LDS 0, occupancy 3 waves/SIMD
//   <fp32, false>  166 VGPRs, 0 AGPRs, 106 SGPRs (65 spilled to VGPR lanes), scratch 0, static LDS 0, occupancy 3 waves/SIMD
//   <bf16, true>   206 VGPRs, 0 AGPRs, 106 SGPRs (80 spilled to VGPR lanes), scratch 0, static LDS 0, occupancy 2 waves/SIMD
//   <fp32, true>   204 VGPRs, 0 AGPRs, 106 SGPRs (81 spilled to VGPR lanes), scratch 0, static LDS 0, occupancy 2 waves/SIMD
// Dynamic LDS = the plan's total: 28,608 B (bf16) / 36,160 B (fp32) for the character model
// [27, 10, 30, 64, 27], so registers (3 workgroups per CU), not LDS, bound its residency; one
// workgroup per CU once a plan passes 80 KiB.
// Measured on an MI355X (profiles/generate_resident_latency.txt), character model, either dtype: 7.0 us
// per token up to 64 rows, 14.2 us at 1024 rows (T = 0.8); at 1 row 4.0 us greedy, 6.8 us sampling,
// 11.3 us with top-k, plus 6-7 us per launch.
#include "sample_core.h"

namespace pz {
namespace {

constexpr int kNT = 256;

template <typename E>
PZ_DEV void copy_elems(char* dst, const void* src, int numel) {
  const E* __restrict__ s = static_cast<const E*>(src);
  E* d = reinterpret_cast<E*>(dst);
  for (int i = threadIdx.x; i < numel; i += kNT) d[i] = s[i];
}

// kNucleus: the request has top_p < 1 or min_p > 0 (sample_core.h)
template <typename T, bool kNucleus>
__global__ void __launch_bounds__(kNT) generate_resident_kernel(ResidentArgs a) {
  extern __shared__ __attribute__((aligned(16))) char res_smem[];
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const int* __restrict__ pl = a.plan;
  const int L = pl[RH_L], E = pl[RH_E], V = pl[RH_V], vocab = pl[RH_VOCAB];
  const int ns = pl[RH_STAGES], np = pl[RH_PARAMS];
  const int steps = a.steps;
  int64_t* seq = a.seq + static_cast<int64_t>(row) * (L + steps);
  if (a.done[row] != 0) {  // block-uniform
    for (int s = tid; s < steps; s += kNT) seq[L + s] = a.stop_token;
    return;
  }
  const int* par = pl + kResHead;
  const int* stg = par + np * kResParam;

  // ---- prologue: parameters, window, batchnorm inverse deviations
  for (int p = 0; p < np; ++p) {
    const int off = par[p * kResParam + RP_OFF];
    if (off < 0) continue;
    if (par[p * kResParam + RP_ESIZE] == 2)
      copy_elems<uint16_t>(res_smem + off, a.params[p], par[p * kResParam + RP_NUMEL]);
    else
      copy_elems<float>(res_smem + off, a.params[p], par[p * kResParam + RP_NUMEL]);
  }
  int* win = reinterpret_cast<int*>(res_smem + pl[RH_OFF_WIN]);  // [L] ids, then the stop flag
  for (int l = tid; l < L; l += kNT) {
    int64_t id = seq[l];
    id = id < 0 ? id + vocab : id;  // Python indexing, as embedding.hip's wrap_id
    win[l] = id >= 0 && id < vocab ? static_cast<int>(id) : -1;  // (-1: the row reads as zeros)
  }
  __syncthreads();
  for (int st = 0; st < ns; ++st) {
    const int* sg = stg + st * kResStage;
    if (sg[RS_KIND] != 2) continue;
    const float* var = reinterpret_cast<const float*>(res_smem + par[sg[RS_PV] * kResParam + RP_OFF]);
    double* inv = reinterpret_cast<double*>(res_smem + sg[RS_OFF_INV]);
    const double eps = __longlong_as_double(
        (static_cast<long long>(static_cast<uint32_t>(sg[RS_EPS_HI])) << 32) | static_cast<uint32_t>(sg[RS_EPS_LO]));
    for (int c = tid; c < sg[RS_N]; c += kNT) inv[c] = 1.0 / sqrt(static_cast<double>(var[c]) + eps);
  }
  __syncthreads();

  const bool table_lds = pl[RH_TABLE_LDS] != 0;
  const float* table_g = static_cast<const float*>(a.params[0]);
  const float* table_s = reinterpret_cast<const float*>(res_smem + (table_lds ? par[RP_OFF] : 0));
  T* buf0 = reinterpret_cast<T*>(res_smem + pl[RH_OFF_BUF0]);
  T* buf1 = reinterpret_cast<T*>(res_smem + pl[RH_OFF_BUF1]);
  float* logits = reinterpret_cast<float*>(res_smem + pl[RH_OFF_LOGITS]);
  float* partial = reinterpret_cast<float*>(res_smem + pl[RH_OFF_PARTIAL]);
  SampleScratch& sm = *reinterpret_cast<SampleScratch*>(res_smem + pl[RH_OFF_SAMPLER]);
  float* lout = a.logits_out != nullptr ? a.logits_out + static_cast<int64_t>(row) * steps * V : nullptr;

  for (int s = 0; s < steps; ++s) {
    // ---- embedding of the window
    for (int i = tid; i < L * E; i += kNT) {
      const int l = i / E, e = i - l * E;
      const int id = win[(s + l) % L];
      float v = 0.f;
      if (id >= 0) v = table_lds ? table_s[id * E + e] : table_g[static_cast<int64_t>(id) * E + e];
      buf0[i] = from_f<T>(v);
    }
    __syncthreads();

    T* cur = buf0;
    T* nxt = buf1;
    for (int st = 0; st < ns; ++st) {
      const int* sg = stg + st * kResStage;
      const int kind = sg[RS_KIND], P = sg[RS_P], K = sg[RS_K], N = sg[RS_N], act = sg[RS_ACT];
      if (kind == 0) continue;
      if (kind == 1) {
        const bool last = st == ns - 1;
        const T* __restrict__ w = reinterpret_cast<const T*>(res_smem + par[sg[RS_PA] * kResParam + RP_OFF]);
        const float* bias =
            sg[RS_PB] >= 0 ? reinterpret_cast<const float*>(res_smem + par[sg[RS_PB] * kResParam + RP_OFF]) : nullptr;
        const int O = P * N;
        auto finish = [&](int o, int n, float acc) {
          if (bias != nullptr) acc += bias[n];
          acc = act_fwd(acc, act);
          if (last) {
            logits[o] = acc;
            if (lout != nullptr) lout[static_cast<int64_t>(s) * V + o] = acc;
          } else {
            nxt[o] = from_f<T>(acc);
          }
        };
        auto dot = [&](int p, int n, int k0, int k1) {
          const T* x = cur + p * K;
          float acc = 0.f;
#pragma unroll 4
          for (int k = k0; k < k1; ++k) acc = fmaf(to_f<T>(x[k]), to_f<T>(w[k * N + n]), acc);
          return acc;
        };
        if (O >= kNT) {
          for (int o = tid; o < O; o += kNT) {
            const int p = o / N, n = o - p * N;
            finish(o, n, dot(p, n, 0, K));
          }
        } else {
          const int opad = (O + kWave - 1) / kWave * kWave;
          const int S = kNT / opad;  // 4, 2 or 1 groups
          const int kc = (K + S - 1) / S;
          const int g = tid / opad, o = tid - g * opad;
          if (g < S && o < O) {
            const int p = o / N, n = o - p * N;
            partial[g * opad + o] = dot(p, n, min(K, g * kc), min(K, (g + 1) * kc));
          }
          __syncthreads();
          if (tid < O) {
            float acc = partial[tid];
            for (int gg = 1; gg < S; ++gg) acc += partial[gg * opad + tid];
            const int p = tid / N;
            finish(tid, tid - p * N, acc);
          }
        }
        __syncthreads();
        if (!last) {
          T* t = cur;
          cur = nxt;
          nxt = t;
        }
      } else {
        const float* gain = reinterpret_cast<const float*>(res_smem + par[sg[RS_PA] * kResParam + RP_OFF]);
        const float* bias = reinterpret_cast<const float*>(res_smem + par[sg[RS_PB] * kResParam + RP_OFF]);
        const float* mean = reinterpret_cast<const float*>(res_smem + par[sg[RS_PM] * kResParam + RP_OFF]);
        const double* inv = reinterpret_cast<const double*>(res_smem + sg[RS_OFF_INV]);
        for (int i = tid; i < P * N; i += kNT) {
          const int c = i % N;
          const double xh = (static_cast<double>(to_f<T>(cur[i])) - static_cast<double>(mean[c])) * inv[c];
          double v = static_cast<double>(gain[c]) * xh + static_cast<double>(bias[c]);
          v = act_fwd<double>(v, act);
          cur[i] = from_f<T>(static_cast<float>(v));
        }
        __syncthreads();
      }
    }

    // ---- the token
    const uint32_t key = mix32(a.seed_lo ^ mix32(a.seed_hi + 0x9E3779B9u * (static_cast<uint32_t>(s) + 1u)));
    const int token = sample_row<kNT, kNucleus>(logits, V, a.temperature, a.top_k, a.top_p, a.min_p, a.row0 + static_cast<uint32_t>(row), key, sm);
    if (tid == 0) {
      seq[L + s] = token;
      win[s % L] = token;
      const bool stop = static_cast<int64_t>(token) == a.stop_token;
      win[L] = stop ? 1 : 0;
      if (stop) a.done[row] = 1;
    }
    __syncthreads();
    if (win[L] != 0) {  // block-uniform
      for (int j = s + 1 + tid; j < steps; j += kNT) seq[L + j] = a.stop_token;
      break;
    }
  }
}

template <typename T, bool kNucleus>
hipError_t launch(const ResidentArgs& a, hipStream_t s) {
  auto kern = generate_resident_kernel<T, kNucleus>;
  static int attr_bytes = 0;  // the largest dynamic LDS size this kernel was granted
  const int lds = a.plan[RH_TOTAL];
  if (lds > attr_bytes) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    attr_bytes = lds;
  }
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(a.rows)), dim3(kNT), static_cast<size_t>(lds), s, a);
  return hipGetLastError();
}

}  // namespace

int generate_resident_static_lds() {
  hipFuncAttributes fa{};
  size_t most = 0;
  const void* kernels[] = {reinterpret_cast<const void*>(generate_resident_kernel<uint16_t, false>),
                           reinterpret_cast<const void*>(generate_resident_kernel<uint16_t, true>),
                           reinterpret_cast<const void*>(generate_resident_kernel<float, false>),
                           reinterpret_cast<const void*>(generate_resident_kernel<float, true>)};
  for (const void* k : kernels)
    if (hipFuncGetAttributes(&fa, k) == hipSuccess) most = fa.sharedSizeBytes > most ? fa.sharedSizeBytes : most;
  return static_cast<int>(most);
}

hipError_t generate_resident(const ResidentArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.steps < 1 || a.steps > kResMaxSteps || a.plan[RH_MAGIC] != kResMagic) return hipErrorInvalidValue;
  if (a.top_p < 1.f || a.min_p > 0.f) return a.plan[RH_ESIZE] == 2 ? launch<uint16_t, true>(a, s) : launch<float, true>(a, s);
  return a.plan[RH_ESIZE] == 2 ? launch<uint16_t, false>(a, s) : launch<float, false>(a, s);
}

}  // namespace pz
