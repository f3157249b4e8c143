// The static schedule of the persistent stream-K GEMM (gemm_sk.hip): how many workgroups run, which
// tiles are cut along K, and the walk of one workgroup through its work units. Plain integer
// arithmetic with no HIP call: gemm_sk_kernel walks it on the device, the host plans with it, and
// tests/native/gemm_sk_plan.cpp builds it with the host compiler alone and checks every invariant
// the kernel's hand-off relies on.
#pragma once

#if defined(__HIPCC__)
#define PZ_SK_FN __host__ __device__ __forceinline__
#else
#define PZ_SK_FN inline
#endif

namespace pz {

constexpr int kSkTile = 256;  // macro tile BM = BN
constexpr int kSkStep = 64;   // K depth of one schedule step

struct SkSched {
  int nprob;
  int tiles0;           // tiles of problem 0 (problem 1's tiles follow)
  int tiles;            // all tiles
  int iters;            // K steps per tile
  int grid;             // workgroups
  int sk_tiles;         // tiles [0, sk_tiles) are stream-K'd over every workgroup
  long long sk_iters;   // sk_tiles * iters
};

// The schedule of one launch: tiles0 (+ tiles1 of a second problem, 0 = none) tiles of K / 64
// steps on at most `cus` workgroups (0 = every CU) of a device with `device_cus` CUs.
// At most TWO contributors per tile. Fewer tiles than workgroups: each tile in two K halves on
// 2T workgroups when the budget holds them and the halves are >= 256 deep, else one workgroup
// per tile (data-parallel; the other CUs idle but the survivors run faster per step). At least
// as many tiles: the "two-tile" region gives every workgroup >= one tile of K steps, so a tile
// meets at most two workgroups' ranges.
PZ_SK_FN SkSched sk_plan(int tiles0, int tiles1, int K, int cus, int device_cus) {
  SkSched s{};
  s.nprob = tiles1 > 0 ? 2 : 1;
  s.tiles0 = tiles0;
  s.tiles = tiles0 + tiles1;
  s.iters = K / kSkStep;
  int grid = cus > 0 && cus < device_cus ? cus : device_cus;
  const int T = s.tiles;
  if (T < grid) grid = (2 * T <= grid && s.iters * kSkStep >= 512) ? 2 * T : T;
  int sk = 0;
  if (T % grid != 0) sk = T < grid ? T : T % grid + grid;
  s.grid = grid;
  s.sk_tiles = sk;
  s.sk_iters = static_cast<long long>(sk) * s.iters;
  return s;
}

// first stream-K iteration of workgroup w (w = grid: the end)
PZ_SK_FN long long sk_start(const SkSched& s, int w) { return static_cast<long long>(w) * s.sk_iters / s.grid; }

// the workgroup whose stream-K range holds iteration `it`
PZ_SK_FN int sk_owner(const SkSched& s, long long it) {
  int w = static_cast<int>(it * s.grid / s.sk_iters);
  while (w + 1 < s.grid && sk_start(s, w + 1) <= it) ++w;
  while (w > 0 && sk_start(s, w) > it) --w;
  return w;
}

// ---- the walk of workgroup w: the stream-K range [s0, s1) cut at tile boundaries, then the
// data-parallel tiles sk_tiles + w, + grid, ...
struct SkWalk {
  long long s0, s1;  // this workgroup's stream-K iterations
  long long it;      // the next one
  int dp_t;          // the next data-parallel tile
};

// K steps [kb, ke) of tile t; slab >= 0: a stream-K partial tile, handed over through that slab
// (slab 2w = the workgroup's first unit, 2w + 1 any later one: a range holds at most two partials)
struct SkUnit {
  int t, kb, ke, slab;
};

PZ_SK_FN SkWalk sk_walk(const SkSched& s, int w) {
  SkWalk k;
  k.s0 = s.sk_iters > 0 ? sk_start(s, w) : 0;
  k.s1 = s.sk_iters > 0 ? sk_start(s, w + 1) : 0;
  k.it = k.s0;
  k.dp_t = s.sk_tiles + w;
  return k;
}

// the next unit of workgroup w; t < 0: the walk is over
PZ_SK_FN SkUnit sk_next(const SkSched& s, int w, SkWalk& k) {
  SkUnit u;
  if (k.it < k.s1) {
    u.t = static_cast<int>(k.it / s.iters);
    u.kb = static_cast<int>(k.it - static_cast<long long>(u.t) * s.iters);
    const long long left = k.s1 - k.it;
    u.ke = left < static_cast<long long>(s.iters - u.kb) ? u.kb + static_cast<int>(left) : s.iters;
    u.slab = (u.kb == 0 && u.ke == s.iters) ? -1 : 2 * w + (k.it == k.s0 ? 0 : 1);
    k.it += u.ke - u.kb;
  } else if (k.dp_t < s.tiles) {
    u.t = k.dp_t;
    u.kb = 0;
    u.ke = s.iters;
    u.slab = -1;
    k.dp_t += s.grid;
  } else {
    u.t = u.kb = u.ke = u.slab = -1;
  }
  return u;
}

// the first stream-K iteration of tile t
PZ_SK_FN long long sk_tile_start(const SkSched& s, int t) { return static_cast<long long>(t) * s.iters; }

// the first and the last workgroup whose ranges meet the stream-K tile that starts at iteration t0
// (sk_tile_start): its contributors (two, or one where wlo == whi), so its ticket counts to whi - wlo
struct SkPair {
  int wlo, whi;
};
PZ_SK_FN SkPair sk_contributors(const SkSched& s, long long t0) {
  return {sk_owner(s, t0), sk_owner(s, t0 + s.iters - 1)};
}

// the slab contributor c wrote its part of the tile that starts at t0 into: its second one when its
// range starts before the tile does (the tile is not its first unit)
PZ_SK_FN int sk_slab_of(const SkSched& s, int c, long long t0) { return 2 * c + (sk_start(s, c) < t0 ? 1 : 0); }

}  // namespace pz
