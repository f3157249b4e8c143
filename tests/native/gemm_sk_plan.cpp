// The stream-K schedule (csrc/gemm_sk_plan.h) as a host program: every workgroup of every schedule
// of a sweep is walked with the header's own functions, the ones gemm_sk_kernel calls, and the
// invariants its slab / ticket hand-off relies on are checked. Driven by
// tests/test_gemm_sk_plan_cpu.py under AddressSanitizer + UBSan; no GPU, no HIP call.
//
//   gemm_sk_plan sweep      the sweep; one line per regime class and per workgroup unit pattern
//                           reached ("regime NAME COUNT", "units PATTERN COUNT"), then "ok N"
//   gemm_sk_plan describe   stdin lines "tiles0 tiles1 K cus device_cus"; per line
//                           "grid sk_tiles iters tiles regime | w0's units | w1's units ..." with
//                           a unit as tile:kb-ke (whole tiles) or tile:kb-ke@slab (partial ones)
//
// A unit pattern is the sequence of a workgroup's units, W a whole tile and P a partial one; a run
// of two or more W is written Wn.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "gemm_sk_plan.h"

namespace {

struct Part {
  int w, kb, ke, slab;
};

struct Checked {
  bool ok = true;
  std::string regime;
  std::vector<std::string> patterns;               // per workgroup
  std::vector<std::vector<pz::SkUnit>> units;      // per workgroup (describe only)
};

// one tile's contributors in the order they were walked (a third one is an error)
struct Parts {
  int n;
  Part p[2];
};

int failures = 0;

void fail(const pz::SkSched& s, int cus, int dev, const char* what, long long a = 0, long long b = 0) {
  if (++failures <= 10)
    std::fprintf(stderr, "FAIL tiles0=%d tiles=%d iters=%d cus=%d dev=%d grid=%d sk_tiles=%d: %s (%lld, %lld)\n", s.tiles0,
                 s.tiles, s.iters, cus, dev, s.grid, s.sk_tiles, what, a, b);
}

// appends one unit to a workgroup's pattern; `run` = whole tiles at its end so far
void pattern_add(std::string& pat, int& run, bool whole) {
  if (!whole) {
    pat += 'P';
    run = 0;
  } else if (++run == 1) {
    pat += 'W';
  } else if (run == 2) {
    pat += 'n';
  }
}

const char* regime_of(const pz::SkSched& s) {
  const int rounds = (s.tiles + s.grid - 1) / s.grid;
  if (s.sk_tiles == 0) return rounds <= 1 ? "dp_one_round" : "dp_rounds";
  if (s.tiles < s.grid) {
    if (s.grid != 2 * s.tiles) return "other";
    return s.iters % 2 == 0 ? "halves_even" : "halves_odd";
  }
  return s.sk_tiles == s.tiles ? "twotile" : "twotile_dp";
}

Checked check(const pz::SkSched& s, int cus, int dev, bool keep_units) {
  Checked r;
#define REQUIRE(cond, what, a, b)                 \
  do {                                            \
    if (!(cond)) {                                \
      fail(s, cus, dev, what, (a), (b));          \
      r.ok = false;                               \
      return r;                                   \
    }                                             \
  } while (0)
  const int budget = cus > 0 && cus < dev ? cus : dev;
  REQUIRE(s.grid >= 1 && s.grid <= budget, "grid <= min(cus, device)", s.grid, budget);
  REQUIRE(s.tiles >= 1 && s.iters >= 2, "a schedule has tiles and at least two steps", s.tiles, s.iters);
  REQUIRE(s.sk_tiles >= 0 && s.sk_tiles <= s.tiles, "sk_tiles within the tiles", s.sk_tiles, s.tiles);
  REQUIRE(s.sk_iters == static_cast<long long>(s.sk_tiles) * s.iters, "sk_iters = sk_tiles * iters", s.sk_iters, 0);
  REQUIRE((s.tiles - s.sk_tiles) % s.grid == 0 || s.sk_tiles == 0, "data-parallel tiles fill whole rounds",
          s.tiles - s.sk_tiles, s.grid);
  if (s.sk_tiles > 0) {
    REQUIRE(pz::sk_start(s, 0) == 0 && pz::sk_start(s, s.grid) == s.sk_iters, "the ranges span the stream-K region", 0, 0);
  }
  r.regime = regime_of(s);
  REQUIRE(r.regime != "other", "a schedule outside the six regimes", 0, 0);

  static std::vector<Parts> parts;
  static std::vector<char> slab_used;
  parts.assign(s.tiles, Parts{});
  slab_used.assign(2 * static_cast<size_t>(s.grid), 0);
  if (keep_units) r.units.resize(s.grid);
  r.patterns.reserve(s.grid);
  for (int w = 0; w < s.grid; ++w) {
    pz::SkWalk walk = pz::sk_walk(s, w);
    int dp_seen = 0, walked = 0, run = 0;
    bool dp_phase = false;
    std::string pat;
    for (;;) {
      const pz::SkUnit u = pz::sk_next(s, w, walk);
      if (u.t < 0) break;
      REQUIRE(++walked <= s.tiles + 2, "the walk ends", w, 0);
      REQUIRE(u.t >= 0 && u.t < s.tiles, "unit inside the tiles", w, u.t);
      REQUIRE(u.kb >= 0 && u.kb < u.ke && u.ke <= s.iters, "unit inside one tile", u.kb, u.ke);
      const bool whole = u.kb == 0 && u.ke == s.iters;
      REQUIRE((u.slab >= 0) == !whole, "slab >= 0 exactly for partial units", u.t, u.slab);
      if (!whole) {
        REQUIRE(u.t < s.sk_tiles, "partial units lie in the ticketed range t < sk_tiles", u.t, s.sk_tiles);
        REQUIRE(u.slab < 2 * s.grid, "slab < 2 * grid", u.slab, s.grid);
        REQUIRE(u.slab == 2 * w || u.slab == 2 * w + 1, "a workgroup writes its own two slabs", u.slab, w);
        REQUIRE(!slab_used[u.slab], "slab indices of a launch are distinct", u.slab, w);
        REQUIRE(!dp_phase, "no partial unit after a data-parallel tile", w, u.t);
        slab_used[u.slab] = 1;
      }
      if (u.t >= s.sk_tiles) {
        dp_phase = true;
        REQUIRE(u.t == s.sk_tiles + w + dp_seen * s.grid, "data-parallel tiles w, w + grid, ... in order", u.t, w);
        ++dp_seen;
      }
      Parts& ps = parts[u.t];
      REQUIRE(ps.n < 2, "a tile has at most two contributors", u.t, w);
      ps.p[ps.n++] = {w, u.kb, u.ke, u.slab};
      pattern_add(pat, run, whole);
      if (keep_units) r.units[w].push_back(u);
    }
    r.patterns.push_back(pat.empty() ? "-" : pat);
  }

  for (int t = 0; t < s.tiles; ++t) {
    const int np = parts[t].n;
    REQUIRE(np >= 1, "every tile is visited", t, 0);
    // walked in workgroup order, and a lower workgroup holds the earlier steps
    const Part &first = parts[t].p[0], &last = parts[t].p[np - 1];
    REQUIRE(first.kb == 0 && last.ke == s.iters, "a tile's steps are covered from 0 to iters", t, 0);
    if (np == 2) {
      REQUIRE(first.ke == last.kb, "every (tile, step) is covered exactly once", first.ke, last.kb);
      REQUIRE(first.w < last.w, "two contributors are two workgroups", first.w, last.w);
    }
    if (t >= s.sk_tiles) {
      REQUIRE(np == 1, "a data-parallel tile is visited once", t, 0);
      continue;
    }
    const long long t0 = pz::sk_tile_start(s, t);
    REQUIRE(t0 == static_cast<long long>(t) * s.iters, "a tile starts at iteration t * iters", t, t0);
    const pz::SkPair who = pz::sk_contributors(s, t0);
    REQUIRE(pz::sk_owner(s, t0) == first.w, "sk_owner agrees with the walk at a tile's first step", t, first.w);
    REQUIRE(pz::sk_owner(s, t0 + s.iters - 1) == last.w, "sk_owner agrees with the walk at a tile's last step", t, last.w);
    REQUIRE(who.wlo == first.w && who.whi == last.w, "sk_contributors names the walkers", who.wlo, who.whi);
    // the ticket of tile t counts to whi - wlo: as many arrivals as contributors
    REQUIRE(who.whi - who.wlo + 1 == np, "a tile has exactly whi - wlo + 1 contributors", t, who.whi - who.wlo);
    if (np == 2) {
      for (const Part& p : parts[t].p)
        REQUIRE(pz::sk_slab_of(s, p.w, t0) == p.slab, "the slab rule names the slab the contributor wrote", p.w, p.slab);
    }
  }
#undef REQUIRE
  return r;
}

int sweep() {
  const int kSteps[] = {2, 3, 5, 8, 9, 16, 64};
  const int kBudgets[] = {0, 1, 2, 3, 4, 5, 7, 12, 37, 100, 200, 240, 255, 256, 300};
  const int kDevices[] = {256, 304};
  const int kPairTiles[] = {1, 2, 3, 4, 5, 7, 8, 12, 30, 37, 64, 100, 255, 256, 300};
  std::map<std::string, long long> regimes, patterns;
  long long n = 0;
  auto one = [&](int tiles0, int tiles1, int steps, int cus, int dev) {
    const pz::SkSched s = pz::sk_plan(tiles0, tiles1, steps * pz::kSkStep, cus, dev);
    if (s.nprob != (tiles1 > 0 ? 2 : 1) || s.tiles0 != tiles0 || s.tiles != tiles0 + tiles1 || s.iters != steps) {
      fail(s, cus, dev, "sk_plan states the problem it was given");
      return;
    }
    const Checked r = check(s, cus, dev, false);
    ++n;
    if (!r.ok) return;
    ++regimes[r.regime];
    for (const std::string& p : r.patterns) ++patterns[p];
  };
  for (int dev : kDevices)
    for (int cus : kBudgets)
      for (int steps : kSteps) {
        for (int T = 1; T <= 600; ++T) one(T, 0, steps, cus, dev);
        for (int t0 : kPairTiles)
          for (int t1 : kPairTiles) one(t0, t1, steps, cus, dev);
      }
  for (const auto& [name, count] : regimes) std::printf("regime %s %lld\n", name.c_str(), count);
  for (const auto& [name, count] : patterns) std::printf("units %s %lld\n", name.c_str(), count);
  if (failures > 0) {
    std::fprintf(stderr, "%d of %lld schedules failed\n", failures, n);
    return 1;
  }
  std::printf("ok %lld\n", n);
  return 0;
}

int describe() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    int tiles0, tiles1, K, cus, dev;
    if (!(in >> tiles0 >> tiles1 >> K >> cus >> dev) || tiles0 < 1 || tiles1 < 0 || K < 2 * pz::kSkStep || dev < 1) {
      std::fprintf(stderr, "bad schedule line: %s\n", line.c_str());
      return 2;
    }
    const pz::SkSched s = pz::sk_plan(tiles0, tiles1, K, cus, dev);
    const Checked r = check(s, cus, dev, true);
    if (!r.ok) return 1;
    std::printf("%d %d %d %d %s", s.grid, s.sk_tiles, s.iters, s.tiles, r.regime.c_str());
    for (const auto& us : r.units) {
      std::printf(" |");
      for (const pz::SkUnit& u : us) {
        if (u.slab >= 0) std::printf(" %d:%d-%d@%d", u.t, u.kb, u.ke, u.slab);
        else std::printf(" %d:%d-%d", u.t, u.kb, u.ke);
      }
    }
    std::printf("\n");
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) return sweep();
  if (argc == 2 && std::strcmp(argv[1], "describe") == 0) return describe();
  std::fprintf(stderr, "usage: gemm_sk_plan sweep | describe\n");
  return 2;
}
