"""The stream-K schedule (csrc/gemm_sk_plan.h: sk_plan, sk_start, sk_owner, the unit walk sk_walk / sk_next,
sk_contributors, sk_slab_of) checked without a GPU.

``tests/native/gemm_sk_plan.cpp`` is built as a plain host program with ``-fsanitize=address,undefined``.
It includes the header gemm_sk_kernel itself calls, so what it walks is the kernel's walk, not a
restatement. Its sweep plans one-problem schedules of 1 to 600 tiles and two-problem schedules over a grid
of tile counts, each at 7 step counts, 15 CU budgets and device CU counts 256 and 304, walks every
workgroup and checks what the kernel's slab / ticket hand-off relies on: every (tile, K step) covered
exactly once by units that lie inside one tile; at most two contributors per tile and exactly
whi - wlo + 1 of them (the ticket's count); slab >= 0 exactly for partial units; distinct slab indices
below 2 grid; the slab rule naming the slab each contributor wrote; sk_owner agreeing with the walk at
the first and last step of every stream-K tile; partial units only at tiles below sk_tiles (the
tickets); grid <= min(cus, device); data-parallel tiles visited once each, in order.

The sweep must reach every regime class and workgroup unit pattern named below, and the schedules the
GPU tests launch (tests/test_gemm_sk_exact_gpu.py: SCHEDULES, PAIRS, imported here) must plan as those
tests assert on a 256-CU device and hold the unit patterns they are there for.
"""
import os
import re
import shutil
import subprocess

import pytest

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import test_gemm_sk_exact_gpu as SKX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "penr_oz_neural_network_torch_amd", "csrc")
REGIMES = {"dp_one_round", "dp_rounds", "halves_even", "halves_odd", "twotile", "twotile_dp"}
# W a whole tile, P a partial one, Wn two or more whole tiles in a row
PATTERNS = {"W", "Wn", "P", "PW", "WP", "PP", "PWP", "PWn", "PPW", "PPWn", "WPW", "WPWn", "PWPW", "PWPWn"}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("sk_plan") / "gemm_sk_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "native", "gemm_sk_plan.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime unavailable: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr

    def run(mode, lines=()):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([out, mode], input="".join(line + "\n" for line in lines), capture_output=True, text=True,
                           env=env, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        assert "runtime error:" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        return r.stdout.splitlines()
    return run


def test_every_schedule_of_the_sweep_keeps_the_hand_off_invariants(planner):
    out = planner("sweep")
    print("\n".join(out))
    assert out[-1].startswith("ok ") and int(out[-1].split()[1]) > 100000
    reached = {kind: {ln.split()[1] for ln in out if ln.startswith(kind + " ")} for kind in ("regime", "units")}
    assert reached["regime"] == REGIMES
    assert PATTERNS <= reached["units"], PATTERNS - reached["units"]
    # a range is shorter than two tiles: no workgroup has two whole tiles between partial ones
    assert not any("PWnP" in p for p in reached["units"])


def describe(planner, lines):
    """Per line: (grid, sk_tiles, iters, tiles), the regime class and each workgroup's units."""
    out = []
    for ln in planner("describe", lines):
        head, *wgs = ln.split(" |")
        grid, sk_tiles, iters, tiles, regime = head.split()
        out.append(((int(grid), int(sk_tiles), int(iters), int(tiles)), regime, [w.split() for w in wgs]))
    return out


def pattern(units):
    return re.sub("W{2,}", "Wn", "".join("P" if "@" in u else "W" for u in units))


def tile(unit):
    return int(unit.split(":")[0])


def steps(unit):
    kb, ke = unit.split(":")[1].split("@")[0].split("-")
    return int(ke) - int(kb)


def test_the_gpu_tests_schedules_are_the_ones_they_name(planner):
    names = list(SKX.SCHEDULES)
    lines = []
    for n in names:
        (M, N, K), cus, _ = SKX.SCHEDULES[n]
        lines.append(f"{(M // 256) * (N // 256)} 0 {K} {cus} 256")
    for n, (plan, regime, wgs) in zip(names, describe(planner, lines)):
        (M, N, K), cus, want = SKX.SCHEDULES[n]
        print(n, plan, regime, wgs)
        assert plan == (*want, K // 64, (M // 256) * (N // 256)), n
        want_regime, want_patterns = SKX.REACHES[n]
        assert regime == want_regime, n
        assert want_patterns <= {pattern(w) for w in wgs}, n
    by_name = dict(zip(names, describe(planner, lines)))

    def partial(n):
        return [u for w in by_name[n][2] for u in w if "@" in u]

    # uneven cuts, the 4 + 5 step halves, one-step partials (at K = 128: nothing but)
    assert {steps(u) for u in partial("twotile")} == {2, 3}
    assert [steps(u) for u in partial("halves_odd")] == [4, 5] * 6
    assert 1 in {steps(u) for u in partial("twotile_pp")}
    assert {steps(u) for u in partial("twotile_k128")} == {1}
    # six tiles on one workgroup; one and two data-parallel tiles per workgroup behind a stream-K region
    assert [len(w) for w in by_name["serial"][2]] == [6]
    assert all(sum(tile(u) >= 5 for u in w) == 1 for w in by_name["sk_dp"][2])
    assert all(sum(tile(u) >= 5 for u in w) == 2 for w in by_name["sk_dp2"][2])


def test_the_binding_reports_the_plan_without_launching():
    """PF.gemm_sk_plan needs no GPU (without one the engine plans for 256 CUs): the GPU tests' plans, and
    arguments the engine cannot schedule are refused."""
    for n, ((M, N, K), cus, want) in SKX.SCHEDULES.items():
        assert PF.gemm_sk_plan(M, N, K, cus) == (*want, K // 64, (M // 256) * (N // 256)), n
    for s0, s1, K, cus, want in SKX.PAIRS.values():
        assert PF.gemm_sk_plan(*s0, K, cus, *s1) == PF.gemm_sk_plan(*s1, K, cus, *s0) == (*want, K // 64, 7)
    for bad in ((768, 500, 320, 4), (768, 512, 96, 4), (768, 512, 64, 4), (0, 512, 320, 4), (768, 512, 320, -1),
                (768, 512, 320, 4, 256, 0), (768, 512, 320, 4, 256, 100)):
        with pytest.raises(RuntimeError, match="gemm_sk_plan"):
            PF.gemm_sk_plan(*bad)


def test_the_gpu_tests_pairs_cut_a_tile_of_each_problem(planner):
    for name, (s0, s1, K, cus, want) in SKX.PAIRS.items():
        for a, b in ((s0, s1), (s1, s0)):
            t0, t1 = (a[0] // 256) * (a[1] // 256), (b[0] // 256) * (b[1] // 256)
            (plan, regime, wgs), = describe(planner, [f"{t0} {t1} {K} {cus} 256"])
            print(name, a, b, plan, regime, wgs)
            assert plan == (*want, K // 64, 7)
            cut = {tile(u) for w in wgs for u in w if "@" in u}
            whole_dp = {tile(u) for w in wgs for u in w if tile(u) >= plan[1]}
            if name == "boundary_in_sk_region":
                # tiles of both problems are cut, among them one next to the boundary between the problems
                assert regime == "twotile" and min(cut) < t0 <= max(cut) and ({t0 - 1, t0} & cut)
            else:
                assert regime == "twotile_dp" and whole_dp and min(whole_dp) >= t0   # the second problem's tiles
