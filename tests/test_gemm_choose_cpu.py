"""The GEMM dispatch decision (csrc/gemm_dispatch.h: gemm_choose, gemm_pair_choose, the kTiled kernel table)
checked without a GPU.

``tests/native/gemm_choose.cpp`` is built as a plain host program with ``-fsanitize=address,undefined``
and run once on every case below: GemmArgs of the shape, layout, types, epilogue and flags that the GPU
tests' run_case / run_pair / launch_update hand to the binding (contiguous operands), the split planned
as the binding plans it. The kernel it names must be the one the GPU test modules predict with their own
restatements of the dispatch (``expected_kernel``, ``PAIR_KERNEL``, ``UPDATE_KERNEL``, ``sk_kernel``: imported
here, not copied), i.e. the one they assert through ``gemm_last_kernel()`` on the device, and every tiled, w4
and pair choice must have a row in the table the launchers are built from.

The stream-K engine's table (kSk): every form of FORMS in each of the four operand layouts, asked for
by engine 2, by engine 0 with PZ_GEMM_SK and by engine 0 with a CU budget, is chosen for the engine
exactly where test_gemm_sk_exact_gpu.SK_TABLE (the restatement its form list comes from) has the
(layout, kind) pair, and is a tiled or generic kernel everywhere else.
"""
import os
import shutil
import subprocess

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import test_gemm_exact_gpu as EX
from tests import test_gemm_fp8_exact_gpu as F8
from tests import test_gemm_pair_update_gpu as PU
from tests import test_gemm_sk_exact_gpu as SKX
from tests.helpers import PAIR_SPLIT_CASES, gemm_pair_split_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "penr_oz_neural_network_torch_amd", "csrc")
DT = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2, torch.float8_e4m3fn: 3, torch.float8_e5m2: 3}


def params_of(test_fn):
    """The argument tuples of a test function's (single) parametrize mark."""
    (mark,) = [m for m in test_fn.pytestmark if m.name == "parametrize"]
    return list(mark.args[1])


def gemm_line(shape, form, p=0.5, *, layout=None, fmts=None, in_dtype=torch.bfloat16, out_dtype=None, no_split=False,
              force_generic=False, engine=1, cus=0, w4=1, sk=0, mode=None):
    """One input line of the program: what EX.run_case passes to PF.gemm for (shape, form, p)."""
    f = EX.FORMS[form]
    M, N, K = shape
    a_kc, b_kc = EX.LAYOUTS[layout or f.layout]
    mode = f.mode if mode is None else mode
    drops = mode != PF.EPI_STORE and p > 0.0   # PF.epi_spec; EPI_STORE runs with NO_EPI
    bwd = mode == PF.EPI_BWD
    out = out_dtype or f.out
    mask = f.mask and in_dtype == torch.bfloat16 and not force_generic
    fields = [0, M, N, K, a_kc, b_kc, DT[in_dtype if fmts is None else fmts[0]], DT[out], DT[out],
              0 if fmts is None else int(fmts[0] == torch.float8_e5m2), 0 if fmts is None else int(fmts[1] == torch.float8_e5m2),
              mode, f.act if mode != PF.EPI_STORE else PF.ACT_NONE, drops and f.pre, drops and f.post, drops and p >= 1.0,
              f.accumulate, f.bias, f.colsum, mask, bwd and not f.mask, f.out8, no_split, force_generic, engine, cus,
              w4, sk, 0, 0]
    return " ".join(str(int(v)) for v in fields)


def pair_line(s0, s1, K, kind):
    fp8 = kind == "fp8"
    fields = [1, s0[0], s0[1], K, 0, 0, 3 if fp8 else 0, 1 if kind == "f32" else 0, 0, 0, int(fp8)] + [0] * 17 + [s1[0], s1[1]]
    return " ".join(str(int(v)) for v in fields)


def update_line(shape):
    """PU.launch_update: the dW layout, bf16 operands, an fp32 gradient view, EPI_OPT."""
    return gemm_line(shape, "dw_f32", engine=0, mode=3)


def cases():
    """(input line, expected kernel name) of every case."""
    out = []
    # bf16 operands on the tiled kernels and w4: every (class, form, no_split) the GPU file expects a name for
    bf16 = {(c, f, False) for c, f in EX.TABLE}
    bf16 |= {(c, f, False) for c, f in params_of(EX.test_store_c_false_writes_only_the_side_outputs)}
    bf16 |= {("Ssplit", f, True) for f in params_of(EX.test_no_split_runs_the_skinny_shape_as_128_tiles)}
    bf16 |= {(c, f, False) for c in ("S128", "S256") for f in ("relu_prepost_out8", "dx_relu_mask_out8", "dx_relu_aux",
                                                               "relu_prepost")}
    for cls, form, no_split in sorted(bf16):
        for p in EX.FORMS[form].p:
            out.append((gemm_line(EX.SHAPES[cls], form, p, no_split=no_split), EX.expected_kernel(cls, form, no_split)))
    # fp8 operands: every (cell, shape, form, no_split) of the fp8 file
    fp8 = {(*t, False) for t in F8.TABLE}
    fp8 |= {(c, s, f, False) for c, s, f, _ in params_of(F8.test_fp8_copy_saturates_and_reaches_subnormal_codes)}
    fp8 |= {(*t, False) for t in params_of(F8.test_fp8_store_c_false_writes_only_the_side_outputs)}
    fp8 |= {(*t, True) for t in params_of(F8.test_fp8_no_split_runs_one_pass)}
    fp8 |= {(*t, False) for t in params_of(F8.test_fp8_strided_views_write_nothing_outside_the_slice)}
    for cell, shape, form, no_split in sorted(fp8, key=str):
        layout, fmts = F8.CELLS[cell]
        for p in EX.FORMS[form].p:
            out.append((gemm_line(shape, form, p, layout=layout, fmts=fmts, no_split=no_split),
                        F8.expected_kernel(cell, shape, form, no_split)))
    # gemm_pair and gemm_update
    for s0, s1, K, split in PAIR_SPLIT_CASES:
        assert gemm_pair_split_plan(s0, s1, K) == split
        for kind in ("bf16", "f32", "fp8"):
            for a, b in ((s0, s1), (s1, s0)):
                out.append((pair_line(a, b, K, kind), f"{PU.PAIR_KERNEL[kind]}/split{split} row"))
    for shape, name in PU.UPDATE_KERNEL.items():
        out.append((update_line(shape), f"{name}/split{PU.UPDATE_SPLIT[shape]}"))
    # the other families
    for in_dtype, kw in ((torch.bfloat16, {}), (torch.float32, dict(out_dtype=torch.float32))):
        out.append((gemm_line(EX.GENERIC, "plain", in_dtype=in_dtype, force_generic=True, **kw), "generic/var0/64x64/ek0/split1"))
    for layout in ("fwd", "dw", "dx"):   # test_gemm_wide_gpu.py::test_gemm_fp32_matrix_cores
        out.append((gemm_line((640, 320, 1024), "plain", layout=layout, in_dtype=torch.float32, out_dtype=torch.float32,
                              engine=0), "wide/var0/128x128/ek0/split1"))
    for form in SKX.SK_FORMS:
        assert form not in EX.SK_KIND or SKX.sk_kernel(form) == f"sk/var0/256x256/ek{EX.SK_KIND[form]}/split1"
        for p in EX.FORMS[form].p:
            for cus in (37, 200):
                out.append((gemm_line(EX.SK, form, p, engine=2, cus=cus), SKX.sk_kernel(form)))
    return out


def sk_table_cases():
    """(input line, the stream-K kernel's name or None) of every form in every layout, and of the pairs
    outside the table at a second shape, each asked for in the three ways that reach the engine."""
    pairs = [(SKX.SCHEDULES["twotile"][0], form, layout) for form in EX.FORMS for layout in EX.LAYOUTS]
    pairs += [(SKX.SCHEDULES[s][0], form, layout) for s in ("twotile", "sk_dp") for form, layout in SKX.OUTSIDE]
    out = []
    for shape, form, layout in pairs:
        for p in EX.FORMS[form].p:
            for kw in (dict(engine=2), dict(engine=0, sk=1), dict(engine=0, cus=37)):
                out.append((gemm_line(shape, form, p, layout=layout, **kw), SKX.sk_kernel(form, layout)))
    return out


def engine0_cases():
    """Engine 0 at the stream-K test's shape: the knob off and cus = 0 stay tiled; either one moves it."""
    line = lambda **kw: gemm_line(EX.SK, "relu_post", engine=0, **kw)
    tiled = "mfma/var6/128x128/ek0/split1"   # 30 tiles, 16 32-deep K steps: no split factor fills 240 CUs
    return [(line(), tiled), (line(w4=0), tiled), (line(sk=1), "sk/var0/256x256/ek4/split1"),
            (line(cus=37), "sk/var0/256x256/ek4/split1"),
            (gemm_line(EX.SK, "relu_post", engine=1, sk=1, cus=37), tiled)]


@pytest.fixture(scope="module")
def chooser(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    out = str(tmp_path_factory.mktemp("choose") / "gemm_choose")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__=1", "-I", CSRC, "-I", os.path.join(rocm, "include"),
           os.path.join(ROOT, "tests", "native", "gemm_choose.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime unavailable: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr

    def run(lines):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([out], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        assert "runtime error:" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        return r.stdout.splitlines()
    return run


def test_every_case_chooses_the_kernel_the_gpu_tests_assert(chooser):
    table = cases() + engine0_cases()
    got = chooser([line for line, _ in table])
    assert len(got) == len(table)
    wrong = []
    for (line, want), g in zip(table, got):
        name, _, row = g.partition(" ")
        if name.split("/")[0] in ("mfma", "w4", "pair"):
            if row != "row":
                wrong.append((line, g, "no row in the kernel table"))
        elif row:
            wrong.append((line, g, "a row flag on a family without a table"))
        if name != want.split(" ")[0]:
            wrong.append((line, g, want))
    assert not wrong, wrong[:10]
    names = {g.split(" ")[0] for g in got}
    print(f"{len(table)} cases, {len(names)} distinct kernels")
    # the cells the issue names
    assert F8.expected_kernel("v15", F8.SW4SHORT, "plain") == "mfma/var15/256x256/ek0/split1" in names
    assert {f"mfma/var14/256x256/ek1/split{s}" for s in (1, 4, 8)} <= names
    assert {f"sk/var0/256x256/ek{k}/split1" for k in (0, 1, 2, 3, 4, 5, 6, 100)} <= names


def test_the_stream_k_engine_is_chosen_exactly_where_it_has_a_kernel(chooser):
    table = sk_table_cases()
    got = chooser([line for line, _ in table])
    assert len(got) == len(table)
    wrong = []
    for (line, want), g in zip(table, got):
        name, _, row = g.partition(" ")
        family = name.split("/")[0]
        if want is not None:
            if name != want:
                wrong.append((line, g, want))
        elif family not in ("mfma", "w4", "generic") or (family != "generic" and row != "row"):
            wrong.append((line, g, "a tiled kernel with a row, or the generic one"))
    assert not wrong, wrong[:10]
    print(f"{len(table)} cases, {sum(w is not None for _, w in table)} on the engine")
    # the pairs gemm_choose used to hand the engine although it has no kernel for them
    for form, layout in SKX.OUTSIDE:
        assert SKX.sk_kernel(form, layout) is None and SKX.sk_kernel(form) is not None
