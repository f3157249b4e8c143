"""The persistent stream-K GEMM (csrc/gemm_sk.hip, engine 2), value for value, on every shape of
schedule ``sk_plan`` (csrc/gemm_sk_plan.h) produces and on every epilogue the engine has a kernel for.

Method and bounds: test_gemm_exact_gpu.run_case and test_gemm_pair_update_gpu.run_pair, unchanged
(integer operands in [-4, 4], so the stream-K fold adds exact integers in any order; outputs start as
NaN; none / ReLU forms at p = 0.5 and 1.0 EQUAL bf16_rne(fp32(ref)) / fp32(ref), p = 0.3 and sigmoid /
tanh keep run_case's 2^-8 bounds; column sums, fp8 codes and amax exact).

Every test asserts the schedule it means to run through ``PF.gemm_sk_plan`` BEFORE it launches (the
plans below are those of a 256-CU device with these budgets; on another device the assertion fails
instead of another schedule being tested) and the kernel through ``PF.gemm_last_kernel()``.
Tiles are 256 x 256 and K steps 64 deep: SCHEDULES holds the smallest shapes that reach each form of
schedule. tests/test_gemm_sk_plan_cpu.py walks these very schedules with the header's own functions
on the host and asserts the unit patterns the ``reaches`` column claims.

  name          M x N       K    cus  (grid, sk_tiles)  reaches
  dp2           768 x 512   320  3    (3, 0)   two data-parallel rounds
  serial        512 x 768   320  1    (1, 0)   six tiles on one workgroup
  halves_odd    768 x 512   576  12   (12, 6)  4 + 5 step K halves (also with cus = 0)
  short_k       768 x 512   256  200  (6, 0)   too shallow to halve
  twotile       768 x 512   320  4    (4, 6)   WP / PW workgroups, uneven cuts
  twotile_pp    1280 x 256  256  4    (4, 5)   PP workgroups, one-step partials
  twotile_pwp   256 x 1792  320  4    (4, 7)   PWP workgroups
  twotile_k128  1792 x 256  128  4    (4, 7)   one-step partials at the minimum K
  sk_dp         1024 x 512  320  3    (3, 5)   a stream-K region, then one data-parallel round
  sk_dp2        2816 x 256  320  3    (3, 5)   a stream-K region, then two data-parallel rounds

SK_FORMS is every form of test_gemm_exact_gpu.FORMS the engine has a kernel for: SK_TABLE restates
kSk (csrc/gemm_dispatch.h), and tests/test_gemm_choose_cpu.py checks the restatement against
gemm_choose for every form in every layout. A (layout, kind) pair outside the table stays on the tiled
kernels under engine 0 and is refused under engine 2 (test_pairs_outside_the_table_*).

Measured on MI355X (the file takes about 3 s): every plan as stated, every none / ReLU form at p = 0.5 and
1.0 exact on every schedule, pairs and back-to-back launches included. Worst err / bound: p = 0.3 kept
values 0.963, their column sums 0.002 (run_case's bounds; the rounding is the epilogue's, the fold adds
integers). Before the table, engine 0 with a CU budget failed the OUTSIDE cases with hipErrorInvalidValue.
"""
import math

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.test_gemm_exact_gpu import BF16, DEV, F32, FORMS, SHAPES, epi_kind, expected_kernel, run_case
from tests.test_gemm_pair_update_gpu import run_pair

pytestmark = pytest.mark.gpu

# name -> (shape, cus, (grid, sk_tiles) on a 256-CU device)
SCHEDULES = {
    "dp2": ((768, 512, 320), 3, (3, 0)),
    "serial": ((512, 768, 320), 1, (1, 0)),
    "halves_odd": ((768, 512, 576), 12, (12, 6)),
    "halves_odd_all_cus": ((768, 512, 576), 0, (12, 6)),
    "short_k": ((768, 512, 256), 200, (6, 0)),
    "twotile": ((768, 512, 320), 4, (4, 6)),
    "twotile_pp": ((1280, 256, 256), 4, (4, 5)),
    "twotile_pwp": ((256, 1792, 320), 4, (4, 7)),
    "twotile_k128": ((1792, 256, 128), 4, (4, 7)),
    "sk_dp": ((1024, 512, 320), 3, (3, 5)),
    "sk_dp2": ((2816, 256, 320), 3, (3, 5)),
}
# what the host walk of each schedule must show (tests/test_gemm_sk_plan_cpu.py): regime class, and
# unit patterns some workgroup has (W a whole tile, P a partial one, Wn two or more whole tiles)
REACHES = {
    "dp2": ("dp_rounds", {"Wn"}),
    "serial": ("dp_rounds", {"Wn"}),
    "halves_odd": ("halves_odd", {"P"}),
    "halves_odd_all_cus": ("halves_odd", {"P"}),
    "short_k": ("dp_one_round", {"W"}),
    "twotile": ("twotile", {"WP", "PW"}),
    "twotile_pp": ("twotile", {"PP", "WP", "PW"}),
    "twotile_pwp": ("twotile", {"PWP", "WP", "PW"}),
    "twotile_k128": ("twotile", {"PWP", "WP", "Wn"}),
    "sk_dp": ("twotile_dp", {"WPW", "PWPW", "PWn"}),
    "sk_dp2": ("twotile_dp", {"WPWn", "PWPWn", "PWn"}),
}
# the pairs of test_pairs_share_one_schedule: (shape 0, shape 1, K, cus, (grid, sk_tiles))
PAIRS = {
    "boundary_in_sk_region": ((768, 256), (256, 1024), 320, 4, (4, 7)),
    "sk_region_then_dp": ((768, 256), (256, 1024), 320, 3, (3, 4)),
}

# kSk (csrc/gemm_dispatch.h): the engine's epilogue codes per operand layout (100 = the fp32 store)
SK_TABLE = {"fwd": {0, 1, 2, 4, 5, 6}, "dx": {0, 1, 3}, "dw": {1, 100}, "tn": set()}


def sk_code(form):
    """The stream-K engine's epilogue code for ``form`` (sk_epilogue, csrc/gemm_dispatch.h), whatever
    the layout: None where its epilogues cannot do what the form asks."""
    f = FORMS[form]
    if f.out == F32:
        return 100 if f.mode == PF.EPI_STORE and not (f.mask or f.out8 or f.colsum) else None
    if f.out != BF16 or f.accumulate or (f.mode == PF.EPI_STORE and f.out8):
        return None
    return epi_kind(f)


def sk_kernel(form, layout=None):
    """gemm_last_kernel() of ``form`` on the stream-K engine, None where it has no kernel (the GEMM
    stays on the tiled kernels)."""
    code = sk_code(form)
    return f"sk/var0/256x256/ek{code}/split1" if code in SK_TABLE[layout or FORMS[form].layout] else None


SK_FORMS = [n for n in FORMS if sk_kernel(n) is not None]
# (layout, kind) pairs gemm_choose used to hand the engine although it has no kernel for them: form, layout
OUTSIDE = [("store_bias", "dw"), ("dx_store_colsum", "dw"),          # the dW layout with the generic epilogue
           ("relu_prepost", "dx"), ("relu_nodrop", "dx"),            # a forward stage on a K-contiguous weight
           ("dx_relu_mask", "fwd"), ("dx_relu_mask_out8", "fwd")]    # the bitmask backward in the forward layout
OUTSIDE_SHAPE = SCHEDULES["twotile"][0]
OUTSIDE_TILED = "mfma/var6/128x128/ek0/split1"   # 6 tiles, 10 32-deep K steps: no split, 128 x 128 tiles


def alpha_kw(form, K):
    """run_case's alpha for the forward fp8-copy forms: alpha_of sizes it for K <= 192 and K = 4096, where
    std(alpha z) = 6.67 sqrt(K) alpha is about 850 and some |y| 2^-3 pass e4m3's 448 (run_case asserts
    that the clamp ran). Here K is in between and the outputs are few: the power of two nearest
    256 / sqrt(K), std(alpha z) about 1700, so that 3584 is 2 to 3 sigma away."""
    f = FORMS[form]
    return dict(alpha=2.0 ** round(math.log2(256 / math.sqrt(K)))) if f.out8 and f.mode == PF.EPI_FWD else {}


def assert_plan(sched):
    shape, cus, want = SCHEDULES[sched]
    M, N, K = shape
    plan = PF.gemm_sk_plan(M, N, K, cus)
    print(f"{sched}: {shape} on cus={cus}: (grid, sk_tiles, iters, tiles) = {plan}")
    assert plan == (*want, K // 64, (M // 256) * (N // 256)), (sched, plan)
    return shape, cus


def run_sched(sched, form, **kw):
    """Every dropout probability of ``form`` on schedule ``sched``; returns the p = 0.5 (first) result."""
    shape, cus = assert_plan(sched)
    first = None
    for p in FORMS[form].p:
        r = run_case(shape, form, p, engine=2, cus=cus, **alpha_kw(form, shape[2]), **kw)
        assert r.name == sk_kernel(form), (sched, form, r.name)
        first = first or r
    return first


def test_the_form_list_is_the_one_the_issue_counts():
    """27 of FORMS' 30: everything but the (A M-contiguous, B K-contiguous) layout and bf16 accumulate."""
    assert set(FORMS) - set(SK_FORMS) == {"tn_bf16", "tn_f32", "fwd_acc"}
    assert {sk_kernel(f).split("/")[3] for f in SK_FORMS} == {f"ek{k}" for k in (0, 1, 2, 3, 4, 5, 6, 100)}


@pytest.mark.parametrize("sched", ["twotile_pwp", "halves_odd", "sk_dp"])
@pytest.mark.parametrize("form", SK_FORMS)
def test_every_form_is_exact_on_three_schedules(native_lib, form, sched):
    run_sched(sched, form)


@pytest.mark.parametrize("form", ["relu_prepost", "dx_relu_mask", "dx_tanh_aux", "dw_f32_acc", "relu_prepost_out8"])
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_every_schedule_is_exact(native_lib, sched, form):
    run_sched(sched, form)


@pytest.mark.parametrize("form", ["relu_prepost_out8", "dx_relu_aux", "dw_f32_acc"])
def test_strided_views_write_nothing_outside_the_slice(native_lib, form):
    """A, B, C, aux and out8 as column slices of wider tensors filled with 7: the contiguous call's
    results, and every element outside the slices still 7 (run_case checks the frames)."""
    flat = run_sched("twotile", form)
    view = run_sched("twotile", form, strided=True)
    N = SCHEDULES["twotile"][0][1]
    assert view.c.stride(0) == N + 16 and torch.equal(view.c, flat.c)
    if view.out8 is not None:
        assert torch.equal(view.out8.contiguous().view(torch.uint8), flat.out8.view(torch.uint8))
        assert torch.equal(view.amax, flat.amax) and torch.equal(view.mask, flat.mask)
    if view.colsum is not None:
        assert torch.equal(view.colsum, flat.colsum)


def test_idx_ld_strides_the_dropout_element_index(native_lib):
    N = SCHEDULES["twotile"][0][1]
    r = run_sched("twotile", "relu_prepost", idx_ld=N + 64)
    assert not torch.equal(r.c, run_sched("twotile", "relu_prepost").c)


@pytest.mark.parametrize("form", ["relu_prepost_out8", "dx_relu_mask_out8"])
def test_store_c_false_writes_only_the_side_outputs(native_lib, form):
    """store_c = False (gemm_choose keeps these on the engine: sk_eligible takes a null C): C untouched,
    the fp8 copy, amax, bitmask and column sums identical."""
    shape, cus = assert_plan("twotile")
    full = run_case(shape, form, engine=2, cus=cus, **alpha_kw(form, shape[2]))
    side = run_case(shape, form, engine=2, cus=cus, store_c=False, **alpha_kw(form, shape[2]))
    assert side.name == full.name == sk_kernel(form)
    assert torch.equal(side.out8.view(torch.uint8), full.out8.view(torch.uint8)) and torch.equal(side.amax, full.amax)
    if FORMS[form].mode == PF.EPI_FWD:
        assert torch.equal(side.mask, full.mask)
    else:
        assert torch.equal(side.colsum, full.colsum)


@pytest.mark.parametrize("kind", ["bf16", "f32"])
@pytest.mark.parametrize("swap", [False, True], ids=["order01", "order10"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_pairs_share_one_schedule(native_lib, pair, swap, kind):
    """gemm_pair on the engine, three launches each (run_pair): 3 + 4 tiles on 4 workgroups, where the
    boundary between the problems falls inside the stream-K region (a tile of each problem cut), and on
    3, where a stream-K region is followed by data-parallel tiles of the second problem."""
    s0, s1, K, cus, want = PAIRS[pair]
    if swap:
        s0, s1 = s1, s0
    plan = PF.gemm_sk_plan(*s0, K, cus, *s1)
    print(f"{pair}: {s0} + {s1}, K = {K}, on cus={cus}: (grid, sk_tiles, iters, tiles) = {plan}")
    assert plan == (*want, K // 64, 7)
    run_pair(s0, s1, K, kind, 1, engine=2, cus=cus, name=f"sk/var0/256x256/ek{1 if kind == 'bf16' else 100}/split1")


def test_tickets_and_slabs_are_clean_between_launches(native_lib):
    """Stream-K schedules and split-K tiled GEMMs back to back (they share the ticket cache; the slabs
    come from the caching allocator): each leaves its tickets at zero and reads no stale slab, so every
    result is exact and the first and the last launch agree bit for bit. Before the last launch a
    NaN-filled tensor of the workspace's size is freed: the allocator is likely (not certain) to hand
    those NaNs back as the slabs."""
    first = run_sched("twotile", "relu_prepost")
    split = expected_kernel("Ssplit", "dw_f32_acc")
    assert split.endswith("/split8")
    assert run_case(SHAPES["Ssplit"], "dw_f32_acc", engine=1).name == split
    run_sched("halves_odd", "relu_prepost")
    run_sched("twotile_pwp", "dx_relu_mask")
    assert run_case(SHAPES["Ssplit"], "dw_f32_acc", engine=1).name == split
    grid = SCHEDULES["twotile"][2][0]
    poison = torch.full((2 * grid * 256 * 256,), float("nan"), device=DEV, dtype=F32)
    del poison
    last = run_sched("twotile", "relu_prepost")
    assert torch.equal(first.c, last.c) and torch.equal(first.mask, last.mask)


@pytest.mark.parametrize("form,layout", OUTSIDE, ids=[f"{f}-as-{lay}" for f, lay in OUTSIDE])
def test_pairs_outside_the_table_are_refused_by_engine_2(native_lib, form, layout):
    assert sk_kernel(form, layout) is None and sk_kernel(form) is not None
    with pytest.raises(RuntimeError, match="stream-K engine cannot run"):
        run_case(OUTSIDE_SHAPE, form, layout=layout, engine=2, cus=37)


@pytest.mark.parametrize("form,layout", OUTSIDE, ids=[f"{f}-as-{lay}" for f, lay in OUTSIDE])
def test_pairs_outside_the_table_run_tiled_under_a_cu_budget(native_lib, form, layout):
    """Engine 0 with a CU budget picks the stream-K engine wherever it is eligible: these stay tiled, exactly."""
    for p in FORMS[form].p:
        assert run_case(OUTSIDE_SHAPE, form, p, layout=layout, engine=0, cus=37).name == OUTSIDE_TILED
    # the same forms in their own layouts do move to the engine (6 tiles of 5 steps: one workgroup each)
    assert PF.gemm_sk_plan(*OUTSIDE_SHAPE, 37) == (6, 0, 5, 6)
    assert run_case(OUTSIDE_SHAPE, form, engine=0, cus=37).name == sk_kernel(form)
