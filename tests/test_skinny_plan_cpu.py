"""``PF.gemm_skinny_plan`` / ``PF.gemm_skinny_w8_plan`` (the launchers' own pz::skinny_plan / pz::skinny_w8_plan,
reported without a launch) checked without a GPU: every plan cell that tests/test_skinny_exact_gpu.py
claims for its shapes (its tables are imported, not copied), and the plans' own invariants."""
import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import test_skinny_exact_gpu as EX


def test_the_exact_tests_reach_the_cells_they_claim():
    for kern, K, N, plan, last in EX.CELLS:
        assert EX.plan_of(kern, K, N) == plan and EX.last_slice_rows(K, plan) == last, (kern, K, N)
    for kern in EX.STRIP_COLS:
        for tail in EX.TAILS:
            K = EX.TAIL_BASE_K + tail
            assert K <= EX.TAIL_K_MAX and EX.plan_of(kern, K, EX.tail_n(kern)) == (EX.TAIL_STRIPS, 3, 512), (kern, tail)
        N, plan, _ = EX.EVERY_ROW[kern]
        assert EX.plan_of(kern, 1104, N) == plan
    EX.test_the_cells_cover_every_slice_length_fold_shape_and_ring_turn(None)
    EX.test_tail_lengths_sit_on_both_sides_of_every_batch_size()


@pytest.mark.parametrize("kern", list(EX.STRIP_COLS))
def test_a_plan_covers_k_in_whole_granules_and_fits_the_x_stage(kern):
    """Whatever (K, N): the slices cover K with none empty, a slice is a whole number of 256-row
    granules no longer than the kernel's x stage, the strips cover N, and N alone decides them."""
    top = 512 if kern == "f32" else 1024
    for K in (1, 2, 255, 256, 257, 511, 777, 1024, 1025, 2049, 4096, 8191, 8192, 50000):
        for N in (16, 64, 80, 1024, 4096, 16448, 65536, 262144):
            strips, slices, slice_len = EX.plan_of(kern, K, N)
            assert strips == -(-N // EX.STRIP_COLS[kern])
            assert slice_len % 256 == 0 and 256 <= slice_len <= top
            assert (slices - 1) * slice_len < K <= slices * slice_len


def test_the_plan_of_other_operand_types_is_refused():
    with pytest.raises(ValueError, match="bf16 / fp32"):
        PF.gemm_skinny_plan(64, 64, torch.float64)
    with pytest.raises(RuntimeError):
        PF.gemm_skinny_plan(0, 64, torch.bfloat16)
    with pytest.raises(RuntimeError):
        PF.gemm_skinny_w8_plan(64, 0)
