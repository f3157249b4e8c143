"""The host references the GPU kernel tests lean on, against plain Python-int arithmetic."""
import numpy as np
import pytest

import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import (fp8_code_values, fp8_encode_reference, fp8_tie_points, gather_picks, gather_seed,
                           histogram_reference, keep2d, keep_mask)

M32 = 0xFFFFFFFF


def picks_by_hand(rows_valid, n_data, lo, hi, epoch):
    if epoch is not None:
        lo = (lo + epoch * 0x632BE5AB) % 2 ** 32
        hi = (hi ^ epoch) % 2 ** 32
    return [(PF.mix32(PF.mix32(row ^ lo) ^ hi) * n_data) >> 32 for row in range(rows_valid)]


@pytest.mark.parametrize("seed,n_data,epoch", [
    ((11, 22), 1000, None),
    ((0xDEADBEEF, 0x0BADF00D), 1000, 5),
    ((0xFFFFFFFF, 0xFFFFFFFF), 3, 7),            # lo + epoch * c wraps
    ((0, 0), 1, 0),
    ((0x2468ACE0, 0x13579BDF), 2 ** 31 + 12345, 123456),
    ((5, 9), 60000, 2 ** 31 - 1),
])
def test_gather_picks_matches_python_ints(seed, n_data, epoch):
    got = gather_picks(257, n_data, seed[0], seed[1], epoch)
    assert got.dtype == np.int64 and got.shape == (257,)
    assert got.tolist() == picks_by_hand(257, n_data, seed[0], seed[1], epoch)
    assert (got >= 0).all() and (got < n_data).all()
    if n_data == 1:
        assert (got == 0).all()


def test_gather_picks_spread_and_epoch_zero():
    a = gather_picks(1000, 1000, 1, 2)
    assert len(set(a.tolist())) > 500  # sampling with replacement: about 632 distinct of 1000
    assert not np.array_equal(a, gather_picks(1000, 1000, 1, 2, epoch=1))
    assert np.array_equal(a, gather_picks(1000, 1000, 1, 2, epoch=0))  # epoch 0 changes neither seed
    assert gather_seed(1, 2, None) == (1, 2) and gather_seed(M32, 6, 3) == ((M32 + 3 * 0x632BE5AB) & M32, 5)
    assert gather_picks(0, 10, 1, 2).shape == (0,)


def test_keep2d_is_the_flat_mask_at_row_stride():
    flat = keep_mask(5 * 16, 3, 4, 2, 0.25, epoch=3).reshape(5, 16)
    assert np.array_equal(keep2d(5, 10, 16, (3, 4), 2, 0.25, epoch=3).numpy(), flat[:, :10])
    assert np.array_equal(keep2d(5, 16, 0, (3, 4), 2, 0.25, epoch=3).numpy(), flat)


FP8 = {"e4m3": (torch.float8_e4m3fn, 448.0, 1020), "e5m2": (torch.float8_e5m2, 57344.0, 996)}


@pytest.mark.parametrize("name", list(FP8))
def test_fp8_code_table_is_the_formats(name):
    fmt, top, _ = FP8[name]
    table = fp8_code_values(fmt)
    by_view = torch.arange(len(table), dtype=torch.uint8).view(fmt).double().numpy()
    assert np.array_equal(table, by_view) and table[-1] == top and (np.diff(table) > 0).all()
    assert not torch.isfinite(torch.tensor([len(table)], dtype=torch.uint8).view(fmt).float()).any()


@pytest.mark.parametrize("name", list(FP8))
def test_fp8_encode_reference_matches_torch_cpu_cast(name):
    """The table-built encoder against torch's CPU cast of the clamped value on every code, every
    midpoint (the ties), their fp32 neighbours, subnormal and out-of-range points, both signs."""
    fmt, top, count = FP8[name]
    pts = fp8_tie_points(fmt)
    assert pts.dtype == torch.float32 and pts.numel() == count and not torch.isnan(pts).any()
    assert torch.equal(pts[:count // 2], -pts[count // 2:])
    got = fp8_encode_reference(pts.double(), fmt)
    ref = pts.clamp(-top, top).to(fmt).view(torch.uint8)
    assert got.dtype == torch.uint8 and torch.equal(got, ref)
    # spot checks by hand: ties to even, the sign of zero, saturation
    table = fp8_code_values(fmt)
    hand = torch.tensor([0.0, -0.0, (table[1] + table[2]) / 2, (table[2] + table[3]) / 2, table[1] / 2, 1e30, -1e30],
                        dtype=torch.float64)
    last = len(table) - 1
    assert fp8_encode_reference(hand, fmt).tolist() == [0, 0x80, 2, 2, 0, last, 0x80 | last]
    # the same points through an exact scale pair, as the codebook GPU test feeds them
    assert torch.equal((pts * 8) * 0.125, pts)


@pytest.mark.parametrize("lo,hi,bins", [(0.0, 8.0, 1), (0.0, 8.0, 8), (0.0, 8.0, 64), (-4.0, 4.0, 8),
                                        (-4.0, 4.0, 64), (0.0, 100.0, 100)])
def test_histogram_reference_matches_torch_histogram(lo, hi, bins):
    v = torch.arange(int(lo * 8) - 16, int(hi * 8) + 17, dtype=torch.float64) / 8  # every edge, hi, outside
    v = torch.cat([v, v[::3], torch.tensor([hi, hi, lo])])
    ref = torch.histogram(v, bins=bins, range=(lo, hi)).hist
    got = histogram_reference(torch.cat([v, torch.tensor([float("nan")])]), lo, hi, bins)
    assert got.dtype == np.int64 and got.tolist() == ref.tolist()
    assert got.sum() == ((v >= lo) & (v <= hi)).sum().item()


@pytest.mark.parametrize("bins", [1, 7, 8, 100])
def test_degenerate_histogram_bin(bins):
    """torch.histogram widens an all-equal range to [c - 0.5, c + 0.5]: everything lands in bin bins // 2
    (what the GPU test of the lo == hi range expects)."""
    h = torch.histogram(torch.full((10,), 3.0, dtype=torch.float64), bins=bins).hist
    want = [0] * bins
    want[bins // 2] = 10
    assert h.tolist() == want
