"""The host references the GPU kernel tests lean on, against plain Python-int arithmetic."""
import numpy as np
import pytest

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import gather_picks, gather_seed, keep2d, keep_mask

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
