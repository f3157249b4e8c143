"""Independent (numpy / plain torch) re-implementations used as references by the kernel tests."""
import numpy as np
import torch

from penr_oz_neural_network_torch_amd.ops.functional import epoch_key, layer_key

M32 = np.uint64(0xFFFFFFFF)


def _mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def keep_mask(numel: int, seed_lo: int, seed_hi: int, lid: int, p: float, epoch: int | None = None) -> np.ndarray:
    """Dropout keep-mask of the pz kernels for logical element indices 0..numel-1 (``epoch``: the
    per-epoch key of a training step, as the fused trainer derives it)."""
    thresh = min(65536, int(round(p * 65536)))
    key = layer_key((seed_lo, seed_hi), lid)
    if epoch is not None:
        key = epoch_key(key, epoch)
    key = np.uint64(key)
    idx = np.arange(numel, dtype=np.uint64)
    bits = _mix32((idx >> np.uint64(1)) ^ key)
    r = np.where(idx & np.uint64(1), bits >> np.uint64(16), bits & np.uint64(0xFFFF))
    return r >= np.uint64(thresh)


def bit_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape, dtype and bytes (NaN payloads and the sign of zero included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def opt_update_reference(p0, graw, m0, v0, weight, dtype, *, adam, lr, b1, b2, eps, bc1, bc2s, grad_scale, l2):
    """``opt_update`` (csrc/pz_common.h) evaluated by plain torch in ``dtype``, operation for
    operation: every hyper-parameter is rounded once to ``dtype`` and ``1 - beta`` is formed in
    ``dtype``, as the kernel does. ``weight``: bool mask of the elements that take the L2 term.
    Returns ``(p, m, v)``; SGD returns the moments it was given."""
    def s(x):
        return torch.tensor(x, dtype=dtype)

    p0, graw = p0.to(dtype), graw.to(dtype)
    l2x2 = weight.to(dtype) * (s(2.0) * s(l2))
    g = graw * s(grad_scale) + l2x2 * p0
    if not adam:
        return p0 - s(lr) * g, m0, v0
    m0, v0 = m0.to(dtype), v0.to(dtype)
    m = m0 + (s(1.0) - s(b1)) * (g - m0)
    v = v0 * s(b2) + (s(1.0) - s(b2)) * g * g
    denom = v.sqrt() / s(bc2s) + s(eps)
    return p0 - (s(lr) / s(bc1)) * (m / denom), m, v
