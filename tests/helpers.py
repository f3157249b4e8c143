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


def gather_seed(seed_lo: int, seed_hi: int, epoch: int | None) -> tuple[int, int]:
    """Minibatch sampler seeds of an epoch (the kernels' ``gather_seed``)."""
    lo, hi = seed_lo & 0xFFFFFFFF, seed_hi & 0xFFFFFFFF
    if epoch is not None:
        lo = (lo + epoch * 0x632BE5AB) & 0xFFFFFFFF
        hi = (hi ^ epoch) & 0xFFFFFFFF
    return lo, hi


def gather_picks(rows_valid: int, n_data: int, seed_lo: int, seed_hi: int, epoch: int | None = None) -> np.ndarray:
    """Data rows that ``gather_rows`` samples for output rows 0..rows_valid-1 (int64)."""
    lo, hi = gather_seed(seed_lo, seed_hi, epoch)
    row = np.arange(rows_valid, dtype=np.uint64)
    h = _mix32(_mix32(row ^ np.uint64(lo)) ^ np.uint64(hi))
    return ((h * np.uint64(n_data)) >> np.uint64(32)).astype(np.int64)


def keep2d(rows: int, cols: int, idx_ld: int, seed: tuple[int, int], lid: int, p: float,
           epoch: int | None = None) -> torch.Tensor:
    """Bool keep-mask of a [rows, cols] tensor whose element (r, c) has the logical index r * idx_ld + c."""
    ld = idx_ld if idx_ld > 0 else cols
    m = keep_mask(rows * ld, seed[0], seed[1], lid, p, epoch).reshape(rows, ld)[:, :cols]
    return torch.from_numpy(m.copy())


# fp64 activations by code (ops.functional ACT_*): forward, and the derivative from the OUTPUT a
ACT_FWD = {0: lambda z: z, 1: lambda z: torch.where(z > 0, z, torch.zeros_like(z)), 2: torch.sigmoid, 3: torch.tanh}
ACT_DOUT = {0: torch.ones_like, 1: lambda a: (a > 0).to(a.dtype), 2: lambda a: a * (1 - a), 3: lambda a: 1 - a * a}


def stage_fwd_reference(x: torch.Tensor, act: int, keep_pre, keep_post, scale) -> torch.Tensor:
    """``drop_post(act(drop_pre(x)))`` in x's dtype, one multiply per dropout (``scale`` a tensor of
    that dtype; a mask of None = no dropout). Dropped elements are +0."""
    zero = torch.zeros_like(x)
    v = x if keep_pre is None else torch.where(keep_pre, x * scale, zero)
    v = ACT_FWD[act](v)
    return v if keep_post is None else torch.where(keep_post, v * scale, zero)


def stage_bwd_reference(g: torch.Tensor, y: torch.Tensor, act: int, keep_pre, keep_post, scale: float) -> torch.Tensor:
    """fp64 ``g * scale_post keep_post * act'(y / scale_post) * scale_pre keep_pre`` from the stored output y."""
    g, a = g.double(), y.double()
    if keep_post is not None:
        g = g * keep_post.double() * scale
        a = a / scale if scale != 0.0 else a
    g = g * ACT_DOUT[act](a)
    if keep_pre is not None:
        g = g * keep_pre.double() * scale
    return g


def xent_reference(logits: torch.Tensor, labels: torch.Tensor, rows_valid: int, loss_scale: float, grad_scale: float,
                   keep=None, scale: float = 1.0) -> dict:
    """fp64 cross-entropy head over rows [0, rows_valid): ``probs``, ``dh`` = (p - onehot) * grad_scale
    through the logits' dropout (zero rows past rows_valid), ``loss`` and ``colsum`` with the sums of
    the absolute values of their terms (``loss_abs``, ``colsum_abs``)."""
    x = logits.double()
    rows, cols = x.shape
    probs = torch.softmax(x, 1)
    lab = labels[:rows_valid].long()
    terms = (torch.logsumexp(x[:rows_valid], 1) - x[:rows_valid].gather(1, lab[:, None])[:, 0]) * loss_scale
    dh = torch.zeros_like(x)
    dh[:rows_valid] = (probs[:rows_valid] - torch.nn.functional.one_hot(lab, cols)) * grad_scale
    if keep is not None:
        dh = dh * keep.double() * scale
    return {"probs": probs, "dh": dh, "loss": terms.sum().item(), "loss_abs": terms.abs().sum().item(),
            "colsum": dh.sum(0), "colsum_abs": dh.abs().sum(0)}
