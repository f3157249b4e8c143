"""Independent (numpy / plain torch) re-implementations used as references by the kernel tests."""
import functools

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


# ------------------------------------------------------------------------------------------- fp8
# (exponent bits, mantissa bits, bias, largest finite code) of the two OCP 8-bit formats
_FP8 = {torch.float8_e4m3fn: (4, 3, 7, 0x7E), torch.float8_e5m2: (5, 2, 15, 0x7B)}


def fp8_code_values(fmt) -> np.ndarray:
    """The finite non-negative values of ``fmt`` by code (fp64, ascending: index == code), from the
    format's definition: 2^(1 - bias) * m / 2^mbits for exponent field 0, 2^(e - bias) * (1 + m / 2^mbits)
    otherwise. e4m3fn: 0 .. 0x7E (448; 0x7F is NaN), e5m2: 0 .. 0x7B (57344; 0x7C is inf)."""
    _, mbits, bias, last = _FP8[fmt]
    code = np.arange(last + 1)
    e, m = code >> mbits, (code & ((1 << mbits) - 1)).astype(np.float64)
    return np.where(e == 0, np.ldexp(m, 1 - bias - mbits), np.ldexp(1.0 + np.ldexp(m, -mbits), e - bias))


def fp8_encode_reference(values_fp64, fmt) -> torch.Tensor:
    """uint8 codes of the nearest finite ``fmt`` value of each fp64 input: ties go to the even code,
    the sign bit is the input's (zero included), |v| past the largest finite value (inf included)
    saturates there. Built from the code table alone: the two neighbouring codes and their midpoint
    (a sum of two neighbours halves exactly in fp64), no float8 cast of the input. NaN is not handled."""
    v = np.asarray(torch.as_tensor(values_fp64, dtype=torch.float64).numpy())
    assert not np.isnan(v).any()
    table = fp8_code_values(fmt)
    last = len(table) - 1
    a = np.minimum(np.abs(v), table[last])
    lo = np.searchsorted(table, a, side="right") - 1   # table[lo] <= a
    hi = np.minimum(lo + 1, last)
    mid = (table[lo] + table[hi]) / 2
    code = np.where(a > mid, hi, np.where(a < mid, lo, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(lo == hi, lo, code)
    return torch.from_numpy((code | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8))


def fp8_tie_points(fmt) -> torch.Tensor:
    """fp32 points where an fp8 rounding rule can go wrong: every finite non-negative code value,
    every midpoint of two neighbouring codes, the fp32 neighbour of each midpoint on both sides,
    2^-149, 2^-126, 1.5 * max, 1e30 and +inf; all of them with both signs (no NaN)."""
    table = fp8_code_values(fmt)
    codes = torch.from_numpy(table).float()
    assert torch.equal(codes.double(), torch.from_numpy(table))
    mids = (codes[:-1] + codes[1:]) / 2
    assert torch.equal(mids.double() * 2, torch.from_numpy(table[:-1] + table[1:]))
    inf = torch.tensor(float("inf"))
    extra = torch.tensor([2.0 ** -149, 2.0 ** -126, 1.5 * table[-1], 1e30, float("inf")], dtype=torch.float32)
    pos = torch.cat([codes, mids, torch.nextafter(mids, -inf), torch.nextafter(mids, inf), extra])
    return torch.cat([pos, -pos])


def histogram_reference(values, lo: float, hi: float, bins: int) -> np.ndarray:
    """int64 counts of ``bins`` equal bins over [lo, hi] (the last one closed) by integer arithmetic.
    ``values`` (any float tensor; NaN allowed, never counted), ``lo`` and ``hi`` must be multiples of
    1/8: the value k/8 then lies in bin floor((k - 8 lo) * bins / (8 hi - 8 lo)), a quotient of
    integers, and ``hi`` itself in the last bin."""
    v = torch.as_tensor(values).double().numpy().ravel()
    v = v[~np.isnan(v)] * 8
    k, lo8, hi8 = np.rint(v).astype(np.int64), int(round(lo * 8)), int(round(hi * 8))
    assert np.array_equal(k.astype(np.float64), v) and lo8 == lo * 8 and hi8 == hi * 8 and hi8 > lo8
    k = k[(k >= lo8) & (k <= hi8)]
    b = np.minimum(((k - lo8) * bins) // (hi8 - lo8), bins - 1)
    return np.bincount(b, minlength=bins).astype(np.int64)


# ------------------------------------------------------------------------------------ exact GEMM
def exact_operands(M: int, N: int, K: int, a_kc: bool, b_kc: bool, seed: int, dtype=torch.bfloat16, hi: int = 4):
    """``a`` ([M, K] if ``a_kc`` else [K, M]) and ``b`` ([N, K] if ``b_kc`` else [K, N]) in ``dtype``
    (bf16, fp32 or fp64) with integer entries in [-hi, hi] from a CPU generator, and the fp64
    ``z = op(a) @ op(b)``. Every partial sum of ``z`` is an integer below K hi^2, which must stay
    under 2^24 (bf16 / fp32 operands: every fp32 accumulation order gives ``z``) or 2^53 (fp64
    operands: every fp64 order does, the reference's own matmul included). bf16 holds the integers up
    to 256."""
    assert dtype in (torch.bfloat16, torch.float32, torch.float64) and hi >= 1
    assert K * hi * hi < (2 ** 53 if dtype == torch.float64 else 2 ** 24)
    assert dtype != torch.bfloat16 or hi <= 256
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randint(-hi, hi + 1, (M, K) if a_kc else (K, M), generator=g).to(dtype)
    b = torch.randint(-hi, hi + 1, (N, K) if b_kc else (K, N), generator=g).to(dtype)
    return a, b, (a.double() if a_kc else a.double().t()) @ (b.double().t() if b_kc else b.double())


def gemm_epilogue_reference(z: torch.Tensor, *, alpha: float, bias, mode: int, act: int, keep_pre, keep_post,
                            scale: float, aux=None, bits=None, c_old=None):
    """fp64 value the GEMM epilogue stores for the fp64 product ``z``, and its column sums (the
    ``colsum`` side output sums the values before they are rounded to the output type).
    ``mode`` 0 (EPI_STORE): ``alpha z + bias``; 1 (EPI_FWD): ``drop_post(act(drop_pre(alpha z + bias)))``;
    2 (EPI_BWD): ``alpha z`` through the stage's derivative, from the stored output ``aux`` or, for a
    ReLU stage, from ``bits`` = (y > 0): ``g * bits * scale_pre * scale_post`` (a keep mask that is
    not None switches that dropout's scale on; its entries are already part of ``bits``).
    ``c_old``: the previous C of an accumulating GEMM, added last."""
    h = z.double() * alpha
    if mode == 2:
        assert bias is None
        if bits is not None:
            total = (scale if keep_pre is not None else 1.0) * (scale if keep_post is not None else 1.0)
            out = h * bits.double() * total
        else:
            out = stage_bwd_reference(h, aux, act, keep_pre, keep_post, scale)
    else:
        if bias is not None:
            h = h + bias.double()
        out = h if mode == 0 else stage_fwd_reference(h, act, keep_pre, keep_post, torch.tensor(scale, dtype=torch.float64))
    if c_old is not None:
        out = out + c_old.double()
    return out, out.sum(0)


def assert_gemm_exact(out: torch.Tensor, ref64: torch.Tensor) -> None:
    """``out`` holds exactly the fp64 reference rounded once to its dtype. The reference must be
    fp32-representable (the kernels' epilogue math is fp32: only then is "exact" meaningful); the
    comparison is by value, so -0 equals +0. An fp64 ``out`` (the fp64 kernels' epilogue math is
    fp64) must equal ``ref64`` itself, which then need not fit fp32."""
    assert torch.isfinite(out).all()
    if out.dtype == torch.float64:
        assert ref64.dtype == torch.float64
        if not torch.equal(out, ref64):
            bad = out != ref64
            i = bad.nonzero()[0].tolist()
            raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements differ; first at {i}: "
                                 f"{out[tuple(i)].item()!r} != {ref64[tuple(i)].item()!r}")
        return
    assert torch.equal(ref64.float().double(), ref64), "the reference is not exact in fp32"
    want = ref64.float().to(out.dtype)
    if not torch.equal(out.float(), want.float()):
        bad = out.float() != want.float()
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements differ; first at {i}: "
                             f"{out[tuple(i)].item()} != {want[tuple(i)].item()}")


@functools.lru_cache(maxsize=64)
def keep2d_cached(rows: int, cols: int, idx_ld: int, seed: tuple[int, int], lid: int, p: float) -> torch.Tensor:
    """:func:`keep2d`, remembered per argument tuple (15.7 M elements take about a second in numpy);
    callers must not modify the result."""
    return keep2d(rows, cols, idx_ld, seed, lid, p)


# ---------------------------------------------------------------------------- exact fp8 GEMM / split plans
def exact_operands_fp8(M: int, N: int, K: int, a_kc: bool, b_kc: bool, fmt_a, fmt_b, seed: int):
    """:func:`exact_operands` cast to the fp8 formats ``fmt_a`` / ``fmt_b``: integers in [-4, 4] are
    exact in e4m3 and in e5m2, so ``z`` is the fp64 product of the fp8 values themselves."""
    a, b, z = exact_operands(M, N, K, a_kc, b_kc, seed)
    return a.to(fmt_a), b.to(fmt_b), z


def fp8_all_codes(fmt):
    """Every finite code of ``fmt`` (both signs, zeros and subnormals included, no NaN / inf) as a
    uint8 tensor, and the fp64 value of each, from :func:`fp8_code_values`."""
    table = fp8_code_values(fmt)
    code = np.arange(len(table), dtype=np.uint8)
    return torch.from_numpy(np.concatenate([code, code | 0x80])), torch.from_numpy(np.concatenate([table, -table]))


K_FILL = 240  # workgroups that fill the device (kFill in csrc/gemm_mfma.hip)


def _split_for(tiles: int, nk: int, factors) -> int:
    for sp in factors:
        if tiles * sp >= K_FILL and nk % sp == 0 and nk // sp >= 16:
            return sp
    return 0


def gemm_split_plan(M: int, N: int, K: int, *, fp8: bool = False, b_kc: bool = False) -> int:
    """``pz::gemm_split`` restated for an MFMA-eligible GEMM outside the bf16 fixed-kind 256x128 rule:
    fp8 GEMMs with a K-contiguous B never split; otherwise the first factor of 2, 4, 8 that fills the
    device with 256 x 256 tiles and leaves each slice >= 16 K steps (32 deep for bf16, 64 for fp8)."""
    if fp8 and b_kc:
        return 1
    tiles = -(-M // 256) * -(-N // 256)
    if tiles >= K_FILL:
        return 1
    return _split_for(tiles, K // (64 if fp8 else 32), (2, 4, 8)) or 1


def gemm_pair_split_plan(shape0, shape1, K: int) -> int:
    """``pz::gemm_pair_split`` restated for an eligible pair (whole 256-tiles, K % 64 == 0): the first
    factor of 1, 2, 4, 8 that fills the device with both problems' tiles at >= 16 64-deep K steps a
    slice; failing that 8 wherever 8 slices of >= 16 steps exist, else 1."""
    tiles = (shape0[0] // 256) * (shape0[1] // 256) + (shape1[0] // 256) * (shape1[1] // 256)
    nk = K // 64
    return _split_for(tiles, nk, (1, 2, 4, 8)) or (8 if nk % 8 == 0 and nk // 8 >= 16 else 1)


# the SGD hyper-parameters of the exact gemm_update tests: all powers of two, so that with an integer
# gradient and p0 in multiples of 1/8 every intermediate of p0 - lr (g scale + 2 l2 p0) is exact in fp32
SGD_EXACT = dict(lr=2.0 ** -6, grad_scale=0.5, l2=2.0 ** -4)

# Split-K factors the GPU tests claim for their shapes (asserted there through gemm_last_kernel /
# gemm_pair_split, and on the CPU against the two restatements above)
FP8_SPLIT_CASES = [  # (M, N, K, b_kc, split): fp8 operands
    ((1536, 2560, 4096), False, 4), ((1528, 2560, 4096), False, 4), ((1536, 1280, 8192), False, 8),
    ((512, 768, 320), False, 1), ((512, 256, 320), False, 1), ((4096, 3840, 64), False, 1),
    ((1536, 2560, 4096), True, 1), ((8192, 1024, 8192), True, 1)]
PAIR_SPLIT_CASES = [  # ((M0, N0), (M1, N1), K, split)
    ((256, 256), (256, 512), 64, 1), ((1536, 2560), (2560, 1536), 2048, 2), ((1536, 1280), (1280, 1536), 4096, 4),
    ((256, 512), (512, 256), 8192, 8), ((4096, 3840), (256, 256), 1024, 1)]
UPDATE_SPLIT_CASES = [  # (M, N, K, split): bf16 operands, fp32 state
    ((256, 256, 64), 1), ((200, 136, 96), 1), ((4088, 3832, 64), 1), ((512, 4096, 512), 1), ((1536, 1280, 4096), 8),
    ((1528, 1280, 4096), 8)]
