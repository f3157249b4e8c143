"""GPU operators with autograd, built on the ``torch.ops.pz`` HIP kernels.

This is the *autograd path* used by :class:`..models.layers.Layer` ``forward`` on GPU tensors
(``compute_output``, ``_forward`` + ``backward`` exactly as the reference calls them). The
throughput path (:mod:`..engine`) calls the same kernels with its own explicit schedule.

Every function here requires the native library; a missing ``_pz_C.so`` raises instead of
falling back to ATen (see :mod:`.native`).
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import native

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
ACT_CODES = {"relu": ACT_RELU, "sigmoid": ACT_SIGMOID, "tanh": ACT_TANH, None: ACT_NONE, "none": ACT_NONE}
EPI_STORE, EPI_FWD, EPI_BWD = 0, 1, 2
SAT_CODES = {"abs_gt": 1, "le": 2, "row_norm_gt": 3, "row_max_gt": 4}


def _ops():
    native.require()
    return torch.ops.pz


# --------------------------------------------------------------------------------------------
# epilogue specs
# --------------------------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def mix32(x: int) -> int:
    """The kernels' 32-bit integer finaliser ("lowbias32"), host side."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def layer_key(seed: tuple[int, int], lid: int) -> int:
    """Per-(seed, layer) dropout key: the mask bit of element pair j is ``mix32(j ^ key)``."""
    return mix32((seed[0] & _M32) ^ mix32((seed[1] + 0x9E3779B9 * (lid + 1)) & _M32))


def epoch_key(key: int, epoch: int) -> int:
    """Per-epoch variant of a (seed, layer) key — the kernels' ``epoch_key`` (pz_common.h)."""
    return mix32((key & _M32) ^ mix32((epoch * 0x9E3779B1 + 0x7F4A7C15) & _M32))


def epi_spec(act: int = ACT_NONE, drop_pre: int = -1, drop_post: int = -1, p: float = 0.0,
             seed: tuple[int, int] = (0, 0), epoch: int | None = None,
             epoch_ptr: int = 0) -> tuple[list[int], list[float]]:
    """Pack a stage epilogue ``drop_post(act(drop_pre(x)))`` for the kernels.

    ``drop_pre`` / ``drop_post`` are the reference layer indices whose dropout is applied (-1 =
    none). Dropout keeps an element iff its 16-bit counter-hash draw is ``>= round(p * 65536)``;
    kept elements are scaled by ``1/(1-p)`` like ``torch.nn.functional.dropout``.

    Training steps vary the masks per epoch: eagerly launched steps pass ``epoch`` (mixed in
    here), graph-replayed steps pass ``epoch_ptr`` = the device address of the trainer's int32
    epoch counter, and the kernels mix ``*epoch_ptr`` in with the same function.
    """
    if p <= 0.0:
        drop_pre = drop_post = -1
    drop_all = 1 if p >= 1.0 else 0
    thresh = min(65536, int(round(p * 65536)))
    scale = 0.0 if drop_all else 1.0 / (1.0 - p)
    inv_scale = 1.0 - p
    kpre = layer_key(seed, drop_pre) if drop_pre >= 0 else 0
    kpost = layer_key(seed, drop_post) if drop_post >= 0 else 0
    if epoch is not None:
        kpre = epoch_key(kpre, epoch) if drop_pre >= 0 else 0
        kpost = epoch_key(kpost, epoch) if drop_post >= 0 else 0
    return ([act, int(drop_pre >= 0), int(drop_post >= 0), kpre, kpost, thresh, drop_all, int(epoch_ptr)],
            [scale, inv_scale])


def new_seed() -> tuple[int, int]:
    """Fresh dropout seed drawn from torch's CPU generator (so ``torch.manual_seed`` controls it)."""
    s = torch.randint(0, 2 ** 62, (1,)).item()
    return s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF


NO_EPI = epi_spec()


# --------------------------------------------------------------------------------------------
# GEMM front-end
# --------------------------------------------------------------------------------------------
def gemm(a: Tensor, a_kc: bool, b: Tensor, b_kc: bool, out: Tensor, *, bias: Tensor | None = None,
         aux: Tensor | None = None, colsum: Tensor | None = None, mode: int = EPI_STORE,
         epi: tuple[list[int], list[float]] = NO_EPI, alpha: float = 1.0, accumulate: bool = False,
         idx_ld: int = 0, force_generic: bool = False, mask: Tensor | None = None,
         scale_a: Tensor | None = None, scale_b: Tensor | None = None, out8: Tensor | None = None,
         out8_qscale: Tensor | None = None, amax: Tensor | None = None, no_split: bool = False,
         store_c: bool = True, engine: int = 0, cus: int = 0) -> Tensor:
    """``out[M,N] = op(a) @ op(b)`` with a fused epilogue.

    ``a_kc``: ``a`` is stored ``[M,K]`` (else ``[K,M]``); ``b_kc``: ``b`` is stored ``[N,K]`` (else ``[K,N]``).
    ``mask`` (uint8 :func:`relu_mask_shape` ``(M, N)``, tile-blocked, MFMA shapes only): EPI_FWD writes the bitmask
    ``y > 0`` of the final output; EPI_BWD with a ReLU stage reads it instead of ``aux``.
    fp8: ``a``/``b`` may be ``float8_e4m3fn`` (both K-contiguous); products are multiplied by the
    device scalars ``scale_a * scale_b``. ``out8`` (e4m3, EPI_FWD) receives ``sat(y * out8_qscale)``
    and ``amax`` (fp32 scalar, caller-zeroed) the running ``max |y|``. ``no_split`` turns the
    split-K plan of a skinny shape off (a GEMM running beside others on its own stream).
    ``store_c=False`` (MFMA path, bf16 ``out``): only the side outputs — ``out8``, ``mask``,
    ``colsum`` — are written, ``out`` is not (the fp8 policy's bf16 tensors nobody reads).
    ``engine``: 0 = the default choice, 1 = the tiled kernels (gemm_mfma.hip), 2 = the persistent
    stream-K engine (gemm_sk.hip; raises if the shape is not eligible), 3 = that engine on its
    4-wave lab main loop (plain stores only); ``cus`` = the CU budget of
    the persistent engine (0 = every CU).
    """
    M, N = out.shape
    K = a.shape[1] if a_kc else a.shape[0]
    _ops().gemm(a, a_kc, b, b_kc, out, bias, aux, colsum, mode, epi[0], epi[1], alpha, accumulate,
                M, N, K, idx_ld, force_generic, mask, scale_a, scale_b, out8, out8_qscale, amax,
                (1 if no_split else 0) | (0 if store_c else 2) | ((engine & 3) << 2) | ((cus & 0xFFFF) << 16))
    return out


def gemm_pair(a0: Tensor, b0: Tensor, out0: Tensor, a1: Tensor, b1: Tensor, out1: Tensor, *,
              scales0: tuple = (None, None), scales1: tuple = (None, None), engine: int = 0, cus: int = 0) -> None:
    """Two weight-gradient GEMMs ``out_i = a_iᵀ @ b_i`` (``a_i`` stored ``[K, M_i]``, ``b_i``
    ``[K, N_i]``, one K) in ONE launch (``pz::gemm_pair``); fp8 operands take their
    ``(scale_a, scale_b)`` dequantisation scalars. Check :func:`gemm_pair_split` first.
    ``engine=2`` (bf16): both problems' tiles as one persistent stream-K schedule on ``cus`` CUs."""
    K = a0.shape[0]
    _ops().gemm_pair(a0, b0, out0, a1, b1, out1, out0.shape[0], out0.shape[1], out1.shape[0], out1.shape[1], K,
                     scales0[0], scales0[1], scales1[0], scales1[1], ((engine & 3) << 2) | ((cus & 0xFFFF) << 16))


def gemm_pair_split(a0: Tensor, b0: Tensor, out0: Tensor, a1: Tensor, b1: Tensor, out1: Tensor, engine: int = 0) -> int:
    """Split-K factor the pair would run with, 0 when the two GEMMs cannot share a launch
    (``engine=2``: or when the persistent stream-K engine cannot run both)."""
    if a0.shape[0] != a1.shape[0]:
        return 0
    return int(_ops().gemm_pair_split(a0, b0, out0, a1, b1, out1, out0.shape[0], out0.shape[1], out1.shape[0],
                                      out1.shape[1], a0.shape[0], engine))


def gemm_sk_plan(M: int, N: int, K: int, cus: int = 0, M1: int = 0, N1: int = 0) -> tuple[int, int, int, int]:
    """``(grid, sk_tiles, iters, tiles)`` of the schedule the persistent stream-K engine (``engine=2``)
    runs an ``[M, N]`` GEMM of depth ``K`` with on a budget of ``cus`` CUs (0 = every CU), as the
    launcher's own ``pz::sk_plan`` reports it on this device (nothing is launched); ``M1, N1``: a
    second problem of the same ``K`` sharing the launch (:func:`gemm_pair`). ``grid`` workgroups walk
    ``tiles`` 256 x 256 tiles of ``iters`` 64-deep K steps; tiles ``[0, sk_tiles)`` are cut along K over
    all workgroups (at most two contributors each), the others run whole, ``grid`` at a time."""
    return tuple(_ops().gemm_sk_plan(M, N, K, cus, M1, N1))


def relu_mask_shape(m: int, n: int) -> tuple[int, int]:
    """Shape of the tile-blocked ReLU bitmask of an ``[m, n]`` output (csrc/pz_launch.h
    GemmArgs::mask): 256 x 256 element blocks of 8 KiB (256 rows of 32 B) in block-row-major order,
    held as a uint8 ``[roundup(m, 256), 32 * ceil(n / 256)]`` tensor."""
    return (m + 255) // 256 * 256, (n + 255) // 256 * 32


def relu_mask_empty(m: int, n: int, device=None) -> Tensor:
    return torch.empty(relu_mask_shape(m, n), device=device, dtype=torch.uint8)


def relu_mask_bits(mask: Tensor, m: int, n: int) -> Tensor:
    """Unpack a tile-blocked ReLU bitmask into a bool ``[m, n]`` (bit ``n & 7`` of each byte)."""
    rows, ld = mask.shape
    tn = ld // 32
    rowmajor = mask.reshape(rows // 256, tn, 256, 32).permute(0, 2, 1, 3).reshape(rows, ld)
    bits = (rowmajor.unsqueeze(-1).int() >> torch.arange(8, device=mask.device, dtype=torch.int32)) & 1
    return bits.reshape(rows, ld * 8)[:m, :n].bool()


def relu_mask_pack(y_pos: Tensor) -> Tensor:
    """The tile-blocked bitmask of a bool ``[m, n]`` (inverse of :func:`relu_mask_bits`)."""
    m, n = y_pos.shape
    rows, ld = relu_mask_shape(m, n)
    full = torch.zeros(rows, ld * 8, device=y_pos.device, dtype=torch.int32)
    full[:m, :n] = y_pos.int()
    rowmajor = (full.reshape(rows, ld, 8) << torch.arange(8, device=y_pos.device, dtype=torch.int32)).sum(-1)
    blocked = rowmajor.to(torch.uint8).reshape(rows // 256, 256, ld // 32, 32).permute(0, 2, 1, 3)
    return blocked.contiguous().reshape(rows, ld)


def gemm_path(a: Tensor, a_kc: bool, b: Tensor, b_kc: bool, out: Tensor, force_generic: bool = False) -> str:
    """The kernel family :func:`gemm` would dispatch these operands to, without launching anything."""
    M, N = out.shape
    K = a.shape[1] if a_kc else a.shape[0]
    path = _ops().gemm_path(a, a_kc, b, b_kc, out, M, N, K, force_generic)
    return {1: "mfma", 2: "mfma_wide"}.get(path, "generic")  # mfma_wide: fp32 / fp64 matrix cores


def gemm_last_kernel() -> str:
    """The GEMM kernel the calling thread launched last, recorded by the launcher itself (unlike
    :func:`gemm_path`, which predicts): ``"family/varV/BMxBN/ekE/splitS"``, e.g.
    ``"w4/var40/256x256/ek3/split1"``. ``family`` is ``generic`` (VALU tile), ``wide`` (fp32 / fp64
    matrix cores), ``mfma`` (the tiled bf16 / fp8 kernels), ``w4`` (the 4-wave LDS-DMA schedule),
    ``sk`` (stream-K) or ``pair`` (``gemm_pair``), ``none`` before the first launch; ``V`` the kernel
    variant (0 where the family has none); ``BMxBN`` the output tile; ``E`` the epilogue kind (0 any,
    1 plain store, 2 ReLU stage, 3 ReLU-bitmask backward, 4-6 the fixed dropout stages; always 0 for
    ``generic`` / ``wide``); ``S`` the split-K factor (1 = none)."""
    return _ops().gemm_last_kernel()


SKINNY_MAX_ROWS = 16


def gemm_skinny_eligible(x: Tensor, w: Tensor, out: Tensor) -> bool:
    """Whether :func:`gemm_skinny` takes these operands: GPU tensors, ``x [M, K]`` and ``w [K, N]``
    of one dtype (bf16 / fp32), ``1 <= M <= 16``, ``out [M, N]`` bf16 / fp32, unit inner strides,
    ``w``'s row bytes and leading dimension multiples of 16 B and its base 16-B aligned."""
    if not (x.is_cuda and w.is_cuda and out.is_cuda) or x.dim() != 2 or w.dim() != 2 or out.dim() != 2:
        return False
    if x.dtype != w.dtype or x.shape[1] != w.shape[0] or out.shape != (x.shape[0], w.shape[1]):
        return False
    return bool(_ops().gemm_skinny_eligible(x, w, out))


def gemm_skinny(x: Tensor, w: Tensor, out: Tensor, *, bias: Tensor | None = None, act: int = ACT_NONE) -> Tensor:
    """``out[M,N] = act(x[M,K] @ w[K,N] + bias)`` for ``1 <= M <= 16``: the forward-only weight-
    streaming kernel of the inference path (csrc/gemm_skinny.hip). ``w`` in the layers' ``[in, out]``
    layout, fp32 ``bias``, fp32 accumulation in a fixed order (bit-reproducible, and a row's result
    does not depend on the rows sent with it). Operands that are not
    :func:`gemm_skinny_eligible` raise; nothing is launched for them."""
    _ops().gemm_skinny(x, w, out, bias, act)
    return out


def gemm_skinny_plan(K: int, N: int, dtype: torch.dtype) -> tuple[int, int, int]:
    """``(strips, slices, slice_len)`` that :func:`gemm_skinny` runs a ``[K, N]`` weight matrix of
    ``dtype`` (bf16 / fp32) with, as the launcher's own ``pz::skinny_plan`` reports it (nothing is
    launched): the grid is ``strips x slices`` workgroups, each summing ``slice_len`` K rows (the
    last slice whatever is left). Never a function of M."""
    code = {torch.bfloat16: 0, torch.float32: 1}.get(dtype)
    if code is None:
        raise ValueError(f"gemm_skinny_plan: bf16 / fp32 operands only, got {dtype}")
    return tuple(_ops().gemm_skinny_plan(K, N, code))


# --------------------------------------------------------------------------------------------
# weight-only e4m3 inference: column quantiser and its skinny GEMM
# --------------------------------------------------------------------------------------------
E4M3_MAX = 448.0


def _check_quantisable(w: Tensor) -> None:
    if w.dim() != 2 or w.dtype != torch.float32:
        raise ValueError(f"quantize_cols takes a 2-D float32 [in, out] weight matrix, got {tuple(w.shape)} {w.dtype}")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_cols: the weight matrix holds a non-finite value; nothing was quantised")


def quantize_cols_reference(w: Tensor) -> tuple[Tensor, Tensor]:
    """Pure-torch definition of :func:`quantize_cols` (runs on the CPU): ``w [K, N]`` fp32 ->
    ``(w8, scale)`` with ``w8`` a ``float8_e4m3fn`` ``[K, N]`` tensor and ``scale [N]`` fp32 powers of two.

    Per column, ``amax = max_k |w[k, n]| = m * 2^x`` with ``m`` in ``[0.5, 1)`` (frexp);
    ``e = x - 9`` if ``m <= 0.875`` else ``x - 8`` — the smallest ``e`` with ``amax <= 448 * 2^e`` —
    but not below -126 (the scale stays a normal fp32; only ``amax < 2^-118`` meets that floor);
    ``scale = 2^e``, 1 for an all-zero column; ``w8 = e4m3_rne(clamp(w * 2^-e, -448, 448))``.
    The multiply is exact, so ``w8.float() * scale`` is exactly representable in bf16."""
    _check_quantisable(w)
    amax = w.abs().amax(dim=0) if w.shape[0] else torch.zeros(w.shape[1], dtype=torch.float32, device=w.device)
    m, x = torch.frexp(amax)
    e = (x - 9 + (m > 0.875).to(x.dtype)).clamp(min=-126)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    one = torch.ones_like(amax)
    scale = torch.ldexp(one, e)
    w8 = (w * torch.ldexp(one, -e)).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return w8, scale


def quantize_cols(w: Tensor) -> tuple[Tensor, Tensor]:
    """``w [K, N]`` fp32 on the GPU (unit inner stride, any row stride) -> ``(w8, scale)`` exactly as
    :func:`quantize_cols_reference` defines them, by the two-phase kernel of csrc/quant_cols.hip.
    ``w8`` is a contiguous ``float8_e4m3fn`` tensor in ``w``'s ``[in, out]`` layout. A non-finite
    weight raises ``ValueError`` (one ``isfinite`` check on the host side); nothing is quantised."""
    if not w.is_cuda:
        raise ValueError("quantize_cols takes a GPU tensor (quantize_cols_reference runs on the CPU)")
    _check_quantisable(w)
    ops = _ops()
    if w.shape[1] > 1 and w.stride(1) != 1:
        w = w.contiguous()
    k, n = w.shape
    w8 = torch.empty(k, n, device=w.device, dtype=torch.float8_e4m3fn)
    scale = torch.ones(n, device=w.device, dtype=torch.float32)
    if k and n:
        ops.quantize_cols(w, w8, scale, torch.zeros(n, device=w.device, dtype=torch.float32))
    return w8, scale


def dequantize_cols(w8: Tensor, scale: Tensor, dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """``w8.float() * scale`` — exact in fp32 and, the scales being powers of two, in bf16."""
    return (w8.float() * scale).to(dtype)


def gemm_skinny_w8_eligible(x: Tensor, w8: Tensor, scale: Tensor, out: Tensor) -> bool:
    """Whether :func:`gemm_skinny_w8` takes these operands: GPU tensors, bf16 ``x [M, K]``,
    ``float8_e4m3fn`` ``w8 [K, N]``, fp32 ``scale [N]``, ``1 <= M <= 16``, ``out [M, N]`` bf16 / fp32,
    unit inner strides, ``w8``'s row bytes (= N) and leading dimension multiples of 16 and its base
    16-B aligned."""
    if not (x.is_cuda and w8.is_cuda and scale.is_cuda and out.is_cuda) or x.dim() != 2 or w8.dim() != 2 or out.dim() != 2:
        return False
    if w8.dtype != torch.float8_e4m3fn or x.shape[1] != w8.shape[0] or out.shape != (x.shape[0], w8.shape[1]):
        return False
    if scale.dtype != torch.float32 or scale.dim() != 1 or scale.shape[0] != w8.shape[1] or not scale.is_contiguous():
        return False
    return bool(_ops().gemm_skinny_w8_eligible(x, w8, scale, out))


def gemm_skinny_w8(x: Tensor, w8: Tensor, scale: Tensor, out: Tensor, *, bias: Tensor | None = None,
                   act: int = ACT_NONE) -> Tensor:
    """``out[M,N] = act(scale[n] * (x[M,K] @ w8[K,N]) + bias[n])`` for ``1 <= M <= 16``: the weight-only
    quantised sibling of :func:`gemm_skinny` (csrc/gemm_skinny_w8.hip). ``x`` bf16, ``w8`` a
    ``torch.float8_e4m3fn`` tensor in the ``[in, out]`` layout with one power-of-two ``scale`` per
    column (:func:`quantize_cols`), fp32 ``bias``, fp32 accumulation in a fixed order
    (bit-reproducible; a row's result does not depend on the rows sent with it). Products and the
    scale multiply are exact, so this computes ``gemm_skinny`` on the dequantised bf16 matrix up to
    summation order. A ``scale`` / ``bias`` whose length is not N, or a ``w8`` of another dtype, is a
    structural error; operands that are not :func:`gemm_skinny_w8_eligible` raise; nothing is
    launched for either."""
    _ops().gemm_skinny_w8(x, w8, scale, out, bias, act)
    return out


def gemm_skinny_w8_plan(K: int, N: int) -> tuple[int, int, int]:
    """``(strips, slices, slice_len)`` that :func:`gemm_skinny_w8` runs a ``[K, N]`` e4m3 matrix with,
    as the launcher's own ``pz::skinny_w8_plan`` reports it (see :func:`gemm_skinny_plan`)."""
    return tuple(_ops().gemm_skinny_w8_plan(K, N))


def _as_2d(x: Tensor) -> tuple[Tensor, tuple]:
    lead = x.shape[:-1]
    return x.reshape(-1, x.shape[-1]).contiguous(), lead


# --------------------------------------------------------------------------------------------
# Linear
# --------------------------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, b: Tensor | None):
        squeeze = x.dim() == 1
        x2, lead = _as_2d(x.unsqueeze(0) if squeeze else x)
        wc = w if w.dtype == x2.dtype else w.to(x2.dtype)
        wc = wc.contiguous()
        out = torch.empty(x2.shape[0], wc.shape[1], device=x.device, dtype=x2.dtype)
        bias_k = None
        if b is not None:  # fp64 models add the fp64 bias (the kernels take fp32 or fp64)
            bias_k = b.detach().to(torch.float64 if x2.dtype == torch.float64 else torch.float32).contiguous()
        gemm(x2, True, wc, False, out, bias=bias_k)
        ctx.save_for_backward(x2, wc)
        ctx.has_bias = b is not None
        ctx.w_dtype = w.dtype
        ctx.b_dtype = b.dtype if b is not None else None
        out = out.view(*lead, wc.shape[1])
        return out.squeeze(0) if squeeze else out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        x2, wc = ctx.saved_tensors
        g2 = grad_out.reshape(-1, wc.shape[1]).to(x2.dtype).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x2)
            gemm(g2, True, wc, True, gx)  # dX = dY @ W^T, W stored [in,out] = [N,K]
            gx = gx.view(*grad_out.shape[:-1], wc.shape[0])
        if ctx.needs_input_grad[1]:
            acc_dtype = torch.float64 if x2.dtype == torch.float64 else torch.float32
            gw = torch.empty(wc.shape, device=wc.device, dtype=acc_dtype)
            gemm(x2, False, g2, False, gw)  # dW = X^T @ dY (K = batch)
            gw = gw.to(ctx.w_dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            acc = torch.float64 if x2.dtype == torch.float64 else torch.float32  # fp64 models stay fp64
            gb = torch.zeros(wc.shape[1], device=wc.device, dtype=acc)
            _ops().colsum(g2, gb)
            gb = gb.to(ctx.b_dtype)
        return gx, gw, gb


def linear(x: Tensor, w: Tensor, b: Tensor | None) -> Tensor:
    return _Linear.apply(x, w, b)


# --------------------------------------------------------------------------------------------
# activations / dropout (stage epilogue kernels)
# --------------------------------------------------------------------------------------------
class _Stage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, ei: list, ef: list):
        xc = x.contiguous()
        y = torch.empty_like(xc)
        _ops().stage_fwd(xc, y, ei, ef)
        ctx.save_for_backward(y)
        ctx.ei, ctx.ef = ei, ef
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        (y,) = ctx.saved_tensors
        gc = g.contiguous().to(y.dtype)
        dx = torch.empty_like(y)
        _ops().stage_bwd(gc, y, dx, ctx.ei, ctx.ef)
        return dx, None, None


def activation(x: Tensor, algo: str) -> Tensor:
    ei, ef = epi_spec(act=ACT_CODES[algo])
    return _Stage.apply(x, ei, ef)


def dropout(x: Tensor, p: float) -> Tensor:
    if p <= 0.0:
        return x
    ei, ef = epi_spec(drop_pre=0, p=p, seed=new_seed())
    return _Stage.apply(x, ei, ef)


# --------------------------------------------------------------------------------------------
# softmax / losses
# --------------------------------------------------------------------------------------------
class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor):
        xc = x.contiguous()
        y = torch.empty_like(xc)
        _ops().softmax_rows(xc, y)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        _ops().softmax_bwd(g.contiguous().to(y.dtype), y, dx)
        return dx


def softmax(x: Tensor) -> Tensor:
    return _Softmax.apply(x)


# --------------------------------------------------------------------------------------------
# token sampling (csrc/sample.hip)
# --------------------------------------------------------------------------------------------
def sample_uniform(seed: tuple[int, int], row: int, step: int) -> float:
    """The uniform in ``[0, 1)`` that row ``row`` draws at generation step ``step``: 24 bits of
    ``mix32(row ^ layer_key(seed, step))`` — integer arithmetic, so exactly the kernel's value."""
    return (mix32((row & _M32) ^ layer_key(seed, step)) >> 8) * 2.0 ** -24


def _sample_uniforms(seed: tuple[int, int], rows: int, step: int, row0: int, device) -> Tensor:
    """:func:`sample_uniform` of rows ``row0 .. row0 + rows - 1`` as an fp64 tensor (the same integers)."""
    x = ((torch.arange(rows, dtype=torch.int64, device=device) + row0) & _M32) ^ layer_key(seed, step)
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32  # (wraps int64; the low 32 bits of the product are exact)
    x = x ^ (x >> 16)
    return (x >> 8).double() * 2.0 ** -24


def _check_nucleus(top_p: float | None, min_p: float | None) -> tuple[float, float]:
    """``(top_p, min_p)`` with the off values ``1.0`` / ``0.0`` for ``None``; ValueError outside
    ``(0, 1]`` / ``[0, 1)`` (NaN included)."""
    if top_p is not None and not 0 < top_p <= 1:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if min_p is not None and not 0 <= min_p < 1:
        raise ValueError(f"min_p must be in [0, 1), got {min_p}")
    return (1.0 if top_p is None else float(top_p)), (0.0 if min_p is None else float(min_p))


def sample_rows_reference(logits: Tensor, seed: tuple[int, int], step: int, temperature: float = 1.0,
                          top_k: int | None = None, row0: int = 0, top_p: float | None = None,
                          min_p: float | None = None) -> Tensor:
    """The sampling rule of :func:`sample_rows` in pure torch, in fp64, on CPU or GPU tensors:
    ``logits [rows, V]`` (or ``[V]``) -> int64 tokens ``[rows]``. It is the sampler of the runtimes
    without the kernel and the yardstick of the kernel's tests.

    * top-k: keep the columns whose logit is ``>=`` the k-th largest of the row (ties all stay);
      ``None`` / ``0`` / ``k >= V`` keep everything;
    * ``temperature == 0``: the lowest index among the maxima, nothing drawn, whatever the options;
    * ``w_c = exp((l_c - max) / T)`` (``T`` rounded to fp32, as the kernel receives it);
    * min-p (``0 < min_p < 1``; ``None`` / ``0`` is off) then drops the kept columns with
      ``w_c < min_p`` — the maximum has ``w = 1`` and stays;
    * top-p (``0 < top_p < 1``; ``None`` / ``1`` is off) then keeps, of what is left with mass ``S0``,
      the columns whose strictly-more-likely columns hold less than ``top_p * S0``: the smallest set
      of most likely columns whose mass reaches ``top_p * S0``, with every column tied with the last
      one admitted; the most likely column always stays;
    * the draw: ``u = sample_uniform(seed, row0 + row, step)``, and the token is the smallest
      kept ``c`` whose inclusive prefix sum of ``w`` exceeds ``u * sum(w)`` — the last kept column if
      rounding leaves none."""
    if temperature != temperature or temperature < 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    if top_k is not None and top_k < 0:
        raise ValueError(f"top_k must be >= 0, got {top_k}")
    top_p, min_p = _check_nucleus(top_p, min_p)
    lg = logits.detach()
    lg = (lg.unsqueeze(0) if lg.dim() == 1 else lg.reshape(-1, lg.shape[-1])).double()
    rows, v = lg.shape
    idx = torch.arange(v, device=lg.device).expand(rows, v)
    mx = lg.max(dim=-1, keepdim=True).values
    if temperature == 0:
        return torch.where(lg == mx, idx, v).min(dim=-1).values
    kept = torch.ones_like(lg, dtype=torch.bool)
    if top_k and top_k < v:
        kept = lg >= torch.topk(lg, top_k, dim=-1).values[:, -1:]
    t32 = float(torch.tensor(temperature, dtype=torch.float32))
    w = torch.exp((lg - mx) / t32)
    if min_p > 0:
        kept = kept & ~(w < min_p)
    w = torch.where(kept, w, torch.zeros_like(lg))
    if top_p < 1:
        # mass of the kept columns with a strictly larger logit: the exclusive prefix of the weights in
        # descending logit order, read at the first column of each run of equal logits
        ls, order = lg.sort(dim=-1, descending=True, stable=True)
        ws = w.gather(1, order)
        excl = ws.cumsum(dim=-1) - ws
        first = torch.ones_like(kept)
        first[:, 1:] = ls[:, 1:] != ls[:, :-1]
        above = torch.where(first, excl, torch.zeros_like(excl)).cummax(dim=-1).values
        stay = above < top_p * ws.sum(dim=-1, keepdim=True)
        kept = kept & torch.zeros_like(kept).scatter(1, order, stay)
        w = torch.where(kept, w, torch.zeros_like(lg))
    cdf = w.cumsum(dim=-1)
    target = _sample_uniforms(seed, rows, step, row0, lg.device) * cdf[:, -1]
    first = torch.where(kept & (cdf > target.unsqueeze(1)), idx, v).min(dim=-1).values
    last_kept = torch.where(kept, idx, -1).max(dim=-1).values
    return torch.where(first < v, first, last_kept)


def nucleus_args(top_p: float | None, min_p: float | None) -> dict:
    """``top_p`` / ``min_p`` as keyword arguments, the set ones only: every layer from ``POST /generate/`` down to
    the operators passes them on this way, so a call without them reaches the layer below exactly as it did
    before they existed (an unset one keeps the operator schema's off value)."""
    return {k: float(v) for k, v in (("top_p", top_p), ("min_p", min_p)) if v is not None}


def sample_rows(logits: Tensor, seq: Tensor, done: Tensor, pos: int, *, seed: tuple[int, int], step: int,
                temperature: float = 1.0, top_k: int | None = None, stop_token: int | None = None,
                row0: int = 0, top_p: float | None = None, min_p: float | None = None) -> None:
    """One token per row of the fp32 ``logits [rows, V]`` into ``seq[:, pos]`` (int64 ``[rows, length]``),
    by the rule of :func:`sample_rows_reference` with ``u = sample_uniform(seed, row0 + row, step)``
    (csrc/sample.hip; one launch, nothing comes back to the host). ``done`` (int32 ``[rows]``): a row
    whose flag is set writes ``stop_token``; a row that draws ``stop_token`` sets its flag. The call is
    bit-reproducible and a row's token does not depend on the rows sent with it. The binding refuses a
    ``top_p`` outside ``(0, 1]`` and a ``min_p`` outside ``[0, 1)``."""
    _ops().sample_rows(logits, seq, done, pos, float(temperature), int(top_k or 0), layer_key(seed, step),
                       -1 if stop_token is None else int(stop_token), int(row0), **nucleus_args(top_p, min_p))


def generate_resident(seq: Tensor, done: Tensor, params: list[Tensor], plan: list[int], steps: int, *,
                      seed: tuple[int, int], temperature: float = 1.0, top_k: int | None = None,
                      stop_token: int | None = None, row0: int = 0, logits_out: Tensor | None = None,
                      top_p: float | None = None, min_p: float | None = None) -> None:
    """A whole generation request in one launch (csrc/generate_resident.hip): one workgroup per row of
    ``seq`` (int64 ``[rows, L + steps]``, the context in its first ``L`` columns) copies ``params`` into
    LDS as ``plan`` (:func:`..engine.resident.resident_plan`) lays them out, then per step runs the
    model on the last ``L`` ids and draws ``seq[:, L + s]`` by the rule and with the random numbers of
    :func:`sample_rows` at ``step=s``. ``logits_out`` (fp32 ``[rows, steps, V]``) receives each step's
    logits. The binding refuses a plan that does not fit the tensors or the device."""
    _ops().generate_resident(seq, done, list(params), [int(v) for v in plan], int(steps), float(temperature),
                             int(top_k or 0), int(seed[0]) & _M32, int(seed[1]) & _M32,
                             -1 if stop_token is None else int(stop_token), int(row0), logits_out,
                             **nucleus_args(top_p, min_p))


# --------------------------------------------------------------------------------------------
# sequence scoring (csrc/token_logprob.hip)
# --------------------------------------------------------------------------------------------
def token_logprob_reference(logits: Tensor, targets: Tensor) -> tuple[Tensor, Tensor]:
    """The rule of :func:`token_logprob` in pure torch, on CPU or GPU tensors: ``logits [rows, V]`` (or
    ``[V]``) of any float dtype and int ``targets [rows]`` -> ``(fp64 logprob [rows], int64 rank [rows])``.
    It is the scorer of the runtimes without the kernel and the yardstick of the kernel's tests.

    * ``logprob = log_softmax(logits.double())[target]``: a ``-inf`` target gives ``-inf``, ``-inf``
      columns contribute nothing;
    * ``rank = #{c : l_c > l_t} + #{c < t : l_c == l_t}``, compared in the logits' own dtype
      (``-0 == +0``): rank 0 is the column greedy sampling picks, the lowest index among the maxima;
    * a target outside ``[0, V)`` gives ``NaN`` / ``-1``."""
    lg = logits.detach()
    lg = lg.unsqueeze(0) if lg.dim() == 1 else lg.reshape(-1, lg.shape[-1])
    rows, v = lg.shape
    t = torch.as_tensor(targets).detach().reshape(-1).to(device=lg.device, dtype=torch.int64)
    if t.shape[0] != rows:
        raise ValueError(f"targets must hold one id per row of the logits: {t.shape[0]} ids, {rows} rows")
    if v < 1:
        raise ValueError("logits must have at least one column")
    valid = (t >= 0) & (t < v)
    tc = t.clamp(0, v - 1).unsqueeze(1)
    logprob = torch.log_softmax(lg.double(), dim=-1).gather(1, tc).squeeze(1)
    lt = lg.gather(1, tc)
    before = torch.arange(v, device=lg.device).unsqueeze(0) < tc
    rank = ((lg > lt) | ((lg == lt) & before)).sum(dim=-1)
    return (torch.where(valid, logprob, torch.full_like(logprob, math.nan)),
            torch.where(valid, rank, torch.full_like(rank, -1)))


def token_logprob(logits: Tensor, targets: Tensor, logprob: Tensor | None = None,
                  rank: Tensor | None = None) -> tuple[Tensor, Tensor | None]:
    """Per row of the fp32 ``logits [rows, V]`` (unit column stride, any row stride ``>= V``), the
    log-probability of ``targets[row]`` (int64 ``[rows]``, any stride) into ``logprob`` (fp32 ``[rows]``,
    any stride; allocated when ``None``) and, when ``rank`` (int32 ``[rows]``, any stride) is given, its
    rank by the rule of :func:`token_logprob_reference` (csrc/token_logprob.hip; one launch, nothing
    comes back to the host). Returns ``(logprob, rank)``; ``rank=None`` computes no rank and returns
    ``None`` for it. The call is bit-reproducible and a row's result does not depend on the rows sent
    with it. The binding refuses tensors of another dtype, device or length and a non-unit column
    stride; no rows is no launch."""
    if logprob is None:
        logprob = torch.empty(logits.shape[0], device=logits.device, dtype=torch.float32)
    _ops().token_logprob(logits, targets, logprob, rank)
    return logprob, rank


# --------------------------------------------------------------------------------------------
# top-k answers (csrc/topk_rows.hip)
# --------------------------------------------------------------------------------------------
TOPK_MAX = 64  # kTopkMaxK of csrc/pz_kernels.h


def check_topk(k, cols: int, what: str = "k") -> int:
    """``k`` as an int, or ValueError unless it is an integer (no boolean) in ``[1, min(cols, TOPK_MAX)]``."""
    if cols < 1:
        raise ValueError("logits must have at least one column")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(cols, TOPK_MAX):
        raise ValueError(f"{what} must be an integer in [1, min({cols}, {TOPK_MAX})] = [1, {min(cols, TOPK_MAX)}], got {k!r}")
    return k


def topk_rows_reference(logits: Tensor, k: int) -> tuple[Tensor, Tensor]:
    """The rule of :func:`topk_rows` in pure torch, on CPU or GPU tensors: ``logits [rows, V]`` (or ``[V]``)
    of any float dtype and ``1 <= k <= min(V, 64)`` -> ``(int64 idx [rows, k], fp64 logprob [rows, k])``.

    * ``idx[r, j]`` is the column whose rank by :func:`token_logprob_reference` is ``j``: descending logit,
      compared in the logits' own dtype (``-0 == +0``), equal logits in ascending column order — a stable
      descending sort, not ``torch.topk`` (whose tie order is unspecified);
    * ``logprob[r, j] = log_softmax(logits.double())[r, idx[r, j]]``; a ``-inf`` column that reaches the
      top k scores ``-inf``.

    ValueError for ``k`` outside ``[1, min(V, 64)]`` and for ``V < 1``."""
    lg = logits.detach()
    k = check_topk(k, lg.shape[-1] if lg.dim() else 0)
    lg = lg.unsqueeze(0) if lg.dim() == 1 else lg.reshape(-1, lg.shape[-1])
    idx = torch.sort(lg, dim=-1, descending=True, stable=True).indices[:, :k]
    return idx, torch.log_softmax(lg.double(), dim=-1).gather(1, idx)


def topk_rows(logits: Tensor, k: int, idx: Tensor | None = None, logprob: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """Per row of the fp32 ``logits [rows, V]`` (unit column stride, any row stride ``>= V``), the ``k``
    most likely columns in rank order into ``idx`` (int32 ``[rows, k]``) and their log-probabilities into
    ``logprob`` (fp32 ``[rows, k]``), by the rule of :func:`topk_rows_reference` (csrc/topk_rows.hip; one
    launch, nothing comes back to the host). Both outputs take a unit column stride and any row stride
    ``>= k`` and are allocated when ``None``. ``1 <= k <= min(V, 64)``. The call is bit-reproducible, a
    row's result does not depend on the rows sent with it, and ``logprob[:, j]`` has the bits of
    ``token_logprob(logits, idx[:, j])[0]``. The binding refuses tensors of another dtype, device or
    shape, other strides and other ``k``; no rows is no launch."""
    if idx is None:
        idx = torch.empty(logits.shape[0], int(k), device=logits.device, dtype=torch.int32)
    if logprob is None:
        logprob = torch.empty(logits.shape[0], int(k), device=logits.device, dtype=torch.float32)
    _ops().topk_rows(logits, int(k), idx, logprob)
    return idx, logprob


def check_index_range(idx: Tensor, lo: int, hi: int, what: str, size: int | None = None) -> None:
    """Raise IndexError (as ATen / Python indexing do) unless every id is in ``[lo, hi)``.
    The HIP kernels never read outside their tables either way, but a bad id must surface as an
    error, not as a silently wrong loss. A GPU tensor costs one small reduction + sync."""
    if idx.numel() == 0:
        return
    v = idx if idx.dtype == torch.int64 else idx.long()
    mn, mx = (int(t) for t in torch.aminmax(v))
    if mn < lo or mx >= hi:
        bad = mn if mn < lo else mx
        raise IndexError(f"{what} {bad} is out of bounds for size {hi if size is None else size}")


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: Tensor, labels: Tensor):
        squeeze = logits.dim() == 1
        l2 = (logits.unsqueeze(0) if squeeze else logits).contiguous()
        check_index_range(labels.reshape(-1), 0, l2.shape[-1], "Target")
        lab = labels.reshape(-1).to(device=l2.device, dtype=torch.int64).contiguous()
        rows = l2.shape[0]
        loss = torch.zeros(1, device=l2.device, dtype=torch.float64 if l2.dtype == torch.float64 else torch.float32)
        dh = torch.empty_like(l2)
        _ops().xent_head(l2, lab, rows, loss, 1.0 / rows, dh, 1.0 / rows, None, None, NO_EPI[0], NO_EPI[1], 0)
        ctx.save_for_backward(dh)
        ctx.squeeze = squeeze
        return loss.reshape(()).to(logits.dtype)

    @staticmethod
    def backward(ctx, g: Tensor):
        (dh,) = ctx.saved_tensors
        out = dh * g.to(dh.dtype)
        return (out.squeeze(0) if ctx.squeeze else out), None


def cross_entropy(logits: Tensor, labels: Tensor) -> Tensor:
    return _CrossEntropy.apply(logits, labels)


class _Mse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y: Tensor, target: Tensor):
        shape = y.shape
        y2 = y.reshape(-1, shape[-1] if y.dim() > 0 else 1).contiguous()
        t2 = target.to(y.dtype).reshape(y2.shape).contiguous()
        n = y2.numel()
        loss = torch.zeros(1, device=y.device, dtype=torch.float64 if y2.dtype == torch.float64 else torch.float32)
        dh = torch.empty_like(y2)
        _ops().mse_head(y2, t2, y2.shape[0], loss, 1.0 / n, dh, 1.0 / n, None, NO_EPI[0], NO_EPI[1], 0)
        ctx.save_for_backward(dh)
        ctx.shape = shape
        return loss.reshape(()).to(y.dtype)

    @staticmethod
    def backward(ctx, g: Tensor):
        (dh,) = ctx.saved_tensors
        return (dh * g.to(dh.dtype)).reshape(ctx.shape), None


def mse_loss(y: Tensor, target: Tensor) -> Tensor:
    return _Mse.apply(y, target)


# --------------------------------------------------------------------------------------------
# batchnorm / embedding
# --------------------------------------------------------------------------------------------
class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gain, bias, rmean, rvar, eps, momentum, training, sync):
        cols = x.shape[-1]
        xc = x.contiguous()
        y = torch.empty_like(xc)
        dev = x.device
        save_mean = torch.empty(cols, device=dev, dtype=torch.float64)
        save_inv = torch.empty(cols, device=dev, dtype=torch.float64)
        partial = torch.empty(2 * cols, device=dev, dtype=torch.float64)
        rows = xc.numel() // max(cols, 1)
        args = (xc, y, gain.detach().contiguous(), bias.detach().contiguous(), rmean, rvar, eps, momentum, training,
                rows, save_mean, save_inv, partial, NO_EPI[0], NO_EPI[1], 0)
        total = rows
        if sync is not None and training:  # synchronised statistics: sums -> all-reduce -> finalise
            _ops().batchnorm_fwd(*args, 1, 0)
            sync.all_reduce_(partial)
            total = int(sync.all_reduce_scalar(float(rows)))
            _ops().batchnorm_fwd(*args, 2, total)
        else:
            _ops().batchnorm_fwd(*args)
        ctx.save_for_backward(xc, y, gain, bias, save_mean, save_inv)
        ctx.rows = rows
        ctx.training = training
        ctx.sync = sync if training else None
        ctx.total = total
        return y

    @staticmethod
    def backward(ctx, g):
        xc, y, gain, bias, save_mean, save_inv = ctx.saved_tensors
        if not ctx.training:  # eval: y = gain * (x - mean) * invstd + bias
            gc = g.contiguous().to(xc.dtype)
            dx = gc * (gain.to(xc.dtype) * save_inv.to(xc.dtype))
            dgain = (gc * ((xc - save_mean.to(xc.dtype)) * save_inv.to(xc.dtype))).reshape(-1, xc.shape[-1]).sum(0)
            return dx, dgain.to(gain.dtype), gc.reshape(-1, xc.shape[-1]).sum(0).to(bias.dtype), None, None, None, \
                None, None, None
        dx = torch.empty_like(xc)
        dgain = torch.zeros_like(gain)
        dbias = torch.zeros_like(bias)
        partial = torch.empty(2 * xc.shape[-1], device=xc.device, dtype=torch.float64)
        args = (g.contiguous().to(xc.dtype), y, xc, dx, gain.detach().contiguous(), bias.detach().contiguous(),
                save_mean, save_inv, dgain, dbias, partial, ctx.rows, NO_EPI[0], NO_EPI[1], 0)
        if ctx.sync is not None:  # local parameter grads; dx from the global sums
            _ops().batchnorm_bwd(*args, 1, 0)
            ctx.sync.all_reduce_(partial)
            _ops().batchnorm_bwd(*args, 2, ctx.total)
        else:
            _ops().batchnorm_bwd(*args)
        return dx, dgain, dbias, None, None, None, None, None, None


def batchnorm(x: Tensor, gain: Tensor, bias: Tensor, rmean: Tensor, rvar: Tensor, eps: float, momentum: float,
              training: bool, sync=None) -> tuple[Tensor, Tensor, Tensor]:
    """Returns ``(y, running_mean, running_var)``; running stats are fresh tensors like the reference.
    ``sync``: a data-parallel context whose ranks share the batch statistics (synchronised BN)."""
    rm = rmean.detach().reshape(-1).to(gain.dtype).clone()
    rv = rvar.detach().reshape(-1).to(gain.dtype).clone()
    y = _BatchNorm.apply(x, gain, bias, rm, rv, float(eps), float(momentum), bool(training), sync)
    return y, rm, rv


class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx: Tensor, table: Tensor):
        vocab = table.shape[0]
        check_index_range(idx.reshape(-1), -vocab, vocab, "index", vocab)  # negative ids wrap (Python indexing)
        ids = idx.to(device=table.device, dtype=torch.int64).contiguous()
        out = torch.empty(*ids.shape, table.shape[1], device=table.device, dtype=table.dtype)
        _ops().embedding_fwd(table.detach().contiguous(), ids, out)
        ctx.save_for_backward(ids)
        ctx.table_shape = table.shape
        ctx.table_dtype = table.dtype
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        (ids,) = ctx.saved_tensors
        acc = torch.float64 if ctx.table_dtype == torch.float64 else torch.float32
        dtable = torch.zeros(ctx.table_shape, device=g.device, dtype=acc)
        _ops().embedding_bwd(g.contiguous(), ids, dtable)
        return None, dtable.to(ctx.table_dtype)


def embedding(idx: Tensor, table: Tensor) -> Tensor:
    return _Embedding.apply(idx, table)


# --------------------------------------------------------------------------------------------
# statistics (N7)
# --------------------------------------------------------------------------------------------
def tensor_summary(t: Tensor, algo: str | None, bins: int) -> dict:
    """mean / unbiased std / saturation / density histogram of a GPU tensor, one D2H copy."""
    from ..utils.stats import saturation_rule
    x = t.detach().contiguous()
    if x.dtype not in (torch.float32, torch.float64, torch.bfloat16):
        x = x.float()
    dev = x.device
    rule, thr = saturation_rule(algo) if algo is not None else ("abs_gt", 0.0)
    moments = torch.empty(8, device=dev, dtype=torch.float64)
    row_len = x.shape[-1] if x.dim() > 0 else 1
    _ops().tensor_moments(x, row_len, SAT_CODES[rule] if algo is not None else 0, thr, moments)
    counts = None
    if bins > 0:
        counts = torch.zeros(bins, device=dev, dtype=torch.int64)  # exact counts (u64 atomics)
        _ops().histogram(x, moments[:2], bins, counts)
    host = torch.cat([moments, counts.double()]) if counts is not None else moments
    host = host.cpu().tolist()
    n = x.numel()
    mn, mx, s, ss, sat = host[0], host[1], host[2], host[3], host[4]
    mean = s / n if n else math.nan
    var = (ss - s * s / n) / (n - 1) if n > 1 else math.nan
    out = {"mean": mean, "std": math.sqrt(var) if var == var and var > 0 else (0.0 if var == var else math.nan)}
    if algo is not None:
        rows = n // max(row_len, 1) if rule in ("row_norm_gt", "row_max_gt") else n
        out["saturated"] = sat / rows if rows else math.nan
    if bins > 0:
        lo, hi = mn, mx
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        width = (hi - lo) / bins
        c = host[8:8 + bins]
        total = sum(c)
        edges = [lo + i * width for i in range(bins)]
        dens = [v / (total * width) if total else 0.0 for v in c]
        out["histogram"] = {"x": edges, "y": dens}
    return out


__all__ = ["gemm", "gemm_path", "gemm_last_kernel", "gemm_skinny", "gemm_skinny_eligible", "gemm_skinny_w8", "gemm_skinny_w8_eligible",
           "gemm_skinny_plan", "gemm_skinny_w8_plan", "gemm_sk_plan",
           "quantize_cols", "quantize_cols_reference", "dequantize_cols", "linear", "activation", "dropout", "softmax", "cross_entropy", "mse_loss",
           "batchnorm", "embedding", "tensor_summary", "epi_spec", "new_seed", "sample_rows", "sample_rows_reference", "nucleus_args",
           "sample_uniform", "generate_resident", "token_logprob", "token_logprob_reference", "topk_rows", "topk_rows_reference",
           "check_topk", "TOPK_MAX"]
