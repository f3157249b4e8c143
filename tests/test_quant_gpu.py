"""pz::quantize_rows, quant_transpose, amax_abs and scale_update (csrc/quant.hip), raw ops, on every path.

Bytes. A finite value goes to the nearest fp8 code, ties to the even code, the sign of zero is kept and
everything past +-448 (e4m3) / +-57344 (e5m2), +inf included, saturates: `fp8_encode_reference` (built
from the code table, guarded on the CPU in test_kernel_refs_cpu.py) on the tie points, torch's CPU cast
of the clamped fp32 product x * q on random data. Equality is exact and covers every element; outputs
start as a sentinel byte and everything outside the written region must still hold it. NaN inputs are
out of scope (quant.hip's header states what happens to them).

Scales. q = maxval / (amax * headroom) costs at most two fp32 roundings and a division, 1 / q one more
division: each is held to 4 x 2^-24 relative of the fp64 value (a division that is not correctly
rounded would still fit). The MI355X shows more: q and 1 / q are bit-equal to the IEEE fp32 quotients
(measured |q - q64| / q64 <= 0.95 x 2^-24, |s q - 1| <= 0.93 x 2^-24), so the tests also require that
equality; where the quotient is exactly representable (amax a power of two) q is exact. The measured
errors are printed by the tests.

Kernels reached, by the launcher's conditions (quantize_rows_fmt: 8-wide needs cols % 8 == 0, ldx % 8 == 0,
ldo % 8 == 0, x 16-B and out 8-B aligned; quant_transpose: FULL needs K % 64 == N % 64 == 0, ldw % 4 == 0,
ldo % 16 == 0, both bases 16-B aligned):
  quantize_rows8_kernel<bf16|float, e4m3|e5m2>  test_codebook[wide-*], test_random[37x24, 37x520: contig, strided],
                                                test_grid_stride_sweeps[wide]; <*, e4m3> with amax_in: test_derived_scale
  quantize_rows_kernel<bf16|float, e4m3|e5m2>   test_codebook[scalar-*], test_random[37x12, 37x20: every layout;
                                                37x24, 37x520: misaligned-x, ldo4], test_grid_stride_sweeps[scalar]
  quant_transpose_kernel<true>                  test_quant_transpose[128x192: contig, strided-w, ldo16]
  quant_transpose_kernel<false>                 test_quant_transpose[128x192: ldo4; 100x70, 99x70, 1x1, 65x3]
  amax_kernel<float>, <uint16_t>                test_amax_abs
  scale_update_kernel                           test_scale_update
"""
import pytest
import torch

from tests.helpers import bit_equal, fp8_encode_reference, fp8_tie_points

pytestmark = pytest.mark.gpu
DEV = "cuda"

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
LIM = {E4: 448.0, E5: 57344.0}
NAME = {F32: "f32", BF16: "bf16", E4: "e4m3", E5: "e5m2"}
SENT = 0x55             # sentinel byte of the outputs (a finite code in both formats)
QBOUND = 4 * 2.0 ** -24  # relative bound of a derived q and of q * (1 / q), see the module docstring


def randn(shape, seed, dtype, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def cast_bytes(prod_f32: torch.Tensor, fmt) -> torch.Tensor:
    """torch's CPU cast of the clamped fp32 product, as bytes."""
    assert prod_f32.dtype == F32 and prod_f32.device.type == "cpu"
    return prod_f32.clamp(-LIM[fmt], LIM[fmt]).to(fmt).view(U8)


def sentinel(rows, cols, fmt):
    return torch.full((rows, cols), SENT, dtype=U8, device=DEV).view(fmt)


def assert_region(buf, ref, what):
    """`buf` (the whole fp8 output buffer) holds `ref` (uint8, CPU) in its top-left corner and the
    sentinel everywhere else."""
    want = torch.full(buf.shape, SENT, dtype=U8)
    want[:ref.shape[0], :ref.shape[1]] = ref
    got = buf.view(U8).cpu()
    bad = (got != want).sum().item()
    assert bad == 0, (what, f"{bad} bytes differ", (got != want).nonzero()[:5].tolist())


def assert_q(q, s, maxval, amax, what):
    """A derived pair {q, s} (fp32 tensors) against the IEEE fp32 quotients of the fp32 amax, and
    the distance from the fp64 quotient."""
    q32 = torch.tensor(maxval, dtype=F32) / amax.float().cpu()
    q64 = maxval / amax.double().item()
    eq, es = abs(q.item() - q64) / q64, abs(s.double().item() * q.double().item() - 1.0)
    print(f"{what}: |q - q64| / q64 = {eq:.3e} ({eq / 2.0 ** -24:.3f} x 2^-24), |s q - 1| = {es:.3e}, "
          f"q == fp32 quotient: {bit_equal(q.cpu().reshape(1), q32.reshape(1))}")
    assert eq <= QBOUND and es <= QBOUND, (what, eq, es)
    assert bit_equal(q.cpu().reshape(1), q32.reshape(1)), what
    assert bit_equal(s.cpu().reshape(1), (1.0 / q32).reshape(1)), what


# ------------------------------------------------------------------------------- 1. codebook
@pytest.mark.parametrize("scale", [1.0, 8.0], ids=["q1", "q1/8"])
@pytest.mark.parametrize("src", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("width", ["wide", "scalar"])
@pytest.mark.parametrize("fmt", [E4, E5], ids=["e4m3", "e5m2"])
def test_codebook(native_lib, fmt, width, src, scale):
    """Every code, every tie, both fp32 neighbours of every tie, subnormal, out-of-range and infinite
    points, both signs: x = point * scale, q = 1 / scale (powers of two: the product is the point)."""
    pts = fp8_tie_points(fmt)
    if src == BF16:
        pts = pts[pts.to(BF16).float() == pts]
        assert pts.numel() > 400  # every code and every tie of an fp8 format fits bf16's 8 bits
    cols = 24 if width == "wide" else 12
    rows = -(-pts.numel() // cols)
    flat = torch.zeros(rows * cols, dtype=F32)
    flat[:pts.numel()] = pts
    x = (flat * scale).to(src).view(rows, cols)
    assert torch.equal(x.float() * (1.0 / scale), flat.view(rows, cols))  # nothing lost on the way in
    ref = fp8_encode_reference(flat.double(), fmt).view(rows, cols)
    qs = torch.tensor([1.0 / scale, scale], device=DEV)
    out = sentinel(rows + 1, cols, fmt)
    torch.ops.pz.quantize_rows(x.to(DEV), out, qs, None)
    assert_region(out, ref, f"codebook {NAME[fmt]} {width} {NAME[src]}")
    assert qs.tolist() == [1.0 / scale, scale]


# ----------------------------------------------------------------- 2. random data, every kernel
def layouts(rows, cols, dtype, wide):
    """(name, x view on the GPU, out buffer) builders; the out buffer is always taller than x."""
    def contig(x):
        return x.to(DEV), (rows + 2, cols)

    def strided(x):          # x a column slice of a wider buffer at a 16-B aligned offset, out wider and taller
        buf = torch.full((rows, cols + 16), 99.0, dtype=dtype, device=DEV)
        buf[:, 8:8 + cols] = x.to(DEV)
        return buf[:, 8:8 + cols], (rows + 3, cols + 8)

    def misaligned_x(x):     # base 8 B past a 16-B boundary: the 8-wide loads are not possible
        off = 4 if dtype == BF16 else 2
        buf = torch.full((rows, cols + 16), 99.0, dtype=dtype, device=DEV)
        buf[:, off:off + cols] = x.to(DEV)
        return buf[:, off:off + cols], (rows + 3, cols + 8)

    def ldo4(x):             # ldo % 8 == 4: the 8-byte stores are not possible
        return x.to(DEV), (rows + 1, cols + 4)

    def odd_ldx(x):          # scalar shapes: any row stride of x
        buf = torch.full((rows, cols + 5), 99.0, dtype=dtype, device=DEV)
        buf[:, 3:3 + cols] = x.to(DEV)
        return buf[:, 3:3 + cols], (rows + 3, cols + 12)

    return [contig, strided, misaligned_x, ldo4] if wide else [contig, strided, odd_ldx, ldo4]


def run_quantize(x_dev, out_shape, fmt, q, preload):
    qs = torch.tensor([q, 123.0], device=DEV)
    amax = None if preload is None else torch.tensor([preload, -7.0], device=DEV)
    out = sentinel(*out_shape, fmt)
    torch.ops.pz.quantize_rows(x_dev, out, qs, None if amax is None else amax[:1])
    assert qs[1].item() == 123.0
    return out, qs[0].cpu(), amax


def check_quantize(x, fmt, amax_mode, builders, what):
    xf = x.float()
    top = xf.abs().max()
    q = LIM[fmt] / xf.abs().median().item()  # half the values saturate
    preload = {None: None, "below": 0.5 * top.item(), "above": 2.0 * top.item()}[amax_mode]
    first = None
    for build in builders:
        x_dev, out_shape = build(x)
        out, q0, amax = run_quantize(x_dev, out_shape, fmt, q, preload)
        ref = cast_bytes(xf * q0, fmt)
        sat = (ref & 0x7F).eq(0x7E if fmt == E4 else 0x7B).float().mean().item()
        assert 0.4 < sat < 0.6, sat
        assert_region(out, ref, f"{what} {build.__name__}")
        first = ref if first is None else first
        assert torch.equal(ref, first)  # every layout: the same bytes
        if amax is not None:
            want = torch.tensor([max(preload, top.item()), -7.0])
            assert bit_equal(amax.cpu(), want), (what, build.__name__, amax.tolist(), want.tolist())


@pytest.mark.parametrize("amax_mode", [None, "below", "above"], ids=["noamax", "amax-below", "amax-above"])
@pytest.mark.parametrize("fmt", [E4, E5], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,cols", [(37, 24), (37, 520), (37, 12), (37, 20)])
def test_random(native_lib, rows, cols, dtype, fmt, amax_mode):
    x = randn((rows, cols), 1000 + cols, dtype, 3.0)
    check_quantize(x, fmt, amax_mode, layouts(rows, cols, dtype, cols % 8 == 0), f"{rows}x{cols}")


@pytest.mark.parametrize("rows,cols,dtype,fmt", [(1032, 520, BF16, E5), (1100, 1004, F32, E4)], ids=["wide", "scalar"])
def test_grid_stride_sweeps(native_lib, rows, cols, dtype, fmt):
    """More work than one sweep of the grid (8-wide: 67080 groups over 66 blocks; scalar: 276100 words
    over 135 blocks), the largest |x| in the last element so that the last sweep reaches the amax. (The
    block caps of the launcher, 256 with an amax output, need over two million elements and are not reached.)"""
    x = randn((rows, cols), 7, dtype, 3.0)
    x[-1, -1] = -64.0
    check_quantize(x, fmt, "below", layouts(rows, cols, dtype, cols % 8 == 0)[:1], f"{rows}x{cols}")


# --------------------------------------------------------------------- 3. derived weight scale
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_derived_scale(native_lib, dtype):
    """amax_in + amax_clear: q = 448 / amax_in derived in the kernel, {q, 1/q} published, the other
    accumulator cleared, the bytes exact against the published q."""
    w = randn((64, 72), 3, dtype, 0.02)
    top = w.float().abs().max()
    amax_in = torch.tensor([top.item(), 5.0], device=DEV)
    clear = torch.tensor([3.0, 5.0], device=DEV)
    qs = torch.full((3,), 7.0, device=DEV)
    out = sentinel(66, 80, E4)
    torch.ops.pz.quantize_rows(w.to(DEV), out, qs, None, amax_in[:1], clear[:1])
    assert_q(qs[0], qs[1], 448.0, top, f"derived scale {NAME[dtype]}")
    assert qs[2].item() == 7.0 and clear.tolist() == [0.0, 5.0] and amax_in.tolist() == [top.item(), 5.0]
    assert_region(out, cast_bytes(w.float() * qs[0].cpu(), E4), "derived scale bytes")


def test_derived_scale_of_zero_amax_is_one(native_lib):
    w = randn((64, 72), 4, F32, 100.0)
    amax_in, clear, qs = torch.zeros(1, device=DEV), torch.ones(1, device=DEV), torch.full((2,), 7.0, device=DEV)
    out = sentinel(64, 72, E4)
    torch.ops.pz.quantize_rows(w.to(DEV), out, qs, None, amax_in, clear)
    assert qs.tolist() == [1.0, 1.0] and clear.item() == 0.0
    assert_region(out, cast_bytes(w, E4), "q = 1")


@pytest.mark.parametrize("case", ["scalar-shape", "e5m2", "no-clear"])
def test_derived_scale_refusals(native_lib, case):
    """What quant.hip refuses comes back as an error, nothing written."""
    cols = 12 if case == "scalar-shape" else 72
    fmt = E5 if case == "e5m2" else E4
    w = randn((64, cols), 5, F32).to(DEV)
    amax_in, clear, qs = torch.ones(1, device=DEV), torch.full((1,), 3.0, device=DEV), torch.full((2,), 7.0, device=DEV)
    out = sentinel(64, cols, fmt)
    with pytest.raises(RuntimeError):
        torch.ops.pz.quantize_rows(w, out, qs, None, amax_in, None if case == "no-clear" else clear)
    torch.cuda.synchronize()
    assert qs.tolist() == [7.0, 7.0] and clear.item() == 3.0 and (out.view(U8) == SENT).all()


# ------------------------------------------------------------------------- 4. quant_transpose
def transpose_layouts(K, N):
    """name -> (ldw, ldo): row strides of w [K, N] and out [N, K]; ldo % 4 == 0 is the op's contract."""
    k4 = -(-K // 4) * 4
    lay = {"contig": (N, k4), "strided-w": (N + 8, k4), "ldo16": (N, -(-K // 16) * 16 + 16), "ldo4": (N + 8, k4 + 4)}
    if K % 64 == 0:
        assert lay["ldo16"][1] % 16 == 0 and lay["ldo4"][1] % 16 == 4 and lay["contig"][1] == K
    return lay


@pytest.mark.parametrize("scale_from", ["amax", "qs"])
@pytest.mark.parametrize("K,N", [(128, 192), (100, 70), (99, 70), (1, 1), (65, 3)])
def test_quant_transpose(native_lib, K, N, scale_from):
    """fp32 W [K, N] -> e4m3 W^T [N, K], q derived from the amax record or taken from qs[0]; every
    layout gives the same bytes (128 x 192: contig, strided-w and ldo16 run FULL, ldo4 the ragged kernel)."""
    w = randn((K, N), 10 * K + N, F32, 0.05)
    top = w.abs().max()
    first = None
    for name, (ldw, ldo) in transpose_layouts(K, N).items():
        wbuf = torch.full((K, ldw), 99.0, device=DEV)
        wv = wbuf[:, ldw - N:]      # offset 0 or 8 floats: 16-B aligned
        wv.copy_(w)
        obuf = sentinel(N + 2, ldo, E4)
        out = obuf[:N, :K]
        clear = torch.tensor([3.0, 5.0], device=DEV)
        if scale_from == "amax":
            qs = torch.full((3,), 7.0, device=DEV)
            torch.ops.pz.quant_transpose(wv, out, qs, torch.tensor([top.item()], device=DEV), clear[:1])
            assert_q(qs[0], qs[1], 448.0, top, f"transpose {K}x{N} {name}")
            assert qs[2].item() == 7.0 and clear.tolist() == [0.0, 5.0]
        else:
            qs = torch.tensor([448.0 / (0.37 * top.item()), 7.0, 7.0], device=DEV)  # |w| > 0.37 max saturates
            torch.ops.pz.quant_transpose(wv, out, qs)
            assert qs[1:].tolist() == [7.0, 7.0] and clear.tolist() == [3.0, 5.0]
        ref = cast_bytes(w.t().contiguous() * qs[0].cpu(), E4)
        assert_region(obuf, ref, f"transpose {K}x{N} {name} {scale_from}")
        assert (wbuf[:, :ldw - N] == 99.0).all()
        first = ref if first is None else first
        assert torch.equal(ref, first)


def test_quant_transpose_zero_amax_and_missing_clear(native_lib):
    w = randn((65, 3), 6, F32, 100.0)
    obuf = sentinel(3, 68, E4)
    qs, clear = torch.full((2,), 7.0, device=DEV), torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError):
        torch.ops.pz.quant_transpose(w.to(DEV), obuf[:, :65], qs, torch.zeros(1, device=DEV))
    torch.cuda.synchronize()
    assert qs.tolist() == [7.0, 7.0] and (obuf.view(U8) == SENT).all()
    torch.ops.pz.quant_transpose(w.to(DEV), obuf[:, :65], qs, torch.zeros(1, device=DEV), clear)
    assert qs.tolist() == [1.0, 1.0] and clear.item() == 0.0
    assert_region(obuf, cast_bytes(w.t().contiguous(), E4), "transpose q = 1")


# -------------------------------------------------------------------------------- 5. amax_abs
# one sweep of the grid: grid_for(n / 4 + 1, 4096, 512) blocks x 256 lanes x 4 elements
def amax_sweep(n):
    return min(max(-(-(n // 4 + 1) // 4096), 1), 512) * 256 * 4


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 524288 + 3075])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_amax_abs(native_lib, dtype, n):
    """max |x| bit-equal to torch's, max-combined with what amax held, wherever the maximum lies:
    first and last element, the n % 4 tail loop, the second sweep of the grid-stride loop, a negative value."""
    base = randn((n,), n, dtype).to(DEV)
    plants = {"first": 0, "last": n - 1, "negative": n // 2}
    if n % 4 and n > 4:
        plants["tail"] = n // 4 * 4
    if n > amax_sweep(n) + 5:
        plants["second-sweep"] = amax_sweep(n) + 5
        assert plants["second-sweep"] < n // 4 * 4
    assert n != 524288 + 3075 or {"tail", "second-sweep"} <= set(plants)
    for name, pos in plants.items():
        x = base.clone()
        x[pos] = -100.0 if name == "negative" else 100.0
        ref = x.float().abs().max().cpu()
        assert ref.item() == 100.0
        for preload in (0.0, 1.0, 1000.0):
            amax = torch.tensor([preload, -7.0], device=DEV)
            torch.ops.pz.amax_abs(x, amax[:1])
            assert bit_equal(amax.cpu(), torch.tensor([max(preload, 100.0), -7.0])), (name, preload, amax.tolist())
    amax = torch.zeros(1, device=DEV)
    torch.ops.pz.amax_abs(base, amax)
    assert bit_equal(amax.cpu(), base.float().abs().max().cpu().reshape(1))  # no plant: an ordinary maximum
    x = base.clone()
    x[n - 1] = float("inf")
    torch.ops.pz.amax_abs(x, amax)
    assert amax.item() == float("inf")


def test_amax_abs_empty_and_misaligned(native_lib):
    amax = torch.tensor([2.5], device=DEV)
    for dtype in (F32, BF16):
        torch.ops.pz.amax_abs(torch.empty(0, dtype=dtype, device=DEV), amax)
        assert amax.item() == 2.5
        buf = torch.full((64,), 9.0, dtype=dtype, device=DEV)
        view = buf[2:34]  # 8 B (fp32) or 4 B (bf16) past the 16-B aligned base
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        with pytest.raises(RuntimeError):
            torch.ops.pz.amax_abs(view, amax)
        torch.cuda.synchronize()
        assert amax.item() == 2.5
    with pytest.raises(RuntimeError):  # no fp64 kernel
        torch.ops.pz.amax_abs(torch.ones(8, dtype=torch.float64, device=DEV), amax)
    assert amax.item() == 2.5


# ---------------------------------------------------------------------------- 6. scale_update
@pytest.mark.parametrize("reset", [True, False], ids=["reset", "keep"])
@pytest.mark.parametrize("maxval", [448.0, 57344.0])
@pytest.mark.parametrize("headroom", [1.0, 2.0])
def test_scale_update(native_lib, headroom, maxval, reset):
    n, pad = 130, 6  # three 64-lane blocks
    g = torch.Generator(device="cpu").manual_seed(11)
    a = torch.rand(n + pad, generator=g) * 10 + 1e-3
    a[::7] = 0.0                                                  # nothing recorded: keep the pair
    a[3::7] = 2.0 ** torch.arange(-8, 11)[:len(a[3::7])].float()  # exact quotients
    assert (a[:n] == 0).sum() > 10 and a[64] > 0 and a[129] > 0
    prev = torch.arange(2 * n + pad, dtype=F32) + 0.25
    amax, qs = a.clone().to(DEV), prev.clone().to(DEV)
    torch.ops.pz.scale_update(amax[:n], qs, headroom, reset, maxval)
    amax, qs = amax.cpu(), qs.cpu()
    assert bit_equal(amax[n:], a[n:]) and bit_equal(qs[2 * n:], prev[2 * n:])
    assert bit_equal(amax[:n], torch.zeros(n) if reset else a[:n])
    zero = a[:n] == 0
    pairs, prev_pairs = qs[:2 * n].view(n, 2), prev[:2 * n].view(n, 2)
    assert bit_equal(pairs[zero], prev_pairs[zero])
    q64 = maxval / (a[:n].double() * headroom)
    q, s = pairs[:, 0].double(), pairs[:, 1].double()
    eq, es = ((q - q64).abs() / q64)[~zero], (s * q - 1).abs()[~zero]
    q32 = (torch.tensor(maxval) / (a[:n] * headroom))
    print(f"scale_update: max |q - q64| / q64 = {eq.max().item():.3e}, max |s q - 1| = {es.max().item():.3e}, "
          f"q bit-equal to the fp32 quotient: {torch.equal(pairs[:, 0][~zero], q32[~zero])}")
    assert (eq <= QBOUND).all() and (es <= QBOUND).all()
    assert bit_equal(pairs[~zero], torch.stack([q32, 1.0 / q32], 1)[~zero])  # IEEE fp32 quotients
    pow2 = torch.zeros(n, dtype=torch.bool)
    pow2[3::7] = True
    pow2 &= ~zero
    assert pow2.sum() >= 18 and torch.equal(q[pow2], q64[pow2])  # exact quotients: exact q


# ------------------------------------------------------------------------ 7. binding refusals
def _bad(kind):
    """A tensor a kernel must never see in place of a GPU fp32 array of >= 2 elements."""
    return {"cpu": torch.full((2,), 7.0), "dtype": torch.full((2,), 7.0, dtype=torch.float64, device=DEV),
            "small": torch.empty(0, device=DEV)}[kind]


KINDS = ["cpu", "dtype", "small"]


def refused(call, *untouched):
    before = [t.clone() for t in untouched]
    with pytest.raises(RuntimeError):
        call()
    torch.cuda.synchronize()
    for t, b in zip(untouched, before):
        assert bit_equal(t, b)


# (the derived scale, amax_in + amax_clear, exists on the 8-wide path only)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cols,arg", [(24, "qs"), (24, "amax"), (24, "amax_in"), (24, "amax_clear"), (12, "qs"),
                                      (12, "amax")])
def test_quantize_rows_refuses_bad_side_tensors(native_lib, cols, arg, kind):
    x = randn((8, cols), 1, F32).to(DEV)
    out = sentinel(8, cols, E4)
    good = {"qs": torch.full((2,), 7.0, device=DEV), "amax": torch.full((1,), 7.0, device=DEV)}
    if arg in ("amax_in", "amax_clear"):
        good.update(amax=None, amax_in=torch.ones(1, device=DEV), amax_clear=torch.full((1,), 7.0, device=DEV))
    args = dict(good, **{arg: _bad(kind)})
    keep = [t for t in args.values() if t is not None]
    refused(lambda: torch.ops.pz.quantize_rows(x, out, args["qs"], args["amax"], args.get("amax_in"),
                                               args.get("amax_clear")), out, *keep)


def test_quantize_rows_refuses_host_or_misaligned_out(native_lib):
    x = randn((8, 24), 1, F32).to(DEV)
    qs = torch.ones(2, device=DEV)
    host = torch.full((8, 24), SENT, dtype=U8).view(E4)
    refused(lambda: torch.ops.pz.quantize_rows(x, host, qs, None), host)
    buf = sentinel(8, 28, E4)  # out[:, 2:]: rows start 2 B past a 4-byte boundary, the packed stores need 4
    refused(lambda: torch.ops.pz.quantize_rows(x, buf[:, 2:], qs, None), buf)
    refused(lambda: torch.ops.pz.quantize_rows(x[:, :12], buf[:, 2:], qs, None), buf)
    torch.ops.pz.quantize_rows(x, buf[:, 4:], qs, None)  # 4-byte aligned: taken (by the scalar kernel)
    assert (buf.view(U8)[:, :4] == SENT).all()
    assert torch.equal(buf.view(U8)[:, 4:].cpu(), cast_bytes(x.float().cpu(), E4))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("arg", ["qs", "amax", "amax_clear"])
def test_quant_transpose_refuses_bad_side_tensors(native_lib, arg, kind):
    w = randn((64, 64), 2, F32).to(DEV)
    out = sentinel(64, 64, E4)
    args = {"qs": torch.full((2,), 7.0, device=DEV), "amax": torch.ones(1, device=DEV),
            "amax_clear": torch.full((1,), 7.0, device=DEV)}
    args[arg] = _bad(kind)
    refused(lambda: torch.ops.pz.quant_transpose(w, out, args["qs"], args["amax"], args["amax_clear"]), out,
            *args.values())
    if arg == "qs":  # also the path that only reads qs, and a record with no room for 1 / q
        refused(lambda: torch.ops.pz.quant_transpose(w, out, args["qs"]), out, args["qs"])
        one = torch.full((1,), 7.0, device=DEV)
        refused(lambda: torch.ops.pz.quant_transpose(w, out, one), out, one)


def test_quant_transpose_refuses_host_or_misaligned_out(native_lib):
    w = randn((64, 64), 2, F32).to(DEV)
    qs = torch.ones(2, device=DEV)
    host = torch.full((64, 64), SENT, dtype=U8).view(E4)
    refused(lambda: torch.ops.pz.quant_transpose(w, host, qs), host)
    buf = sentinel(64, 68, E4)
    refused(lambda: torch.ops.pz.quant_transpose(w, buf[:, 2:66], qs), buf)


@pytest.mark.parametrize("kind", KINDS)
def test_amax_abs_refuses_bad_amax(native_lib, kind):
    x = torch.ones(64, device=DEV)
    bad = _bad(kind)
    refused(lambda: torch.ops.pz.amax_abs(x, bad), bad)


@pytest.mark.parametrize("kind", KINDS)
def test_scale_update_refuses_bad_qs(native_lib, kind):
    amax = torch.ones(1, device=DEV)
    bad = _bad(kind)
    refused(lambda: torch.ops.pz.scale_update(amax, bad, 1.0, True, 448.0), amax, bad)
    short = torch.full((5,), 7.0, device=DEV)  # 3 scales need 6 slots
    amax3 = torch.ones(3, device=DEV)
    refused(lambda: torch.ops.pz.scale_update(amax3, short, 1.0, True, 448.0), amax3, short)
