"""The skinny GEMMs (csrc/gemm_skinny.hip: bf16 and fp32; csrc/gemm_skinny_w8.hip: e4m3 weights), value for
value, on every K-split plan cell, row bucket and last-slice tail.

Method (that of test_gemm_exact_gpu.py). x holds integers in [-4, 4] without the zero (no lost term
can vanish), W integers in [-4, 4]: exact in bf16, fp32 and e4m3. K <= 8192, so every partial sum is
an integer below 2^17 and every fp32 summation order (lane FMAs, the DPP pair add, the LDS fold, the
slice fold) gives the same z. Bias entries are multiples of 1/8 in [-4, 4]: z + bias needs at most
17 + 3 bits. For act in {none, ReLU}, with and without bias, the output must EQUAL the fp64 reference
rounded once to the output type (fp32 and bf16, assert_gemm_exact). ``out`` is a NaN-filled column
slice of a wider NaN tensor whose margins must stay NaN. Sigmoid / tanh stay with the bound tests of
test_skinny_gpu.py / test_skinny_w8_gpu.py: they do not depend on the plan cell.

The e4m3 kernel takes the integers as e4m3 codes directly, with scale[n] = 2^(n % 10 - 6), i.e. 2^e for
e in [-6, 3], a different one for neighbouring columns. scale z is a multiple of 2^e below 2^(17 + e),
the bias a multiple of 2^-3 up to 4: the sum is a multiple of 2^min(e, -3) below 2^(18 + max(e, 0)),
which needs 18 + max(e, 0) - min(e, -3) bits. That is 24, the fp32 significand, at both e = -6 and
e = 3, and less in between: scale z + bias is exact in fp32, and no wider exponent range would be.

Every (K, N) runs at M in {1, 2, 3, 4, 7, 8, 11, 16}: every bucket MB (1, 2, 4, 8, 16), full and partly
filled; z is computed once for 16 rows. Every test asserts the cell it means to reach from
PF.gemm_skinny_plan / PF.gemm_skinny_w8_plan, (strips, slices, slice_len) as the launcher plans them.

K rows per batch (Shape::kRows, W8Shape::kRows; BATCH_ROWS below), by bucket MB = 1, 2, 4, 8, 16:
    bf16 256 256 256 128 64 (two register sets)     fp32 256 256 256 256 128 (two register sets)
    w8   256 256 256 128 32 (two register sets; a ring of eight in the 16-row bucket)

Cells reached: kernel (K, N) -> strips x slices of slice_len; batches of a full slice by bucket, then those
of the last slice where it is shorter.
  slice_len 512, slices > 1
    bf16 (8192, 1088)   17 x 16 of 512     2 2 2 4 8
    w8   (8192, 2176)   17 x 16 of 512     2 2 2 4 16 (two turns of the ring)
    fp32 (8192, 544)    17 x 16 of 512     2 2 2 2 4 (the 512-row LDS stage filled)
  slice_len 768, a 513-row last slice
    bf16 (2049, 16448)  257 x 3 of 768     3 3 3 6 12; last 3 3 3 5 9
    w8   (2049, 32784)  257 x 3 of 768     3 3 3 6 24; last 3 3 3 5 17 (two turns and one batch)
  slice_len 1024, 4 slices
    bf16 (4096, 6592)   103 x 4 of 1024    4 4 4 8 16
    w8   (4096, 13184)  103 x 4 of 1024    4 4 4 8 32
  one slice (no ticket, no slab), the x stage full
    bf16 (1024, 32768)  512 x 1 of 1024    4 4 4 8 16
    w8   (1024, 65536)  512 x 1 of 1024    4 4 4 8 32
    fp32 (512, 16384)   512 x 1 of 512     2 2 2 2 4
  one ragged slice, the last strip ragged too
    bf16 (777, 33000)   516 x 1 of 1024    4 4 4 7 13
    w8   (777, 65552)   513 x 1 of 1024    4 4 4 7 25 (three turns and one batch)
    fp32 (389, 16388)   513 x 1 of 512     2 2 2 2 4
  a 1-row last slice
    bf16 (257, 64), w8 (257, 64)   1 x 2 of 256;   fp32 (1537, 16388)   513 x 4 of 512
  slice fold, 17 and 11 slices (neither <= 8 nor a multiple of 8: det_fold's remainder loop; the w8
  fold's chunks of CH = 16 (MB <= 4) and 8 (MB >= 8) end in a partial one, through its clamp)
    bf16, w8 (4352, 64) 1 x 17 of 256, (2816, 64) 1 x 11 of 256;  fp32 the same with 2 strips
  last-slice tails (test_last_slice_tails): K = 1024 + T, 171 strips of which the last holds one lane's
  columns, 3 slices of 512 (two batches in flight in the narrow buckets), the last of T rows, for
    T = 1, 31, 33, 63, 65, 127, 129, 255, 257, 300: one row short of and one row past a batch of 32, 64, 128
    and 256 rows, none a multiple of 8 but 300 (x staging: the element path at k + VEC > k1 while vec_ok
    holds); batches of the last slice in the 16-row bucket: bf16 1 1 1 1 2 2 3 4 5 5, fp32 1 1 1 1 1 1 2 2 3 3,
    w8 1 1 2 2 3 4 5 8 9 10 (9 and 10: the ring's second turn, partial)
  misaligned x (vec_ok false) at K = 1281, 3 slices of 512: an odd ldx, and a base 1 element off 16 B
  every W row once (test_every_row_of_w_is_returned_exactly): K = 1104, 69 calls of 16 one-hot rows
    bf16 (1104, 10944) 171 x 3 of 512;  fp32 (1104, 5472) 171 x 3 of 512;  w8 (1104, 32768) 256 x 2 of 768

Mutations. Each was built once into a copy of the library (values only, every address as before) and run
once on an MI355X against this file (63 tests), against test_skinny_gpu.py + test_skinny_w8_gpu.py as they
were before this file came ("old", 47 tests) and against the three long-slice row-invariance cases added
to them with this file ("added"). cells = test_plan_cell_is_exact_in_every_bucket.
  1  '>' for '>=' in load_batch's zeroing, both kernels: nothing fails anywhere, and nothing can. The
     clamped row k1 - 1 is then kept once more, for row k1 of the slice, but x is staged with zeros
     from row k1 on, so the extra term is 0 * w for every finite w: an equivalent mutant.
  1b the zeroing one row early ('>= k1 - 1': the last row of EVERY slice is lost): this file 61 (all
     that launch), old 34, added 0.
  1n exactly one row lost, the last of K, where K >= 2048 (the off-by-one the bound tests are too wide
     for): this file 13, every cell with K >= 2048, both kernels, all three types. old 4: the bound
     catches it at (5, 4096, 1024) and misses it at (16, 8192, 64), in both kernels. added 0.
  2  no 'wa[u] = wb[u]' copy: this file 40, every bf16 and fp32 test. old 11 (the buckets of 8 and 16
     rows run several batches of a 256-row slice). added 2.
  2n the same in the buckets MB <= 4 only, where a 256-row slice is one batch: this file 33 (every
     bf16 / fp32 cell with slice_len >= 512, all tails, misaligned x). old 0. added 2 (bf16, fp32).
  3  the e4m3 ring issuing into set (s + NS - 2) % NS: this file 21, every e4m3 test. old 10. added 1.
  3n the same from the ring's second turn on, 8-set ring only: this file 18 (e4m3 cells with a slice
     over 256 rows, all tails, misaligned x, every row). old 0. added 1.
  4  the e4m3 fold adding the clamped re-read: this file 18, every e4m3 test whose slice count is not
     a whole number of chunks (3, 4, 2, 17, 11 slices; not 16, not 1). old 4 (2 and 4 slices). added 1.
  4n the same in every chunk but the first: this file 2, the cells of 17 and 11 slices. old 0. added 0.
So the old files did see 2, 3 and 4 in their plain form, through the wide buckets; narrowed to the paths
no old shape ran (2n, 3n, 4n) they pass the old files and fail here.

Measured on MI355X: every test passes; the file takes about 3 s (63 tests, 2.5 s in pytest; the
slowest, the first to touch the device, 0.6 s). Operands and fp64 products are made on the GPU.
"""
import functools

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import ACT_FWD, assert_gemm_exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32, E4M3 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
ROWS = 16
MS = (1, 2, 3, 4, 7, 8, 11, 16)
STRIP_COLS = {"bf16": 64, "f32": 32, "w8": 128}
# K rows per batch by bucket: Shape<T, MB>::kRows / W8Shape<MB>::kRows. Only used to say, and to
# check, which batch boundary a tail length sits next to; the kernels do not read it
BATCH_ROWS = {"bf16": {1: 256, 2: 256, 4: 256, 8: 128, 16: 64},
              "f32": {1: 256, 2: 256, 4: 256, 8: 256, 16: 128},
              "w8": {1: 256, 2: 256, 4: 256, 8: 128, 16: 32}}


def plan_of(kern, K, N):
    """(strips, slices, slice_len) as the launcher itself plans this shape."""
    return PF.gemm_skinny_w8_plan(K, N) if kern == "w8" else PF.gemm_skinny_plan(K, N, BF16 if kern == "bf16" else F32)


def last_slice_rows(K, plan):
    return K - (plan[1] - 1) * plan[2]


def int_operands(kern, K, N, seed):
    """x [16, K] with integers in [-4, 4] \\ {0}, W [K, N] with integers in [-4, 4] (e4m3 for ``w8``,
    else the operand dtype), scale [N] (``w8`` only), bias [N] in multiples of 1/8, all on the GPU."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    wi = torch.randint(-4, 5, (K, N), device=DEV, generator=g, dtype=torch.int8)
    xi = torch.randint(1, 5, (ROWS, K), device=DEV, generator=g) * (2 * torch.randint(0, 2, (ROWS, K), device=DEV, generator=g) - 1)
    bias = torch.randint(-32, 33, (N,), device=DEV, generator=g).float() / 8
    xdt = F32 if kern == "f32" else BF16
    x, w = xi.to(xdt), wi.to(xdt)
    scale = None
    if kern == "w8":
        w = w.to(E4M3)
        assert torch.equal(w.float(), wi.float())
        scale = torch.ldexp(torch.ones(N, device=DEV), torch.arange(N, device=DEV, dtype=torch.int32) % 10 - 6)
    assert (x != 0).all()
    return x, w, scale, bias


def product(x, w):
    """fp64 x @ W on the GPU: integers below 2^17, exact in any order."""
    return x.double() @ w.float().double()


def launch(kern, x, w, scale, out, bias, act):
    if kern == "w8":
        assert PF.gemm_skinny_w8_eligible(x, w, scale, out)
        PF.gemm_skinny_w8(x, w, scale, out, bias=bias, act=act)
    else:
        assert PF.gemm_skinny_eligible(x, w, out)
        PF.gemm_skinny(x, w, out, bias=bias, act=act)


def check_exact(kern, x, w, scale, bias, z, ms=MS):
    """Every M of ``ms``, fp32 and bf16 outputs, with and without bias, no activation and ReLU: the
    output equals the reference rounded once; NaN margins around ``out`` stay NaN."""
    n = w.shape[1]
    zs = z * scale.double() if scale is not None else z
    for has_bias in (False, True):
        pre = zs + bias.double() if has_bias else zs
        for act in (PF.ACT_NONE, PF.ACT_RELU):
            ref = ACT_FWD[act](pre)
            for m in ms:
                for out_dtype in (F32, BF16):
                    parent = torch.full((m, n + 5), float("nan"), device=DEV, dtype=out_dtype)
                    out = parent[:, 2:2 + n]
                    launch(kern, x[:m], w, scale, out, bias if has_bias else None, act)
                    try:
                        assert_gemm_exact(out, ref[:m])
                    except AssertionError as e:
                        raise AssertionError(f"M={m} out={out_dtype} bias={has_bias} act={act}: {e}") from None
                    assert parent[:, :2].isnan().all() and parent[:, 2 + n:].isnan().all(), (m, out_dtype, has_bias, act)


# (kernel, K, N, (strips, slices, slice_len), rows of the last slice)
CELLS = [
    ("bf16", 8192, 1088, (17, 16, 512), 512),
    ("w8", 8192, 2176, (17, 16, 512), 512),
    ("f32", 8192, 544, (17, 16, 512), 512),
    ("bf16", 2049, 16448, (257, 3, 768), 513),
    ("w8", 2049, 32784, (257, 3, 768), 513),
    ("bf16", 4096, 6592, (103, 4, 1024), 1024),
    ("w8", 4096, 13184, (103, 4, 1024), 1024),
    ("bf16", 1024, 32768, (512, 1, 1024), 1024),
    ("w8", 1024, 65536, (512, 1, 1024), 1024),
    ("f32", 512, 16384, (512, 1, 512), 512),
    ("bf16", 777, 33000, (516, 1, 1024), 777),
    ("w8", 777, 65552, (513, 1, 1024), 777),
    ("f32", 389, 16388, (513, 1, 512), 389),
    ("bf16", 257, 64, (1, 2, 256), 1),
    ("w8", 257, 64, (1, 2, 256), 1),
    ("f32", 1537, 16388, (513, 4, 512), 1),
    ("bf16", 4352, 64, (1, 17, 256), 256),
    ("w8", 4352, 64, (1, 17, 256), 256),
    ("f32", 4352, 64, (2, 17, 256), 256),
    ("bf16", 2816, 64, (1, 11, 256), 256),
    ("w8", 2816, 64, (1, 11, 256), 256),
    ("f32", 2816, 64, (2, 11, 256), 256),
]


@pytest.mark.parametrize("kern,K,N,plan,last", CELLS, ids=[f"{c[0]}_{c[1]}x{c[2]}" for c in CELLS])
def test_plan_cell_is_exact_in_every_bucket(native_lib, kern, K, N, plan, last):
    assert plan_of(kern, K, N) == plan
    assert last_slice_rows(K, plan) == last and plan[0] == -(-N // STRIP_COLS[kern])
    x, w, scale, bias = int_operands(kern, K, N, seed=K + N)
    check_exact(kern, x, w, scale, bias, product(x, w))


def test_the_cells_cover_every_slice_length_fold_shape_and_ring_turn(native_lib):
    """What the table above is for, from the reported plans: per kernel every slice length with
    several slices, a full single slice, a ragged one, a 1-row last slice, slice counts that leave the
    folds a partial chunk; and for the e4m3 kernel's ring of 8 sets slices of more than 8 batches
    that are no multiple of 8."""
    got = {kern: [] for kern in STRIP_COLS}
    for kern, K, N, _, _ in CELLS:
        got[kern].append((K, N) + plan_of(kern, K, N))
    for kern, cells in got.items():
        lens = (256, 512) if kern == "f32" else (256, 512, 768, 1024)
        for ln in lens:
            assert any(c[4] == ln and c[3] > 1 for c in cells), (kern, ln)
        top = lens[-1]
        assert any(c[3] == 1 and c[0] == top for c in cells), kern                       # one full slice
        assert any(c[3] == 1 and c[0] % 256 and c[1] % STRIP_COLS[kern] for c in cells), kern  # one ragged slice
        assert any(c[3] > 1 and last_slice_rows(c[0], c[2:]) == 1 for c in cells), kern
        assert any(c[3] > 8 and c[3] % 8 for c in cells), kern
    ring = {-(-min(c[4], last_slice_rows(c[0], c[2:])) // BATCH_ROWS["w8"][16]) for c in got["w8"]}
    assert {17, 25} <= ring and any(b > 8 and b % 8 == 0 for b in ring), ring


# ------------------------------------------------------------------------------- last-slice tails
TAILS = (1, 31, 33, 63, 65, 127, 129, 255, 257, 300)
TAIL_BASE_K = 1024          # two full 512-row slices before the tail
TAIL_K_MAX = 1328           # a multiple of 8: the row views x[:, :K] keep vec_ok
TAIL_STRIPS = 171


def tail_n(kern):
    """170 whole strips and one that holds a single lane's columns (16 B of a W row)."""
    return (TAIL_STRIPS - 1) * STRIP_COLS[kern] + {"bf16": 8, "f32": 4, "w8": 16}[kern]


@functools.lru_cache(maxsize=None)
def tail_operands(kern):
    x, w, scale, bias = int_operands(kern, TAIL_K_MAX, tail_n(kern), seed=77)
    return x, w, scale, bias, w.float().double()


def test_tail_lengths_sit_on_both_sides_of_every_batch_size():
    for kern, rows in BATCH_ROWS.items():
        for br in set(rows.values()):
            assert br - 1 in TAILS and br + 1 in TAILS, (kern, br)
    assert sum(t % 8 != 0 for t in TAILS) >= 8
    assert any(8 < -(-t // BATCH_ROWS["w8"][16]) < 16 for t in TAILS)    # the ring's second turn, partial


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("kern", list(STRIP_COLS))
def test_last_slice_tails(native_lib, kern, tail):
    """K = 1024 + tail: two full 512-row slices and a last slice of ``tail`` rows, in every bucket;
    the last strip is ragged. x[:, :K] and W[:K] are views of one operand pair (vec_ok holds)."""
    K, N = TAIL_BASE_K + tail, tail_n(kern)
    plan = plan_of(kern, K, N)
    assert plan == (TAIL_STRIPS, 3, 512) and last_slice_rows(K, plan) == tail and N % STRIP_COLS[kern] != 0
    xf, wf, scale, bias, w64 = tail_operands(kern)
    x, w = xf[:, :K], wf[:K]
    assert x.data_ptr() % 16 == 0 and (x.stride(0) * x.element_size()) % 16 == 0
    check_exact(kern, x, w, scale, bias, x.double() @ w64[:K])


@pytest.mark.parametrize("how", ["odd_ldx", "base_off_16B"])
@pytest.mark.parametrize("kern", list(STRIP_COLS))
def test_misaligned_x_with_a_long_slice(native_lib, kern, how):
    """vec_ok false: every x element is staged by the element path, 512 rows a slice, 257 in the last."""
    K, N = TAIL_BASE_K + 257, tail_n(kern)
    assert plan_of(kern, K, N) == (TAIL_STRIPS, 3, 512)
    xf, wf, scale, bias, w64 = tail_operands(kern)
    if how == "odd_ldx":
        x = torch.zeros(ROWS, K + 2, device=DEV, dtype=xf.dtype)[:, :K]
        assert x.data_ptr() % 16 == 0 and (x.stride(0) * x.element_size()) % 16 != 0
    else:
        x = torch.zeros(ROWS, K + 7, device=DEV, dtype=xf.dtype)[:, 1:1 + K]
        assert x.data_ptr() % 16 != 0 and (x.stride(0) * x.element_size()) % 16 == 0
    x.copy_(xf[:, :K])
    check_exact(kern, x, wf[:K], scale, bias, x.double() @ w64[:K])


# ------------------------------------------------------------------------------- every W row, once
def row_pattern(K, N, base):
    """Integers in [0, base): W[k, n] = (digit (n % 3) of k in base ``base`` + 3 n) % base. Any three
    neighbouring columns name the row (K < base^3) and neighbouring columns differ, so neither a
    wrong row nor a wrong column can hide. (The pattern of the 300-row identity tests, (7 k + 3 n) %
    251, repeats every 251 rows.)"""
    assert K < base ** 3
    k = torch.arange(K, device=DEV)[:, None]
    n = torch.arange(N, device=DEV)[None, :]
    return (k // (base ** (n % 3)) + 3 * n) % base


# kernel -> (N, plan of (1104, N), base of the pattern: 251 fits bf16's integers, 17 e4m3's)
EVERY_ROW = {"bf16": (10944, (171, 3, 512), 251), "f32": (5472, (171, 3, 512), 251), "w8": (32768, (256, 2, 768), 17)}


@pytest.mark.parametrize("kern", list(STRIP_COLS))
def test_every_row_of_w_is_returned_exactly(native_lib, kern):
    """x = 16 one-hot rows per call, stepping through all K rows of a long-slice plan: each call
    returns those 16 rows of W (times the column scales for e4m3), fp32 and bf16 outputs."""
    K = 1104
    N, plan, base = EVERY_ROW[kern]
    assert plan_of(kern, K, N) == plan and plan[2] >= 512
    wi = row_pattern(K, N, base)
    xdt = F32 if kern == "f32" else BF16
    w, scale = wi.to(xdt), None
    if kern == "w8":
        w = w.to(E4M3)
        scale = torch.ldexp(torch.ones(N, device=DEV), torch.arange(N, device=DEV, dtype=torch.int32) % 10 - 6)
    assert torch.equal(w.float().double(), wi.double())
    want = wi.double() * scale.double() if scale is not None else wi.double()
    eye = torch.eye(K, device=DEV, dtype=xdt)
    for k0 in range(0, K, ROWS):
        x = eye[k0:k0 + ROWS]
        for out_dtype in (F32, BF16):
            parent = torch.full((ROWS, N + 5), float("nan"), device=DEV, dtype=out_dtype)
            out = parent[:, 2:2 + N]
            launch(kern, x, w, scale, out, None, PF.ACT_NONE)
            try:
                assert_gemm_exact(out, want[k0:k0 + ROWS])
            except AssertionError as e:
                raise AssertionError(f"rows {k0}..{k0 + ROWS - 1} out={out_dtype}: {e}") from None
            assert parent[:, :2].isnan().all() and parent[:, 2 + N:].isnan().all()
