"""pz::stage_fwd / stage_bwd, softmax_rows / softmax_bwd and gather_rows, raw ops, against fp64 torch.

Bounds. fp64 kernels: 1e-12 |ref| + 1e-12. fp32-math kernels (fp32 and bf16 data; __expf): per element
1e-5 x the scale of the quantity (|ref| for activations, the row's largest |ref| for softmax) + 1e-12,
and 2^-8 |ref| more when the output is stored as bf16. Data movement, relu and dropout (one multiply
by the scale per dropout) are bit-equal to the same operations done by torch in the math dtype.

Kernels reached (csrc/elementwise.hip): stage_fwd_kernel<in, out> for f64-f64, f32-f32, bf16-bf16,
f32-bf16 and bf16-f32 (the four pairs that mix fp64 with another dtype have no caller and no test);
stage_bwd_kernel, softmax_rows_kernel and softmax_bwd_kernel for f64, f32 and bf16;
gather_rows_kernel<in, out> for f32-f32, f64-f64, f32-bf16 and bf16-bf16 (GATHER_CASES "scalar-*";
the other five pairs have no caller and no test) and gather_rows_vec_kernel<float>, <bf16> ("vec-*").
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import (bit_equal, gather_picks, gather_seed, keep2d, stage_bwd_reference, stage_fwd_reference)

pytestmark = pytest.mark.gpu
DEV = "cuda"

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NAME = {F64: "f64", F32: "f32", BF16: "bf16"}
SEED = (0x1234ABCD, 0x00C0FFEE)
P = 0.25
LID_PRE, LID_POST = 3, 4
# dropout placement -> (drop_pre, drop_post) layer ids of PF.epi_spec
DROPS = {"nodrop": (-1, -1), "pre": (LID_PRE, -1), "post": (-1, LID_POST), "pre+post": (LID_PRE, LID_POST)}
ACTS = {"none": PF.ACT_NONE, "relu": PF.ACT_RELU, "sigmoid": PF.ACT_SIGMOID, "tanh": PF.ACT_TANH}
U32 = 2.0 ** -24  # unit roundoff of the fp32 math


def math_dtype(t):
    return F64 if t == F64 else F32


def randn(shape, seed, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F64).to(dtype)


def assert_close(got, ref, scale, what, extra=None):
    """`got` (any float dtype, GPU or CPU) against the fp64 `ref`; `scale`: the fp32-math bound's scale
    per element (broadcastable); `extra`: a derived absolute allowance, see the call site."""
    got64 = got.double().cpu()
    assert torch.isfinite(got64).all(), what
    err = (got64 - ref).abs()
    if got.dtype == F64:
        bound = 1e-12 * ref.abs() + 1e-12
    else:
        bound = 1e-5 * scale + 1e-12 + (2.0 ** -8 * ref.abs() if got.dtype == BF16 else 0.0)
        if extra is not None:
            bound = bound + extra
    worst = (err / bound).max().item() if err.numel() else 0.0
    print(f"{what}: max err {err.max().item() if err.numel() else 0.0:.3e}, worst err/bound {worst:.3f}")
    assert (err <= bound).all(), (what, err.max().item(), worst)


# ------------------------------------------------------------------------------------------ stage
def stage_masks(n, drop, p, epoch=None):
    pre, post = DROPS[drop]
    kp = keep2d(1, n, n, SEED, pre, p, epoch)[0] if pre >= 0 else None
    kq = keep2d(1, n, n, SEED, post, p, epoch)[0] if post >= 0 else None
    return kp, kq


def run_stage_fwd(x, tout, spec):
    y = torch.full(x.shape, 7.0, dtype=tout, device=DEV)
    torch.ops.pz.stage_fwd(x.to(DEV), y, spec[0], spec[1])
    torch.cuda.synchronize()
    return y.cpu()


def check_stage_fwd(x, y, act, kp, kq, spec, what):
    """y = drop_post(act(drop_pre(x))) for the stored x. relu / no activation: bit-equal to the same
    multiplies done in the math dtype and one rounding to y's dtype."""
    F = math_dtype(y.dtype)
    if act in (PF.ACT_NONE, PF.ACT_RELU):
        exact = stage_fwd_reference(x.to(F), act, kp, kq, torch.tensor(spec[1][0], dtype=F)).to(y.dtype)
        assert bit_equal(y, exact), what
        return
    ref = stage_fwd_reference(x.double(), act, kp, kq, torch.tensor(spec[1][0], dtype=F64))
    assert_close(y, ref, ref.abs(), what)
    if kq is not None:  # dropped after the activation: exactly zero (after drop_pre sigmoid(0) = 0.5 follows)
        assert (y[~kq] == 0).all(), what


def check_stage_bwd(g, y, dx, act, kp, kq, p, what):
    """dx against g * scale_post keep_post * act'(y / scale_post) * scale_pre keep_pre from the stored y.

    The derivative comes from the OUTPUT: a = fl(y * (1 - p)), then fl(1 - fl(a a)) (tanh) or
    fl(a fl(1 - a)) (sigmoid). For |a| <= 1 those err by at most 4 u absolutely (u = 2^-24: one rounding
    of a, of a a and of the subtraction), however small the derivative itself is — a cancellation the
    relative bound cannot cover — so the bound gains 4 u |g| scale_post scale_pre."""
    sc = 1.0 / (1.0 - p)
    ref = stage_bwd_reference(g, y, act, kp, kq, sc)
    total = (sc if kp is not None else 1.0) * (sc if kq is not None else 1.0)
    extra = 4 * U32 * g.double().abs() * total if act in (PF.ACT_SIGMOID, PF.ACT_TANH) else None
    assert_close(dx, ref, ref.abs(), what, extra)
    for k in (kp, kq):
        if k is not None:
            assert (dx[~k] == 0).all(), what


PAIRS = [(F64, F64), (F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)]


@pytest.mark.parametrize("drop", list(DROPS))
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("tin,tout", PAIRS, ids=[f"{NAME[a]}-{NAME[b]}" for a, b in PAIRS])
def test_stage_fwd_epilogues(native_lib, tin, tout, act, drop):
    pre, post = DROPS[drop]
    spec = PF.epi_spec(ACTS[act], drop_pre=pre, drop_post=post, p=P, seed=SEED)
    for n in (1, 255, 257):
        x = 1.5 * randn((n,), 100 + n, tin)
        kp, kq = stage_masks(n, drop, P)
        y = run_stage_fwd(x, tout, spec)
        check_stage_fwd(x, y, ACTS[act], kp, kq, spec, f"stage_fwd n={n}")
    if drop == "pre+post":
        kp, kq = stage_masks(257, drop, P)
        assert 0.6 < kp.double().mean() < 0.9 and not torch.equal(kp, kq)  # two layer ids, two masks


@pytest.mark.parametrize("drop", list(DROPS))
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
def test_stage_bwd_epilogues(native_lib, t, act, drop):
    pre, post = DROPS[drop]
    spec = PF.epi_spec(ACTS[act], drop_pre=pre, drop_post=post, p=P, seed=SEED)
    for n in (1, 255, 257):
        x, g = 1.5 * randn((n,), 200 + n, t), randn((n,), 300 + n, t)
        kp, kq = stage_masks(n, drop, P)
        y = run_stage_fwd(x, t, spec)  # the stored forward output (checked by the forward test)
        dx = torch.full((n,), 7.0, dtype=t, device=DEV)
        torch.ops.pz.stage_bwd(g.to(DEV), y.to(DEV), dx, spec[0], spec[1])
        torch.cuda.synchronize()
        check_stage_bwd(g, y, dx.cpu(), ACTS[act], kp, kq, P, f"stage_bwd n={n}")


@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
def test_stage_grid_stride_second_pass(native_lib, t):
    """1 048 579 elements: 4096 blocks x 256 lanes cover 1 048 576, so three elements (and the masks of
    indices past 2^20) come from the second grid-stride pass."""
    n = 1_048_579
    spec = PF.epi_spec(PF.ACT_RELU, drop_pre=LID_PRE, drop_post=LID_POST, p=P, seed=SEED)
    x, g = 1.5 * randn((n,), 41, t), randn((n,), 42, t)
    kp, kq = stage_masks(n, "pre+post", P)
    y = run_stage_fwd(x, t, spec)
    check_stage_fwd(x, y, PF.ACT_RELU, kp, kq, spec, "stage_fwd 2^20+3")
    assert (y[-3:] != 7.0).all()
    dx = torch.full((n,), 7.0, dtype=t, device=DEV)
    torch.ops.pz.stage_bwd(g.to(DEV), y.to(DEV), dx, spec[0], spec[1])
    torch.cuda.synchronize()
    check_stage_bwd(g, y, dx.cpu(), PF.ACT_RELU, kp, kq, P, "stage_bwd 2^20+3")


@pytest.mark.parametrize("drop", ["pre", "post", "pre+post"])
@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
def test_stage_drop_all_is_exactly_zero(native_lib, t, drop):
    pre, post = DROPS[drop]
    spec = PF.epi_spec(PF.ACT_TANH, drop_pre=pre, drop_post=post, p=1.0, seed=SEED)
    assert spec[0][6] == 1
    for n in (1, 257):
        x, g = randn((n,), 51, t), randn((n,), 52, t)
        y = run_stage_fwd(x, t, spec)
        dx = torch.full((n,), 7.0, dtype=t, device=DEV)
        torch.ops.pz.stage_bwd(g.to(DEV), y.to(DEV), dx, spec[0], spec[1])
        torch.cuda.synchronize()
        zero = torch.zeros(n, dtype=t)
        assert bit_equal(y, zero) and bit_equal(dx.cpu(), zero)


@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
def test_stage_device_epoch_counter_matches_eager_epoch(native_lib, t):
    """A graph-replayed step reads the epoch from a device counter; an eager one mixes it on the host."""
    n = 257
    counter = torch.tensor([3], dtype=torch.int32, device=DEV)
    kw = dict(drop_pre=LID_PRE, drop_post=LID_POST, p=P, seed=SEED)
    dev_spec = PF.epi_spec(PF.ACT_RELU, epoch_ptr=counter.data_ptr(), **kw)
    eager = PF.epi_spec(PF.ACT_RELU, epoch=3, **kw)
    x, g = 1.5 * randn((n,), 61, t), randn((n,), 62, t)
    kp, kq = stage_masks(n, "pre+post", P, epoch=3)
    assert not torch.equal(kp, stage_masks(n, "pre+post", P)[0])
    y = run_stage_fwd(x, t, dev_spec)
    assert bit_equal(y, run_stage_fwd(x, t, eager))
    check_stage_fwd(x, y, PF.ACT_RELU, kp, kq, eager, "stage_fwd epoch counter")
    outs = []
    for spec in (dev_spec, eager):
        dx = torch.full((n,), 7.0, dtype=t, device=DEV)
        torch.ops.pz.stage_bwd(g.to(DEV), y.to(DEV), dx, spec[0], spec[1])
        torch.cuda.synchronize()
        outs.append(dx.cpu())
    assert bit_equal(outs[0], outs[1])
    check_stage_bwd(g, y, outs[0], PF.ACT_RELU, kp, kq, P, "stage_bwd epoch counter")
    assert counter.item() == 3


# ---------------------------------------------------------------------------------------- softmax
def run_softmax(x):
    y = torch.full(x.shape, 7.0, dtype=x.dtype, device=DEV)
    torch.ops.pz.softmax_rows(x.to(DEV), y)
    torch.cuda.synchronize()
    return y.cpu()


def check_softmax(x, y, what):
    ref = torch.softmax(x.double(), -1)
    assert_close(y, ref, ref.amax(-1, keepdim=True), what)
    return ref


def check_softmax_bwd(g, y, what):
    dx = torch.full(y.shape, 7.0, dtype=y.dtype, device=DEV)
    torch.ops.pz.softmax_bwd(g.to(DEV), y.to(DEV), dx)
    torch.cuda.synchronize()
    y64, g64 = y.double(), g.double()
    ref = y64 * (g64 - (g64 * y64).sum(-1, keepdim=True))
    assert_close(dx, ref, ref.abs().amax(-1, keepdim=True), what)


SOFTMAX_SHAPES = [(r, c) for r in (1, 5) for c in (1, 63, 64, 65, 130)] + [(2, 3, 65)]


@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
@pytest.mark.parametrize("shape", SOFTMAX_SHAPES, ids=["x".join(map(str, s)) for s in SOFTMAX_SHAPES])
def test_softmax_forward_backward(native_lib, shape, t):
    x = 3.0 * randn(shape, 7 + sum(shape), t)
    y = run_softmax(x)
    check_softmax(x, y, "softmax_rows")
    check_softmax_bwd(randn(shape, 9 + sum(shape), t), y, "softmax_bwd")


@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
@pytest.mark.parametrize("cols", [1, 65, 130])
def test_softmax_shift_invariance(native_lib, cols, t):
    """Rows x, x + s and x - s give the same result. The shifted rows must hold x + s exactly, so x is
    made of multiples of 1/8 and s = 1e4 (17 significand bits) for fp32 / fp64; bf16 has 8 bits, so
    there s = 9984 (the bf16 next to 1e4, spacing 64) and x is made of multiples of 64."""
    g = torch.Generator(device="cpu").manual_seed(cols)
    if t == BF16:
        base, s = -64.0 * torch.randint(0, 3, (cols,), generator=g).double(), 9984.0
    else:
        base, s = torch.round(24.0 * torch.randn(cols, generator=g, dtype=F64)) / 8.0, 1e4
    x = torch.stack([base, base + s, base - s]).to(t)
    assert torch.equal(x.double(), torch.stack([base, base + s, base - s]))
    y = run_softmax(x)
    ref = check_softmax(x[:1], y[:1], "softmax unshifted")
    for r in (1, 2):
        assert_close(y[r:r + 1], ref, ref.amax(-1, keepdim=True), f"softmax shifted row {r}")


@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
@pytest.mark.parametrize("cols", [65, 130])
def test_softmax_minus_inf_and_dominant_entries(native_lib, cols, t):
    x = 3.0 * randn((2, cols), 70 + cols, t)
    x[0, 0] = x[0, 63] = x[0, 64] = x[0, cols - 1] = float("-inf")
    x[1, cols - 2] = 40.0
    y = run_softmax(x)
    ref = check_softmax(x, y, "softmax -inf / dominant")
    hole = torch.isinf(x[0])
    assert hole.sum() >= 3 and (y[0][hole] == 0).all() and (y[0][~hole] > 0).all()
    room = 1e-12 * cols if t == F64 else 1e-5 * cols + (2.0 ** -8 if t == BF16 else 0.0)  # the per-element bounds, summed
    assert abs(y[0].double().sum().item() - 1.0) <= room
    assert ref[1, cols - 2] > 0.999999 and abs(y[1, cols - 2].item() - 1.0) <= 1e-5
    check_softmax_bwd(randn((2, cols), 71, t), y, "softmax_bwd -inf / dominant")


# ----------------------------------------------------------------------------------------- gather
ROWS, ROWS_VALID = 37, 33
GSEED = (0xDEADBEEF, 0x0BADF00D)
# name: (data dtype, out dtype, cols, data buffer (left, right) extra columns, out extra columns, kernel)
GATHER_CASES = {
    "scalar-f32-f32-c4": (F32, F32, 4, (0, 0), 0),
    "scalar-f64-f64-c4": (F64, F64, 4, (0, 0), 0),
    "scalar-f32-bf16-c12": (F32, BF16, 12, (0, 0), 0),         # cols % 8 != 0
    "scalar-bf16-bf16-ld12": (BF16, BF16, 8, (0, 4), 4),       # cols % 8 == 0 but ld % 8 != 0
    "vec-f32-bf16-c8": (F32, BF16, 8, (8, 0), 8),
    "vec-bf16-bf16-c8": (BF16, BF16, 8, (8, 0), 8),
    "vec-f32-bf16-c520": (F32, BF16, 520, (8, 0), 8),          # 520 > 512: the second lane iteration
    "vec-bf16-bf16-c520": (BF16, BF16, 520, (8, 0), 8),
}


class Gather:
    """One gather_rows case: a [n_data, cols] table (a column slice of a wider buffer), labels, and
    sentinel-filled outputs."""

    def __init__(self, case, n_data, rows=ROWS, rows_valid=ROWS_VALID, with8=False):
        tin, tout, cols, (left, right), out_extra = GATHER_CASES[case]
        g = torch.Generator(device="cpu").manual_seed(n_data + cols)
        self.rows, self.rows_valid, self.cols, self.n_data, self.tout = rows, rows_valid, cols, n_data, tout
        buf = torch.randn(n_data, left + cols + right, generator=g, dtype=F64).to(tin)
        self.table = buf[:, left:left + cols]
        self.data = buf.to(DEV)[:, left:left + cols]
        self.labels = torch.randint(0, 1000, (n_data,), generator=g)
        self.out_buf = torch.full((rows, cols + out_extra), 7.0, dtype=tout, device=DEV)
        self.out = self.out_buf[:, :cols]
        self.lab = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
        self.picked = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
        self.data8 = self.out8 = None
        if with8:
            self.table8 = torch.randint(0, 256, (n_data, cols), generator=g, dtype=torch.uint8)
            self.data8 = self.table8.to(DEV).view(torch.float8_e4m3fn)
            self.out8 = torch.full((rows, cols), 7, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)

    def run(self, indices=None, seed=GSEED, epoch=None, su=()):
        torch.ops.pz.gather_rows(self.data, indices, seed[0], seed[1], self.out, self.rows_valid, self.labels.to(DEV),
                                 self.lab, self.picked, epoch, self.data8, self.out8, *su)
        torch.cuda.synchronize()

    def check(self, picks):
        n = self.rows_valid
        picks = torch.as_tensor(picks)
        assert picks.dtype == torch.int64 and picks.min() >= 0 and picks.max() < self.n_data
        assert torch.equal(self.picked[:n].cpu(), picks)
        assert (self.picked[n:] == -7).all()  # no pick for a padding row
        assert torch.equal(self.lab[:n].cpu(), self.labels[picks]) and (self.lab[n:] == 0).all()
        out = self.out_buf.cpu()
        assert bit_equal(out[:n, :self.cols], self.table[picks].to(self.tout))
        assert bit_equal(out[n:, :self.cols], torch.zeros(self.rows - n, self.cols, dtype=self.tout))
        assert (out[:, self.cols:] == 7.0).all()  # the buffer's other columns
        if self.out8 is not None:
            o8 = self.out8.view(torch.uint8).cpu()
            assert torch.equal(o8[:n], self.table8[picks]) and (o8[n:] == 0).all()


@pytest.mark.parametrize("n_data", [1, 3, 1000])
@pytest.mark.parametrize("case", list(GATHER_CASES))
def test_gather_sampled_rows_match_the_hash(native_lib, case, n_data):
    c = Gather(case, n_data)
    c.run()
    picks = gather_picks(ROWS_VALID, n_data, *GSEED)
    c.check(picks)
    if n_data == 1000:
        assert len(set(picks.tolist())) > 20  # a sample, not a constant


@pytest.mark.parametrize("case", list(GATHER_CASES))
def test_gather_explicit_indices(native_lib, case):
    n_data = 50
    c = Gather(case, n_data)
    idx = torch.arange(ROWS_VALID) * 7 % n_data
    idx[:4] = torch.tensor([n_data - 1, 0, n_data - 1, 5])
    idx[-1] = 5
    c.run(indices=torch.cat([idx, torch.full((ROWS - ROWS_VALID,), 7)]).to(DEV))  # padding rows stay zero
    c.check(idx)


@pytest.mark.parametrize("case", ["scalar-f32-bf16-c12", "vec-f32-bf16-c520"])
def test_gather_device_epoch_counter(native_lib, case):
    from penr_oz_neural_network_torch_amd.engine.trainer import FusedTrainer

    n_data = 1000
    counter = torch.tensor([5], dtype=torch.int32, device=DEV)
    c = Gather(case, n_data)
    c.run(epoch=counter)
    picks = gather_picks(ROWS_VALID, n_data, *GSEED, epoch=5)
    c.check(picks)
    assert not np.array_equal(picks, gather_picks(ROWS_VALID, n_data, *GSEED))
    # the host mirror the eager steps use: the same seeds, so the same sample
    me = SimpleNamespace(base_seed=GSEED, ctx=SimpleNamespace(rank=0))
    host = FusedTrainer._gather_seed(me, 5)
    assert host == gather_seed(*GSEED, 5) and FusedTrainer._gather_seed(me, None) == GSEED
    e = Gather(case, n_data)
    e.run(seed=host)
    e.check(picks)
    assert counter.item() == 5


@pytest.mark.parametrize("indices", [False, True], ids=["hash", "indices"])
@pytest.mark.parametrize("case", ["scalar-f32-bf16-c12", "vec-f32-bf16-c520", "vec-bf16-bf16-c520"])
def test_gather_e4m3_side_table(native_lib, case, indices):
    n_data = 100
    c = Gather(case, n_data, with8=True)
    if indices:
        idx = (torch.arange(ROWS_VALID) * 13 + 99) % n_data
        c.run(indices=idx.to(DEV))
        c.check(idx)
    else:
        c.run()
        c.check(gather_picks(ROWS_VALID, n_data, *GSEED))


def check_scale_update(amax, qs, prev=None):
    """ScaleUpd with amax = [2, 0, 0.5], headroom 2, maxval 448 over a 7.0-filled qs."""
    q = qs.cpu()
    assert q[0].item() == 112.0 and q[4].item() == 448.0
    for i, v in ((1, 112.0), (5, 448.0)):
        ref = np.float32(1.0 / v)
        assert abs(np.float64(q[i].item()) - np.float64(1.0) / v) <= 2 * np.float64(np.spacing(ref))
    assert torch.equal(q[2:4], torch.full((2,), 7.0) if prev is None else prev[2:4].cpu())  # no amax: not recomputed
    assert (q[6:] == 7.0).all() and (amax == 0).all()


@pytest.mark.parametrize("case", ["scalar-f32-bf16-c12", "vec-f32-bf16-c520"])
def test_gather_folded_scale_update(native_lib, case):
    n_data = 100
    plain = Gather(case, n_data)
    plain.run()
    c = Gather(case, n_data)
    amax = torch.tensor([2.0, 0.0, 0.5], device=DEV)
    qs = torch.full((8,), 7.0, device=DEV)
    c.run(su=(amax, qs, 2.0, 448.0))
    check_scale_update(amax, qs)
    c.check(gather_picks(ROWS_VALID, n_data, *GSEED))
    assert bit_equal(c.out_buf, plain.out_buf)


def test_gather_single_row_and_no_padding(native_lib):
    for case in ("scalar-f32-f32-c4", "vec-f32-bf16-c8"):
        for rows in (1, 5):
            c = Gather(case, 3, rows=rows, rows_valid=rows)
            c.run()
            c.check(gather_picks(rows, 3, *GSEED))


# ------------------------------------------------------------------------------ binding refusals
def test_stage_and_softmax_refuse_mismatched_tensors(native_lib):
    """Three tensors walked with one index: another size or dtype is refused, nothing is launched."""
    ops, spec = torch.ops.pz, PF.epi_spec(PF.ACT_TANH)
    full = lambda n, t=F32: torch.full((n,), 7.0, dtype=t, device=DEV)  # noqa: E731
    g, y, dx = full(257), full(257), full(257)
    calls = [lambda: ops.stage_bwd(g, full(256), dx, spec[0], spec[1]),
             lambda: ops.stage_bwd(g, y, full(256), spec[0], spec[1]),
             lambda: ops.stage_bwd(g, full(257, BF16), dx, spec[0], spec[1]),
             lambda: ops.stage_fwd(g, full(256), spec[0], spec[1]),
             lambda: ops.softmax_rows(g, full(256)),
             lambda: ops.softmax_rows(g, full(257, BF16)),
             lambda: ops.softmax_bwd(full(257, BF16), y, dx),
             lambda: ops.softmax_bwd(g, y, full(257, F64)),
             lambda: ops.softmax_bwd(full(256), y, dx),
             lambda: ops.softmax_bwd(g, y, full(256))]
    for call in calls:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert (dx == 7.0).all() and (y == 7.0).all() and (g == 7.0).all()


def _refused(c, **kw):
    """The call raises before anything is launched: every output keeps its pre-fill."""
    args = dict(indices=None, rows_valid=c.rows_valid, labels_in=c.labels.to(DEV), labels_out=c.lab, picked=c.picked)
    args.update(kw)
    with pytest.raises(RuntimeError):
        torch.ops.pz.gather_rows(c.data, args["indices"], GSEED[0], GSEED[1], c.out, args["rows_valid"],
                                 args["labels_in"], args["labels_out"], args["picked"])
    torch.cuda.synchronize()
    assert (c.out_buf == 7.0).all() and (c.lab == -7).all() and (c.picked == -7).all()


@pytest.mark.parametrize("case", ["scalar-f32-f32-c4", "vec-f32-bf16-c8"])
def test_gather_refuses_bad_optional_tensors(native_lib, case):
    c = Gather(case, 50)
    _refused(c, indices=torch.zeros(ROWS, dtype=torch.int32, device=DEV))
    _refused(c, indices=torch.zeros(ROWS_VALID - 1, dtype=torch.int64, device=DEV))
    _refused(c, indices=torch.zeros(2 * ROWS, dtype=torch.int64, device=DEV)[::2])
    _refused(c, rows_valid=ROWS + 1)
    _refused(c, rows_valid=-1)
    _refused(c, labels_in=None)                      # labels_out without labels_in
    _refused(c, labels_in=c.labels[:49].to(DEV))     # shorter than the table
    _refused(c, labels_out=torch.full((ROWS - 1,), -7, dtype=torch.int64, device=DEV))
    _refused(c, picked=torch.full((ROWS_VALID - 1,), -7, dtype=torch.int64, device=DEV))
    _refused(c, picked=torch.full((ROWS,), -7, dtype=torch.int32, device=DEV))
    c.run()  # and the well-formed call still goes through
    c.check(gather_picks(ROWS_VALID, 50, *GSEED))
