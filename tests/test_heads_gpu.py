"""pz::xent_head and pz::mse_head, raw ops, on every kernel and option, against fp64 torch.

Bounds. fp64 kernels: 1e-12 |ref| + 1e-12. fp32-math kernels (fp32 and bf16 logits; __expf / __logf):
per element 1e-5 x the row's largest |ref| + 1e-12, and 2^-8 |ref| more for a value stored as bf16.
Accumulated outputs (loss, column sums): the same relative factor applied to the fp64 sum of the
absolute values of the terms; for bf16 heads 2^-8 of it more (the separate-pass column sum adds the
stored, rounded gradients). Logits are 3 randn, for which the bound is stated. Zeroed padding rows,
untouched neighbours and everything the deterministic bf16 fold produces are compared bit for bit.

Kernels reached (csrc/elementwise.hip): XENT_CASES names, per case, the kernel the dispatcher picks
for it: xent_head_kernel<f32>, <f64>, <bf16> ("general-*", "wide-*"), xent_head_bf16_kernel<1>, <2>,
<4> ("registerN-*") and all 24 xent_head_lean_kernel<N, COLSUM, OUT8, DROP> ("leanN-*");
mse_head_kernel for f64, f32, bf16; colsum_kernel<f32, f32>, <f64, f64>, <bf16, f32> with and without
the ordered fold (colsum_fold_kernel) — the pairs that mix fp64 with another dtype have no caller
and no test. The float-atomic column sums of PZ_DETERMINISTIC=0 are not run: the switch is read once
per process and the default is what ships.
"""
import numpy as np
import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import bit_equal, keep2d, stage_bwd_reference, stage_fwd_reference, xent_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SEED = (0x2468ACE0, 0x13579BDF)
LID = 5  # layer id of the heads' dropout
U32 = 2.0 ** -24


def acc_dtype(t):
    return F64 if t == F64 else F32


def rel_of(t, accumulated=False):
    if t == F64:
        return 1e-12
    return 1e-5 + (2.0 ** -8 if (t == BF16 and accumulated) else 0.0)


def assert_close(got, ref, scale, what, extra=None):
    """`got` (in its stored dtype) against the fp64 `ref`; `scale`: the fp32-math bound's scale."""
    got64 = got.double().cpu()
    assert torch.isfinite(got64).all(), what
    err = (got64 - ref).abs()
    if got.dtype == F64:
        bound = 1e-12 * ref.abs() + 1e-12
    else:
        bound = 1e-5 * scale + 1e-12 + (2.0 ** -8 * ref.abs() if got.dtype == BF16 else 0.0)
        if extra is not None:
            bound = bound + extra
    worst = (err / bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err/bound {worst:.3f}")
    assert (err <= bound).all(), (what, err.max().item(), worst)


def assert_sum_close(got, ref, abs_sum, t, what, extra=None):
    """An accumulated output against its fp64 value; `abs_sum`: the sum of |term| behind each entry;
    `extra`: the terms' derived absolute allowances, summed."""
    err = (got.double().cpu() - ref).abs()
    bound = rel_of(t, True) * abs_sum + 1e-12 + (0.0 if extra is None or t == F64 else extra)
    worst = (err / bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err/bound {worst:.3f}")
    assert (err <= bound).all(), (what, err.max().item(), worst)


def sliced(rows, cols, pad, dtype, fill=None, gen=None, std=1.0):
    """A [rows, cols] column slice of a buffer pad[0] + pad[1] columns wider: (buffer, view), on the GPU."""
    width = pad[0] + cols + pad[1]
    if fill is not None:
        buf = torch.full((rows, width), fill, dtype=dtype, device=DEV)
    else:
        buf = (std * torch.randn(rows, width, generator=gen, dtype=F64)).to(dtype).to(DEV)
    return buf, buf[:, pad[0]:pad[0] + cols]


def neighbours_kept(buf, pad, cols, fill=7.0):
    return bool((buf[:, :pad[0]] == fill).all() and (buf[:, pad[0] + cols:] == fill).all())


def check_scale_update(amax, qs, prev=None):
    """ScaleUpd with amax = [2, 0, 0.5], headroom 2, maxval 448 over a 7.0-filled qs."""
    q = qs.cpu()
    assert q[0].item() == 112.0 and q[4].item() == 448.0
    for i, v in ((1, 112.0), (5, 448.0)):
        assert abs(np.float64(q[i].item()) - 1.0 / v) <= 2 * np.float64(np.spacing(np.float32(1.0 / v)))
    assert torch.equal(q[2:4], torch.full((2,), 7.0) if prev is None else prev[2:4].cpu())  # no amax: not recomputed
    assert (q[6:] == 7.0).all() and (amax == 0).all()


# -------------------------------------------------------------------------------- cross-entropy
class Xent:
    """One xent_head case: inputs on the GPU (column slices of wider buffers when `pad` says so),
    sentinel-filled outputs, pre-loaded column sums, and the fp64 reference of the stored values."""

    def __init__(self, t, cols, rows=37, rows_valid=33, pad=(0, 0), dh_pad=None, dh=True, probs=False, loss=True,
                 colsum=True, p=0.0, idx_extra=0, epoch=None, out8=False, pad_rows=None):
        g = torch.Generator(device="cpu").manual_seed(1000 * cols + rows)
        self.t, self.cols, self.rows, self.n, self.p = t, cols, rows, rows_valid, p
        self.pad, self.dh_pad = pad, pad if dh_pad is None else dh_pad
        self.lbuf, self.logits = sliced(rows, cols, pad, t, gen=g, std=3.0)
        if pad_rows == "nonfinite":   # padding rows nobody may read: NaN and +inf alternating
            fill = torch.tensor([float("nan"), float("inf")], dtype=t, device=DEV).repeat(cols)[:cols]
            self.logits[rows_valid:] = fill
        elif pad_rows == "zero":
            self.logits[rows_valid:] = 0
        self.labels = torch.randint(0, cols, (rows,), generator=g)
        self.labels[0], self.labels[rows_valid - 1] = 0, cols - 1
        self.dbuf, self.dh = sliced(rows, cols, self.dh_pad, t, fill=7.0) if dh else (None, None)
        self.pbuf, self.probs = sliced(rows, cols, pad, t, fill=7.0) if probs else (None, None)
        A = acc_dtype(t)
        self.loss = torch.zeros(4, dtype=A, device=DEV) if loss else None
        self.cs0 = (0.01 * torch.randn(cols, generator=g, dtype=F64)).to(A)
        self.colsum = self.cs0.clone().to(DEV) if colsum else None
        self.idx_ld = cols + idx_extra if idx_extra else 0
        self.counter = None if epoch is None else torch.tensor([epoch], dtype=torch.int32, device=DEV)
        self.epoch = epoch
        self.spec = PF.epi_spec(drop_pre=LID, p=p, seed=SEED,
                                epoch_ptr=0 if epoch is None else self.counter.data_ptr())
        self.out8 = self.qs8 = self.amax = None
        if out8:
            self.out8 = torch.full((rows, cols), 7, dtype=torch.uint8, device=DEV).view(torch.float8_e5m2)
            self.qs8 = torch.tensor([1024.0, 1.0 / 1024.0], device=DEV)
            self.amax = torch.zeros(1, device=DEV)
        self.scale = 1.0 / rows_valid

    def run(self, su=None):
        kw = {}
        if su is not None:
            kw = dict(su_amax=su[0], su_qs=su[1], su_headroom=2.0, su_maxval=448.0, su_qs_prev=su[2])
        torch.ops.pz.xent_head(self.logits, self.labels.to(DEV), self.n, self.loss, self.scale, self.dh, self.scale,
                               self.colsum, self.probs, self.spec[0], self.spec[1], self.idx_ld, self.out8,
                               None if self.qs8 is None else self.qs8[0:1], self.amax, True, **kw)
        torch.cuda.synchronize()
        return self

    def reference(self):
        keep = None
        if self.p > 0.0:
            keep = keep2d(self.rows, self.cols, self.idx_ld, SEED, LID, self.p, self.epoch)
        return xent_reference(self.logits.cpu(), self.labels, self.n, self.scale, self.scale, keep, 1.0 / (1.0 - self.p))

    def check(self):
        n, t, ref = self.n, self.t, self.reference()
        if self.loss is not None:
            got = self.loss.double().sum().reshape(1)
            want, mag = (torch.tensor([ref[k]], dtype=F64) for k in ("loss", "loss_abs"))
            assert_sum_close(got, want, mag, acc_dtype(t), "loss")
        if self.dh is not None:
            d = ref["dh"][:n]
            assert_close(self.dh[:n], d, d.abs().amax(1, keepdim=True), "dh")
            assert bit_equal(self.dh[n:], torch.zeros_like(self.dh[n:]))  # padding rows: exact zeros
            assert neighbours_kept(self.dbuf, self.dh_pad, self.cols)
        if self.colsum is not None:
            if self.dh is None:
                assert bit_equal(self.colsum.cpu(), self.cs0)  # no gradient, no sums
            else:
                assert_sum_close(self.colsum, self.cs0.double() + ref["colsum"], self.cs0.double().abs() + ref["colsum_abs"],
                                 t, "colsum")
        if self.probs is not None:
            pr = ref["probs"][:n]
            assert_close(self.probs[:n], pr, pr.amax(1, keepdim=True), "probs")
            assert (self.probs[n:] == 7.0).all()  # nothing is written for a padding row
            assert neighbours_kept(self.pbuf, self.pad, self.cols)
        if self.out8 is not None:
            # the e5m2 copy of the STORED bf16 gradient times the scale (a power of two: exact), one rounding
            o8 = self.out8.view(torch.uint8).cpu()
            want = (self.dh.float() * self.qs8[0]).to(torch.float8_e5m2).view(torch.uint8).cpu()
            assert torch.equal(o8[:n], want[:n]) and (o8[n:] == 0).all()
            assert self.amax.item() == self.dh.float().abs().max().item()  # the max of the stored bf16 values
        if self.counter is not None:
            assert self.counter.item() == self.epoch
        return self


STRIDED = (8, 8)   # slices that keep the fast paths' 16-byte alignment (bf16: ld = cols + 16)
ODD_LD = (4, 8)    # a bf16 view with ld % 8 != 0 (and an 8-byte base): the general kernel
XENT_CASES = {
    # ---- xent_head_kernel<float>, <double>, <bf16>
    "general-f32-c27": dict(t=F32, cols=27),
    "general-f32-c70": dict(t=F32, cols=70),
    "general-f64-c27": dict(t=F64, cols=27),
    "general-f64-c70": dict(t=F64, cols=70),
    "general-bf16-c27": dict(t=BF16, cols=27),                    # cols % 8 != 0
    "general-bf16-c2056": dict(t=BF16, cols=2056),                # cols > 2048
    "general-bf16-c520-odd-ld": dict(t=BF16, cols=520, pad=ODD_LD, probs=True, p=0.2),
    "general-f32-c70-probs": dict(t=F32, cols=70, probs=True),
    "general-f32-c27-probs-only": dict(t=F32, cols=27, probs=True, dh=False),
    "general-f64-c27-probs-only": dict(t=F64, cols=27, probs=True, dh=False),
    "general-f32-c70-no-loss": dict(t=F32, cols=70, loss=False),
    "general-f32-c70-no-colsum": dict(t=F32, cols=70, colsum=False),
    "general-f32-c70-strided": dict(t=F32, cols=70, pad=STRIDED, probs=True),
    "general-f64-c27-strided": dict(t=F64, cols=27, pad=STRIDED, probs=True),
    "general-f32-c70-drop-idx-ld": dict(t=F32, cols=70, p=0.2, idx_extra=8),
    "general-f64-c70-drop-idx-ld": dict(t=F64, cols=70, p=0.2, idx_extra=8),
    "general-f32-c27-drop-epoch": dict(t=F32, cols=27, p=0.2, epoch=3),
    # ---- xent_head_bf16_kernel<1>, <2>, <4> (1536 columns: nch == 3 runs <4>)
    "register1-bf16-c8": dict(t=BF16, cols=8),
    "register2-bf16-c520": dict(t=BF16, cols=520),
    "register4-bf16-c1032": dict(t=BF16, cols=1032),
    "register4-bf16-c1536": dict(t=BF16, cols=1536),
    "register1-bf16-c512-probs": dict(t=BF16, cols=512, probs=True),    # probs: the lean kernel is out
    "register2-bf16-c520-probs": dict(t=BF16, cols=520, probs=True),
    "register2-bf16-c520-probs-only": dict(t=BF16, cols=520, probs=True, dh=False),
    "register2-bf16-c520-no-loss": dict(t=BF16, cols=520, loss=False),
    "register2-bf16-c520-no-colsum": dict(t=BF16, cols=520, colsum=False),
    "register2-bf16-c520-strided": dict(t=BF16, cols=520, pad=STRIDED, probs=True),
    "register2-bf16-c520-drop-idx-ld": dict(t=BF16, cols=520, p=0.2, idx_extra=8),
    "register2-bf16-c520-drop-epoch": dict(t=BF16, cols=520, p=0.2, epoch=3),
    "register4-bf16-c1536-drop": dict(t=BF16, cols=1536, p=0.2),
    # ---- xent_head_lean_kernel<1>, <2>, <4> x COLSUM x OUT8 x DROP: all 24 instantiations
    **{f"lean{nch}-bf16-c{512 * nch}{'-colsum' if cs else ''}{'-out8' if o8 else ''}{'-drop' if p else ''}":
       dict(t=BF16, cols=512 * nch, colsum=cs, out8=o8, p=p)
       for nch in (1, 2, 4) for cs in (False, True) for o8 in (False, True) for p in (0.0, 0.2)},
    "lean1-bf16-c512-no-loss": dict(t=BF16, cols=512, loss=False),
    "lean1-bf16-c512-strided": dict(t=BF16, cols=512, pad=STRIDED, p=0.2),
    "lean1-bf16-c512-drop-idx-ld": dict(t=BF16, cols=512, p=0.2, idx_extra=8),
    "lean2-bf16-c1024-drop-epoch": dict(t=BF16, cols=1024, p=0.2, epoch=3),
    "register2-bf16-c520-out8": dict(t=BF16, cols=520, out8=True),
    # ---- more than 16384 columns (8192 in fp64): the column sums are a separate pass over dh
    "wide-f32-c16392": dict(t=F32, cols=16392, rows=5, rows_valid=4),
    "wide-f64-c8200": dict(t=F64, cols=8200, rows=5, rows_valid=4),
    "wide-bf16-c16392": dict(t=BF16, cols=16392, rows=5, rows_valid=4),
    "wide-f32-c16392-sliced-dh": dict(t=F32, cols=16392, rows=5, rows_valid=4, dh_pad=STRIDED),
    "wide-f64-c8200-sliced-dh": dict(t=F64, cols=8200, rows=5, rows_valid=4, dh_pad=STRIDED),
    "wide-bf16-c16392-sliced-dh": dict(t=BF16, cols=16392, rows=5, rows_valid=4, dh_pad=STRIDED),
    # ---- block edges: one row, exactly one block, one row past it
    "general-f32-c27-1row": dict(t=F32, cols=27, rows=1, rows_valid=1),
    "general-f32-c27-17rows": dict(t=F32, cols=27, rows=17, rows_valid=16),
    "register2-bf16-c520-33rows": dict(t=BF16, cols=520, rows=33, rows_valid=32),
    "lean1-bf16-c512-33rows": dict(t=BF16, cols=512, rows=33, rows_valid=33),
    "lean1-bf16-c512-1row": dict(t=BF16, cols=512, rows=1, rows_valid=1),
}


@pytest.mark.parametrize("case", list(XENT_CASES))
def test_xent_head_case(native_lib, case):
    Xent(**XENT_CASES[case]).run().check()


def test_xent_dropout_mask_is_the_layer_mask(native_lib):
    """The reference mask of the dropout cases drops about p of the elements and differs per epoch."""
    k0 = keep2d(37, 520, 528, SEED, LID, 0.2)
    k3 = keep2d(37, 520, 528, SEED, LID, 0.2, epoch=3)
    assert 0.75 < k0.double().mean() < 0.85 and 0.75 < k3.double().mean() < 0.85 and not torch.equal(k0, k3)


@pytest.mark.parametrize("cols,p", [(512, 0.0), (512, 0.2), (520, 0.0)],
                         ids=["lean-c512", "lean-c512-drop", "register-c520"])
def test_xent_deterministic_colsum_fold_two_groups(native_lib, cols, p):
    """549 rows: 18 blocks of 32, so two ticket groups of 16 and 2 blocks, the last block holding 5
    rows. Three launches fold the column sums in the same order: bit-identical, and right."""
    runs = [Xent(BF16, cols, rows=549, rows_valid=545, p=p).run() for _ in range(3)]
    runs[0].check()
    for r in runs[1:]:
        assert bit_equal(r.colsum, runs[0].colsum) and bit_equal(r.dh, runs[0].dh)


@pytest.mark.parametrize("case", ["general-f32-c70", "register2-bf16-c520", "lean1-bf16-c512-colsum-out8"])
def test_xent_padding_rows_are_never_read(native_lib, case):
    """Rows past rows_valid get a zero gradient whatever they hold: NaN / +inf logits there change
    nothing (bf16: bit for bit, the fold is ordered; fp32: within the bound, float atomics)."""
    bad = Xent(pad_rows="nonfinite", **XENT_CASES[case]).run().check()
    zero = Xent(pad_rows="zero", **XENT_CASES[case]).run().check()
    assert torch.isnan(bad.logits[bad.n:, 0]).all() and torch.isinf(bad.logits[bad.n:, 1]).all()
    assert bit_equal(bad.dh, zero.dh)
    if bad.t == BF16:
        assert bit_equal(bad.loss, zero.loss) and bit_equal(bad.colsum, zero.colsum)
    if bad.out8 is not None:
        assert bit_equal(bad.out8.view(torch.uint8), zero.out8.view(torch.uint8)) and bit_equal(bad.amax, zero.amax)


@pytest.mark.parametrize("with_prev", [False, True], ids=["keep", "qs_prev"])
@pytest.mark.parametrize("case", ["general-f32-c27", "register2-bf16-c520", "lean1-bf16-c512-colsum-out8"])
def test_xent_folded_scale_update(native_lib, case, with_prev):
    plain = Xent(**XENT_CASES[case]).run()
    c = Xent(**XENT_CASES[case])
    amax = torch.tensor([2.0, 0.0, 0.5], device=DEV)
    qs = torch.full((8,), 7.0, device=DEV)  # not the record out8_qscale points into
    prev = torch.arange(1.0, 9.0, device=DEV) if with_prev else None
    c.run(su=(amax, qs, prev)).check()
    check_scale_update(amax, qs, prev)
    assert bit_equal(c.dh, plain.dh)
    if c.t == BF16:
        assert bit_equal(c.loss, plain.loss) and bit_equal(c.colsum, plain.colsum)
    if c.out8 is not None:
        assert bit_equal(c.out8.view(torch.uint8), plain.out8.view(torch.uint8))


# ------------------------------------------------------------------------------------------ MSE
class Mse:
    """One mse_head case. y is the stored output of the fp64 reference forward of the epilogue, so the
    derivative from the output means something; y, target and dh are column slices of wider buffers."""

    PAD = (3, 5)

    def __init__(self, t, cols, act=PF.ACT_NONE, p=0.0, rows=37, rows_valid=33, slots=4, dh=True, pad=None,
                 dh_pad=None, idx_extra=6):
        g = torch.Generator(device="cpu").manual_seed(77 * cols + act)
        pad = self.PAD if pad is None else pad
        self.t, self.cols, self.rows, self.n, self.act, self.p = t, cols, rows, rows_valid, act, p
        self.pad, self.dh_pad = pad, pad if dh_pad is None else dh_pad
        self.idx_ld = cols + idx_extra
        self.keep = keep2d(rows, cols, self.idx_ld, SEED, LID, p) if p > 0.0 else None
        self.sc = 1.0 / (1.0 - p)
        x = 1.5 * torch.randn(rows, cols, generator=g, dtype=F64)
        y = stage_fwd_reference(x, act, None, self.keep, torch.tensor(self.sc, dtype=F64)).to(t)
        self.ybuf, self.y = sliced(rows, cols, pad, t, gen=g)
        self.y.copy_(y)
        self.tbuf, self.target = sliced(rows, cols, pad, t, gen=g)
        self.dbuf, self.dh = sliced(rows, cols, self.dh_pad, t, fill=7.0) if dh else (None, None)
        A = acc_dtype(t)
        self.loss0 = (0.5 + torch.rand(slots, generator=g, dtype=F64)).to(A)
        self.cs0 = (0.01 * torch.randn(cols, generator=g, dtype=F64)).to(A)
        self.loss, self.colsum = self.loss0.clone().to(DEV), self.cs0.clone().to(DEV)
        self.spec = PF.epi_spec(act, drop_post=LID, p=p, seed=SEED)
        self.scale = 1.0 / (rows_valid * cols)

    def run(self):
        torch.ops.pz.mse_head(self.y, self.target, self.n, self.loss, self.scale, self.dh, self.scale, self.colsum,
                              self.spec[0], self.spec[1], self.idx_ld)
        torch.cuda.synchronize()
        return self

    def check(self):
        """dh against epi_bwd(2 (y - t) grad_scale, y). sigmoid / tanh take their derivative from the
        stored output, fl(a fl(1 - a)) or fl(1 - fl(a a)) with a = fl(y (1 - p)): at most 4 u off
        absolutely (u = 2^-24) however small the derivative, so the bound gains 4 u |2 (y - t)
        grad_scale| scale (see test_stage_softmax_gather_gpu.check_stage_bwd)."""
        n, t = self.n, self.t
        y, tg = self.y.double().cpu(), self.target.double().cpu()
        d = y[:n] - tg[:n]
        terms = d * d * self.scale
        # loss slots pre-loaded: the kernel adds. Their own magnitude is part of the sum's terms.
        assert_sum_close(self.loss.double().sum().reshape(1), (self.loss0.double().sum() + terms.sum()).reshape(1),
                         (self.loss0.double().sum() + terms.sum()).reshape(1), acc_dtype(t), "loss")
        if self.dh is None:
            assert bit_equal(self.colsum.cpu(), self.cs0)
            return self
        g = 2.0 * d * self.scale
        keep = None if self.keep is None else self.keep[:n]
        ref = stage_bwd_reference(g, y[:n], self.act, None, keep, self.sc)
        extra = 4 * U32 * g.abs() * self.sc if self.act in (PF.ACT_SIGMOID, PF.ACT_TANH) else None
        assert_close(self.dh[:n], ref, ref.abs().amax(1, keepdim=True), "dh", extra)
        assert bit_equal(self.dh[n:], torch.zeros_like(self.dh[n:]))
        assert neighbours_kept(self.dbuf, self.dh_pad, self.cols)
        assert_sum_close(self.colsum, self.cs0.double() + ref.sum(0), self.cs0.double().abs() + ref.abs().sum(0), t,
                         "colsum", None if extra is None else extra.sum(0))
        return self


MSE_EPI = {"none": (PF.ACT_NONE, 0.0), "sigmoid": (PF.ACT_SIGMOID, 0.0), "tanh": (PF.ACT_TANH, 0.0),
           "relu": (PF.ACT_RELU, 0.0), "sigmoid-drop": (PF.ACT_SIGMOID, 0.25)}


@pytest.mark.parametrize("slots", [1, 4])
@pytest.mark.parametrize("epi", list(MSE_EPI))
@pytest.mark.parametrize("cols", [10, 70])
@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
def test_mse_head_epilogues(native_lib, t, cols, epi, slots):
    act, p = MSE_EPI[epi]
    Mse(t, cols, act, p, slots=slots).run().check()


@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
def test_mse_head_loss_only(native_lib, t):
    Mse(t, 70, PF.ACT_SIGMOID, 0.25, dh=False).run().check()


@pytest.mark.parametrize("dh_pad", [(0, 0), (8, 8)], ids=["dense-dh", "sliced-dh"])
@pytest.mark.parametrize("t,cols", [(F64, 8200), (F32, 16392)], ids=["f64-c8200", "f32-c16392"])
def test_mse_head_wide_rows_separate_colsum_pass(native_lib, t, cols, dh_pad):
    Mse(t, cols, PF.ACT_TANH, rows=5, rows_valid=4, pad=(0, 0), dh_pad=dh_pad).run().check()


def test_mse_head_contiguous_single_block(native_lib):
    for rows, n in ((1, 1), (16, 16), (17, 16)):
        Mse(F32, 10, PF.ACT_RELU, rows=rows, rows_valid=n, pad=(0, 0), idx_extra=0).run().check()


# ------------------------------------------------------------------------------ binding refusals
def test_mse_head_refuses_bad_optional_tensors(native_lib):
    m = Mse(BF16, 10)

    def refused(**kw):
        a = dict(dh=m.dh, rows_valid=m.n, loss=m.loss, colsum=m.colsum, target=m.target)
        a.update(kw)
        with pytest.raises(RuntimeError):
            torch.ops.pz.mse_head(m.y, a["target"], a["rows_valid"], a["loss"], m.scale, a["dh"], m.scale, a["colsum"],
                                  m.spec[0], m.spec[1], m.idx_ld)
        torch.cuda.synchronize()
        for o in (a["dh"], m.dh):
            assert (o == 7.0).all()
        assert bit_equal(m.loss.cpu(), m.loss0) and bit_equal(m.colsum.cpu(), m.cs0)

    refused(dh=torch.full((37, 10), 7.0, dtype=F32, device=DEV))       # would be written as bf16
    refused(dh=torch.full((36, 10), 7.0, dtype=BF16, device=DEV))
    refused(dh=torch.full((37, 20), 7.0, dtype=BF16, device=DEV)[:, ::2])
    refused(rows_valid=38)
    refused(rows_valid=-1)
    refused(colsum=torch.zeros(9, device=DEV))
    refused(loss=torch.zeros(8, device=DEV)[::2])
    refused(target=m.target[:32])
    m.run().check()


@pytest.mark.parametrize("case", ["general-f32-c70-probs", "register2-bf16-c520-probs"])
def test_xent_head_refuses_bad_optional_tensors(native_lib, case):
    c = Xent(**XENT_CASES[case])
    t, cols = c.t, c.cols
    other = F32 if t == BF16 else BF16

    def refused(**kw):
        a = dict(labels=c.labels.to(DEV), rows_valid=c.n, loss=c.loss, dh=c.dh, colsum=c.colsum, probs=c.probs)
        a.update(kw)
        with pytest.raises(RuntimeError):
            torch.ops.pz.xent_head(c.logits, a["labels"], a["rows_valid"], a["loss"], c.scale, a["dh"], c.scale,
                                   a["colsum"], a["probs"], c.spec[0], c.spec[1], 0)
        torch.cuda.synchronize()
        for o in (a["dh"], a["probs"], c.dh, c.probs):
            assert (o == 7.0).all()
        assert (c.loss == 0).all() and bit_equal(c.colsum.cpu(), c.cs0)

    refused(labels=c.labels[:c.n - 1].to(DEV))
    refused(labels=c.labels.to(torch.int32).to(DEV))
    refused(colsum=torch.zeros(cols - 1, device=DEV))
    refused(rows_valid=c.rows + 1)
    refused(rows_valid=-1)
    refused(dh=torch.full((c.rows, cols), 7.0, dtype=other, device=DEV))
    refused(dh=torch.full((c.rows - 1, cols), 7.0, dtype=t, device=DEV))
    refused(probs=torch.full((c.rows, cols - 1), 7.0, dtype=t, device=DEV))
    refused(probs=torch.full((c.rows, 2 * cols), 7.0, dtype=t, device=DEV)[:, ::2])
    refused(loss=torch.zeros(4, dtype=F64, device=DEV))
    c.run().check()


# ------------------------------------------------------------------- column sums (pz::colsum)
@pytest.mark.parametrize("rows", [5, 300], ids=["r5", "r300"])
@pytest.mark.parametrize("t", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
def test_colsum_accumulates_in_block_order(native_lib, t, rows):
    """out[c] += sum_r x[r][c] over 70 columns (two 64-column strips) and, at 300 rows, two 256-row
    parts whose partial rows are folded in order: three launches agree bit for bit."""
    g = torch.Generator(device="cpu").manual_seed(rows)
    x = torch.randn(rows, 70, generator=g, dtype=F64).to(t)
    out0 = torch.randn(70, generator=g, dtype=F64).to(acc_dtype(t))
    outs = []
    for _ in range(3):
        out = out0.clone().to(DEV)
        torch.ops.pz.colsum(x.to(DEV), out)
        torch.cuda.synchronize()
        outs.append(out)
    # the inputs are exact: only the fp32 additions err (accumulated=False: no bf16 store anywhere)
    err = (outs[0].double().cpu() - (out0.double() + x.double().sum(0))).abs()
    assert (err <= rel_of(t) * (out0.double().abs() + x.double().abs().sum(0)) + 1e-12).all(), err.max().item()
    assert bit_equal(outs[1], outs[0]) and bit_equal(outs[2], outs[0])
