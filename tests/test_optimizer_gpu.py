"""pz::optimizer_step, pz::segment_stats and pz::step_finalize against plain fp64 references.

The raw ops are driven over a hand-built flat layout (no ParamStore), so that one launch holds a
vectorised multi-block weight, a scalar-path multi-block weight, a vectorised bias and a scalar
bias, with random values in the padding gaps that no launch may touch.
"""
import math

import pytest
import torch

from tests.helpers import bit_equal, opt_update_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"

ELEMS_PER_BLOCK = 4096  # kOptElemsPerBlock
# (shape, is_weight): vector path 3 blocks / scalar path 2 blocks, tail of 29 / vector path, 25
# vectors / scalar path / a segment that no launch lists
SHAPES = [((96, 100), 1), ((33, 125), 1), ((100,), 0), ((7,), 0), ((130,), 0)]
W_VEC, W_SCA, B_VEC, B_SCA, SPARE = range(5)
LAUNCHED = [W_VEC, W_SCA, B_VEC, B_SCA]
# every term matters: eps is ~1 % of sqrt(v) / bc2s, the L2 term and the gradient scale are on
HP = dict(lr=0.01, b1=0.9, b2=0.99, eps=1e-3, bc1=1 - 0.9 ** 3, bc2s=math.sqrt(1 - 0.99 ** 3), grad_scale=0.5,
          l2=1e-3)
STATE = ("params", "grads", "m", "v")


class Flat:
    """Flat master / gradient / moment buffers with 64-aligned segments; `*0` are the CPU originals."""

    def __init__(self, dtype, seed=0):
        self.dtype = dtype
        self.numels = [math.prod(s) for s, _ in SHAPES]
        self.is_weight = [w for _, w in SHAPES]
        self.offsets, off = [], 0
        for n in self.numels:
            self.offsets.append(off)
            off = (off + n + 63) // 64 * 64
        self.total = off + 64
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.params0 = torch.randn(self.total, generator=g, dtype=torch.float64).to(dtype)
        self.grads0 = torch.randn(self.total, generator=g, dtype=torch.float64).to(dtype)
        self.m0 = (0.01 * torch.randn(self.total, generator=g, dtype=torch.float64)).to(dtype)
        self.v0 = (1e-4 + 1e-3 * torch.rand(self.total, generator=g, dtype=torch.float64)).to(dtype)
        for k in STATE:
            setattr(self, k, getattr(self, k + "0").clone().to(DEV))

    def seg(self, i, lo=0, n=None):
        """Flat slice of elements [lo, lo + n) of segment i (n = None: to its end)."""
        n = self.numels[i] - lo if n is None else n
        return slice(self.offsets[i] + lo, self.offsets[i] + lo + n)

    def poison_grads(self, sl):
        """NaN fp32 gradients: a launch that reads them cannot pass."""
        self.grads0[sl] = float("nan")
        self.grads[sl] = self.grads0[sl].to(DEV)

    def index(self, ranges):
        """(flat element indices, L2 mask) of the launched ranges [(segment, lo, numel)]."""
        idx = torch.cat([torch.arange(self.offsets[i] + lo, self.offsets[i] + lo + n) for i, lo, n in ranges])
        wt = torch.cat([torch.full((n,), bool(self.is_weight[i])) for i, lo, n in ranges])
        return idx, wt

    def assert_rest_untouched(self, ranges, skip=()):
        idx, _ = self.index(ranges)
        rest = torch.ones(self.total, dtype=torch.bool)
        rest[idx] = False
        for k in STATE:
            if k not in skip:
                assert bit_equal(getattr(self, k).cpu()[rest], getattr(self, k + "0")[rest]), k


def whole(fl, segs=LAUNCHED):
    return [(i, 0, fl.numels[i]) for i in segs]


def launch(fl, ranges, *, adam=True, hp=HP, shadows=None, grads16=None, zero_grad=None, amax=None, w8=None,
           slots=None, stats=None, table=None, epoch=None, stats_every=1, max_grid=0, moments=True):
    """One pz::optimizer_step over `ranges`; the per-range extras are dicts keyed by position."""
    n = len(ranges)
    pick = lambda d: [None if d is None else d.get(k) for k in range(n)]  # noqa: E731
    w8 = w8 or {}
    numels = [r[2] for r in ranges]
    blocks = [max(1, math.ceil(x / ELEMS_PER_BLOCK)) for x in numels]
    starts = [sum(blocks[:k]) for k in range(n)]
    pack = torch.ops.pz.pack_segments(
        [fl.offsets[i] + lo for i, lo, _ in ranges], numels, [fl.is_weight[i] for i, _, _ in ranges],
        [-1] * n if slots is None else slots, pick(shadows), pick(grads16), [0] * n if zero_grad is None else zero_grad,
        pick(amax), [w8[k][0] if k in w8 else None for k in range(n)],
        [w8[k][1] if k in w8 else None for k in range(n)], [w8[k][2] if k in w8 else None for k in range(n)]).to(DEV)
    block_seg = torch.tensor(starts, dtype=torch.int64, device=DEV)
    use_m = adam or moments
    torch.ops.pz.optimizer_step(fl.params, fl.grads, fl.m if use_m else None, fl.v if use_m else None, pack, block_seg,
                                n, sum(blocks), adam, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["bc1"], hp["bc2s"],
                                hp["grad_scale"], hp["l2"], stats, table, epoch, stats_every, max_grid)
    torch.cuda.synchronize()
    return sum(blocks)


def check_update(fl, ranges, *, adam=True, hp=HP, graw=None, label=""):
    """params / m / v of the launched ranges against the fp64 formula. fp32 masters: within
    4 max|fp32 formula - fp64 formula| + 2^-23 |ref| (the factor covers FMA contraction and the
    sqrt / div roundings torch and the kernel do not share); fp64 masters: 1e-12."""
    idx, wt = fl.index(ranges)
    graw = fl.grads0[idx] if graw is None else graw
    args = (fl.params0[idx], graw, fl.m0[idx], fl.v0[idx], wt)
    ref = opt_update_reference(*(a.double() if a.is_floating_point() else a for a in args), torch.float64, adam=adam,
                               **hp)
    got = [fl.params.cpu()[idx], fl.m.cpu()[idx], fl.v.cpu()[idx]]
    if not adam:
        assert bit_equal(got[1], fl.m0[idx]) and bit_equal(got[2], fl.v0[idx])  # SGD has no moments
        ref, got = ref[:1], got[:1]
    if fl.dtype == torch.float64:
        for r, x in zip(ref, got):
            torch.testing.assert_close(x, r, rtol=1e-12, atol=1e-12)
        return
    f32 = opt_update_reference(*args, torch.float32, adam=adam, **hp)
    for name, r, x, f in zip("pmv", ref, got, f32):
        e = (f.double() - r).abs().max().item()
        err = (x.double() - r).abs()
        print(f"optimizer_step fp32 {label} {name}: max|kernel - fp64| = {err.max().item():.3e}, "
              f"max|fp32 formula - fp64| = {e:.3e}")
        assert (err <= 4 * e + 2.0 ** -23 * r.abs()).all(), (name, err.max().item(), e)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("adam", [True, False])
def test_update_matches_fp64_formula(native_lib, dtype, adam):
    """Adam / SGD over the vector and scalar paths, several blocks per segment.

    Measured on MI355X (fp32 masters), max|kernel - fp64| next to max|fp32 formula - fp64|, of which
    the bound allows 4: Adam p 1.712e-07 / 1.712e-07, m 5.546e-08 / 5.546e-08, v 3.646e-08 /
    4.019e-08; SGD p 1.195e-07 / 1.192e-07."""
    fl = Flat(dtype, seed=1)
    assert launch(fl, whole(fl), adam=adam, moments=False) == 7
    check_update(fl, whole(fl), adam=adam, label="adam" if adam else "sgd")
    fl.assert_rest_untouched(whole(fl))
    assert bit_equal(fl.grads.cpu(), fl.grads0)
    if not adam:  # moments that are passed to SGD stay as they are
        fl = Flat(dtype, seed=1)
        launch(fl, whole(fl), adam=False, moments=True)
        check_update(fl, whole(fl), adam=False, label="sgd+moments")
        assert bit_equal(fl.m.cpu(), fl.m0) and bit_equal(fl.v.cpu(), fl.v0)


def test_bf16_gradients_replace_fp32_gradients(native_lib):
    fl = Flat(torch.float32, seed=2)
    g = torch.Generator(device="cpu").manual_seed(20)
    g16 = {k: torch.randn(fl.numels[k], generator=g).to(torch.bfloat16) for k in (W_VEC, W_SCA)}
    dev16 = {k: t.to(DEV) for k, t in g16.items()}
    for k in g16:  # the fp32 gradients of these segments must not be read
        fl.poison_grads(fl.seg(k))
    launch(fl, whole(fl), grads16=dev16)
    graw = torch.cat([g16[k].float() if k in g16 else fl.grads0[fl.seg(k)] for k in LAUNCHED])
    check_update(fl, whole(fl), graw=graw, label="grad16")
    fl.assert_rest_untouched(whole(fl))
    assert bit_equal(fl.grads.cpu(), fl.grads0)
    for k in g16:
        assert bit_equal(dev16[k].cpu(), g16[k])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("flags", [[1, 0, 0, 1], [0, 1, 1, 0]])
def test_zero_grad_clears_flagged_segments_only(native_lib, dtype, flags):
    fl = Flat(dtype, seed=3)
    launch(fl, whole(fl), zero_grad=flags)
    check_update(fl, whole(fl), label="zero_grad")
    grads = fl.grads.cpu()
    for k, f in zip(LAUNCHED, flags):
        if f:
            assert (grads[fl.seg(k)] == 0).all(), k
        else:
            assert bit_equal(grads[fl.seg(k)], fl.grads0[fl.seg(k)]), k
    fl.assert_rest_untouched(whole(fl))


def test_zero_grad_with_bf16_gradients_updates_from_them(native_lib):
    fl = Flat(torch.float32, seed=4)
    g = torch.Generator(device="cpu").manual_seed(40)
    g16 = {k: torch.randn(fl.numels[k], generator=g).to(torch.bfloat16) for k in (W_VEC, W_SCA)}
    launch(fl, whole(fl), grads16={k: t.to(DEV) for k, t in g16.items()}, zero_grad=[1, 1, 1, 0])
    graw = torch.cat([g16[k].float() if k in g16 else fl.grads0[fl.seg(k)] for k in LAUNCHED])
    check_update(fl, whole(fl), graw=graw, label="grad16+zero_grad")
    grads = fl.grads.cpu()  # (nothing is asserted about the fp32 gradients behind a grad16)
    assert (grads[fl.seg(B_VEC)] == 0).all() and bit_equal(grads[fl.seg(B_SCA)], fl.grads0[fl.seg(B_SCA)])
    fl.assert_rest_untouched(whole(fl), skip=("grads",))


def _shadows(fl, dtypes):
    return {k: torch.full((fl.numels[k],), 7.0, device=DEV, dtype=dt) for k, dt in dtypes.items()}


def _assert_shadows(fl, sh):
    for k, t in sh.items():
        assert torch.equal(t, fl.params[fl.seg(k)].float().to(t.dtype)), k


def test_shadows_are_the_rounded_new_parameters(native_lib):
    fl = Flat(torch.float32, seed=5)
    sh = _shadows(fl, {W_VEC: torch.bfloat16, W_SCA: torch.bfloat16, B_VEC: torch.float32})
    launch(fl, whole(fl), shadows=sh)
    check_update(fl, whole(fl), label="shadows")
    _assert_shadows(fl, sh)
    fl.assert_rest_untouched(whole(fl))


def test_fp64_master_writes_its_shadows_on_both_paths(native_lib):
    """The double2 vector path used to skip the shadow (and e4m3) stores that the scalar path
    performs: an aligned fp64 segment kept its stale low-precision copy."""
    fl = Flat(torch.float64, seed=6)
    sh = _shadows(fl, {W_VEC: torch.float32, W_SCA: torch.float32, B_VEC: torch.bfloat16, B_SCA: torch.bfloat16})
    launch(fl, whole(fl), shadows=sh)
    check_update(fl, whole(fl))
    _assert_shadows(fl, sh)
    fl.assert_rest_untouched(whole(fl))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("start", [0.0, 100.0])
def test_amax_is_max_abs_of_new_parameters(native_lib, dtype, start):
    fl = Flat(dtype, seed=7)
    amax = {k: torch.full((1,), start, device=DEV) for k in LAUNCHED}
    launch(fl, whole(fl), amax=amax)
    check_update(fl, whole(fl), label="amax")
    for k in LAUNCHED:
        want = max(start, fl.params[fl.seg(k)].float().abs().max().item())
        assert amax[k].item() == want, (k, amax[k].item(), want)
    fl.assert_rest_untouched(whole(fl))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("amax_prev", [3.0, 0.0])
def test_e4m3_copy_uses_the_delayed_scale(native_lib, dtype, amax_prev):
    """q = 448 / amax_prev (some |w| > amax_prev: the copy saturates), or the recorded q when no
    amax was reduced yet. One fp32 product and one RNE cast on both sides: no mismatch."""
    fl = Flat(dtype, seed=8)
    w8 = {}
    for k in (W_VEC, W_SCA, B_VEC):
        w8[k] = (torch.zeros(fl.numels[k], device=DEV, dtype=torch.uint8).view(torch.float8_e4m3fn),
                 torch.full((1,), amax_prev, device=DEV), torch.tensor([100.0, -1.0], device=DEV))
    launch(fl, whole(fl), w8=w8)
    check_update(fl, whole(fl), label="w8")
    q_want = 448.0 / amax_prev if amax_prev > 0 else 100.0
    for k, (q8, prev, qs) in w8.items():
        q, qi = qs.tolist()
        assert abs(q - q_want) <= 1e-6 * q_want and abs(qi - 1.0 / q_want) <= 1e-6 / q_want, (q, qi)
        assert prev.item() == amax_prev
        want = (fl.params[fl.seg(k)].float().cpu() * torch.tensor(q)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        assert (want.view(torch.uint8) != q8.cpu().view(torch.uint8)).sum().item() == 0, k
    if amax_prev > 0:
        assert fl.params[fl.seg(W_VEC)].abs().max().item() > amax_prev  # the clamp is exercised
    fl.assert_rest_untouched(whole(fl))


SLOTS = [0, 1, 1, -1]  # two segments share slot 1, the last bias adds nothing; slot 2 stays unused
NSLOTS = 3


def _stats_buffer(seed):
    """fp64 stats as a view inside a larger buffer, so that a bad slot index stays in owned memory."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    big = torch.randn(8 + 4 * NSLOTS + 8, generator=g, dtype=torch.float64).to(DEV)
    return big, big[8:8 + 4 * NSLOTS]


def _stats_reference(fl):
    ref = torch.zeros(NSLOTS, 4, dtype=torch.float64)
    p1, p0 = fl.params.cpu(), fl.params0
    for k, slot in zip(LAUNCHED, SLOTS):
        if slot < 0:
            continue
        d = (p1[fl.seg(k)] - p0[fl.seg(k)]).double()  # subtracted in the master dtype, as the kernel does
        w = p1[fl.seg(k)].double()
        ref[slot] += torch.stack([d.sum(), (d * d).sum(), w.sum(), (w * w).sum()])
    return ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("every,epoch,full", [(1, None, True), (0, None, False), (2, 4, True), (2, 5, False)])
def test_statistics_accumulate_per_slot(native_lib, dtype, every, epoch, full):
    fl = Flat(dtype, seed=9)
    big, stats = _stats_buffer(90)
    before = big.cpu().clone()
    ctr = None if epoch is None else torch.tensor([epoch], dtype=torch.int32, device=DEV)
    launch(fl, whole(fl), slots=SLOTS, stats=stats, epoch=ctr, stats_every=every)
    check_update(fl, whole(fl), label="stats")
    after = big.cpu()
    assert bit_equal(after[:8], before[:8]) and bit_equal(after[-8:], before[-8:])
    b, a, ref = before[8:-8].view(NSLOTS, 4), after[8:-8].view(NSLOTS, 4), _stats_reference(fl)
    assert bit_equal(a[2], b[2])
    if full:
        torch.testing.assert_close(a[:2], b[:2] + ref[:2], rtol=1e-9, atol=1e-9)
    else:
        assert bit_equal(a[:2, :3], b[:2, :3])
        torch.testing.assert_close(a[:2, 3], b[:2, 3] + ref[:2, 3], rtol=1e-9, atol=1e-9)
    if ctr is not None:
        assert ctr.item() == epoch
    fl.assert_rest_untouched(whole(fl))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("adam", [True, False])
def test_hp_table_row_of_the_device_epoch_overrides_the_scalars(native_lib, dtype, adam):
    fl = Flat(dtype, seed=10)
    rows = [[0.01 * (r + 1), 1 - 0.9 ** (r + 1), math.sqrt(1 - 0.99 ** (r + 1)), 0.0] for r in range(6)]
    table = torch.tensor(rows, dtype=torch.float64, device=DEV)
    ctr = torch.tensor([3], dtype=torch.int32, device=DEV)  # inside the table: the kernel does not bound-check
    wrong = dict(HP, lr=1.0, bc1=0.5, bc2s=0.5)
    launch(fl, whole(fl), adam=adam, hp=wrong, table=table, epoch=ctr)
    check_update(fl, whole(fl), adam=adam, hp=dict(HP, lr=rows[3][0], bc1=rows[3][1], bc2s=rows[3][2]), label="hp")
    assert ctr.item() == 3 and torch.equal(table.cpu(), torch.tensor(rows, dtype=torch.float64))
    fl.assert_rest_untouched(whole(fl))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_capped_grid_computes_the_same(native_lib, dtype):
    out = []
    for max_grid in (0, 2):  # 2 workgroups loop over the 7 work blocks
        fl = Flat(dtype, seed=11)
        sh = _shadows(fl, {W_VEC: torch.bfloat16, W_SCA: torch.bfloat16, B_VEC: torch.float32})
        amax = {k: torch.zeros(1, device=DEV) for k in LAUNCHED}
        big, stats = _stats_buffer(110)
        launch(fl, whole(fl), shadows=sh, amax=amax, slots=SLOTS, stats=stats, max_grid=max_grid)
        fl.assert_rest_untouched(whole(fl))
        out.append((fl, sh, amax, big.cpu()))
    (f0, s0, a0, st0), (f1, s1, a1, st1) = out
    check_update(f0, whole(f0), label="max_grid")
    for k in ("params", "m", "v"):
        assert bit_equal(getattr(f0, k).cpu(), getattr(f1, k).cpu()), k
    for k in s0:
        assert bit_equal(s0[k].cpu(), s1[k].cpu()), k
    for k in a0:
        assert a0[k].item() == a1[k].item()
    torch.testing.assert_close(st1, st0, rtol=1e-12, atol=0.0)  # the double atomics only reorder


def test_slice_group_updates_only_its_range(native_lib):
    """What FusedOptimizer.define_slice packs: a one-segment table whose offset lies inside a weight,
    with the gradient and the shadow indexed from 0 of the slice."""
    fl = Flat(torch.float32, seed=12)
    lo, n = ELEMS_PER_BLOCK + 64, 2048
    g = torch.Generator(device="cpu").manual_seed(120)
    g16 = torch.randn(n, generator=g).to(torch.bfloat16)
    shadow = torch.full((n,), 7.0, device=DEV, dtype=torch.bfloat16)
    fl.poison_grads(fl.seg(W_VEC, lo, n))
    big, stats = _stats_buffer(121)
    before = big.cpu().clone()
    ranges = [(W_VEC, lo, n)]
    assert launch(fl, ranges, shadows={0: shadow}, grads16={0: g16.to(DEV)}, slots=[1], stats=stats) == 1
    check_update(fl, ranges, graw=g16.float(), label="slice")
    fl.assert_rest_untouched(ranges)
    assert bit_equal(fl.grads.cpu(), fl.grads0)
    assert torch.equal(shadow, fl.params[fl.seg(W_VEC, lo, n)].to(torch.bfloat16))
    after = big.cpu()
    slot1 = torch.zeros_like(before, dtype=torch.bool)
    slot1[8 + 4:8 + 8] = True
    assert bit_equal(after[~slot1], before[~slot1])
    p1, p0 = fl.params.cpu()[fl.seg(W_VEC, lo, n)], fl.params0[fl.seg(W_VEC, lo, n)]
    d, w = (p1 - p0).double(), p1.double()  # the slice's own sums, in the whole weight's slot
    ref = torch.stack([d.sum(), (d * d).sum(), w.sum(), (w * w).sum()])
    torch.testing.assert_close(after[slot1], before[slot1] + ref, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_segment_stats_sums_the_weights(native_lib, dtype):
    fl = Flat(dtype, seed=13)
    big, stats = _stats_buffer(130)
    before = big.cpu().clone()
    pack = torch.ops.pz.pack_segments([fl.offsets[k] for k in LAUNCHED], [fl.numels[k] for k in LAUNCHED],
                                      [fl.is_weight[k] for k in LAUNCHED], SLOTS, [None] * 4, [None] * 4, [0] * 4,
                                      [None] * 4, [None] * 4, [None] * 4, [None] * 4).to(DEV)
    block_seg = torch.tensor([0, 3, 5, 6], dtype=torch.int64, device=DEV)
    torch.ops.pz.segment_stats(fl.params, pack, block_seg, 4, 7, stats)
    torch.cuda.synchronize()
    after = big.cpu()
    assert bit_equal(after[:8], before[:8]) and bit_equal(after[-8:], before[-8:])
    b, a = before[8:-8].view(NSLOTS, 4), after[8:-8].view(NSLOTS, 4)
    ref = torch.zeros(NSLOTS, 2, dtype=torch.float64)
    for k, slot in zip(LAUNCHED, SLOTS):
        if slot >= 0:
            w = fl.params0[fl.seg(k)].double()
            ref[slot] += torch.stack([w.sum(), (w * w).sum()])
    assert bit_equal(a[:, :2], b[:, :2]) and bit_equal(a[2], b[2])
    torch.testing.assert_close(a[:2, 2:], b[:2, 2:] + ref[:2], rtol=1e-12, atol=1e-12)
    assert bit_equal(fl.params.cpu(), fl.params0)


# ------------------------------------------------------------------------------ step_finalize
FIN_SLOTS = 70  # more than the 64 threads of the launch: the stride loops run twice


def _std_from_sums(s, ss, n):
    var = ((ss - s * s / n) / (n - 1.0)).clamp_min(0.0)
    return torch.where(n < 2, torch.full_like(s, float("nan")), var.sqrt())


class Fin:
    """Inputs of one pz::step_finalize launch; costs and ratios are leading views of larger tensors."""

    def __init__(self, loss_dtype, n_costs=12, n_rows=4, seed=0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        numel = torch.randint(2, 400, (FIN_SLOTS,), generator=g).double()
        numel[5] = 1.0  # std of one element: NaN, as the kernel defines it
        cur = torch.empty(FIN_SLOTS, 4, dtype=torch.float64)
        for k in range(FIN_SLOTS):
            n = int(numel[k])
            d = 1e-3 * torch.randn(n, generator=g, dtype=torch.float64)
            w = torch.randn(n, generator=g, dtype=torch.float64) + 0.1
            cur[k] = torch.stack([d.sum(), (d * d).sum(), w.sum(), (w * w).sum()])
        cur[9, 1] = cur[9, 0] ** 2 / numel[9] * (1 - 1e-3)  # a negative variance clamps to 0
        self.numel, self.cur = numel, cur
        self.prev = torch.rand(FIN_SLOTS, 4, generator=g, dtype=torch.float64) * 50
        self.loss = (torch.rand(4, generator=g, dtype=torch.float64) * 3).to(loss_dtype)
        self.n_costs, self.n_rows = n_costs, n_rows
        self.costs_big = torch.full((n_costs + 6,), -5.0, dtype=torch.float64, device=DEV)
        self.ratios_big = torch.full(((n_rows + 2) * FIN_SLOTS,), -5.0, device=DEV)
        self.costs = self.costs_big[:n_costs]
        self.ratios = self.ratios_big[:n_rows * FIN_SLOTS]
        self.d_numel, self.d_cur, self.d_prev, self.d_loss = (t.to(DEV) for t in (numel, cur, self.prev, self.loss))
        self.clear = torch.full((5,), 3.0, device=DEV)

    def run(self, epoch, ratio_row, ctr=None, every=1, loss_div=2.0, l2=1e-3):
        self.loss_div, self.l2 = loss_div, l2
        torch.ops.pz.step_finalize(self.d_loss, loss_div, self.d_prev.view(-1), self.d_cur.view(-1), self.d_numel,
                                   FIN_SLOTS, l2, self.costs, epoch, self.ratios, ratio_row, ctr, every, self.clear)
        torch.cuda.synchronize()

    def check(self, cost_at, row):
        """costs / ratios hold exactly the entries `cost_at` / `row` (None: nothing written)."""
        costs = torch.full((self.n_costs + 6,), -5.0, dtype=torch.float64)
        if cost_at is not None:
            costs[cost_at] = self.loss.double().sum() / self.loss_div + self.l2 * self.prev[:, 3].sum()
        got = self.costs_big.cpu()
        keep = torch.ones_like(costs, dtype=torch.bool)
        if cost_at is not None:
            keep[cost_at] = False
            torch.testing.assert_close(got[cost_at], costs[cost_at], rtol=1e-12, atol=0.0)
        assert bit_equal(got[keep], costs[keep])
        ratios = torch.full(((self.n_rows + 2), FIN_SLOTS), -5.0)
        got_r = self.ratios_big.cpu().view(self.n_rows + 2, FIN_SLOTS)
        if row is not None:
            c = self.cur
            sd, sw = _std_from_sums(c[:, 0], c[:, 1], self.numel), _std_from_sums(c[:, 2], c[:, 3], self.numel)
            ratios[row] = (sd / (sw + 1e-8)).float()
            assert torch.isnan(ratios[row, 5]) and ratios[row, 9] == 0
        assert torch.equal(torch.isnan(got_r), torch.isnan(ratios))
        # the same correctly rounded fp64 operations on both sides, then one cast to fp32: equal
        print("step_finalize ratios: max|kernel - ref| =", (got_r - ratios).abs().nan_to_num(0.0).max().item())
        assert torch.equal(got_r.nan_to_num(-1.0), ratios.nan_to_num(-1.0))
        # reset and advance
        assert (self.d_loss == 0).all() and (self.d_prev == 0).all() and (self.clear == 0).all()
        assert bit_equal(self.d_cur.cpu(), self.cur) and bit_equal(self.d_numel.cpu(), self.numel)


@pytest.mark.parametrize("loss_dtype", [torch.float32, torch.float64])
def test_step_finalize_cost_ratios_reset_and_advance(native_lib, loss_dtype):
    f = Fin(loss_dtype, seed=1)
    ctr = torch.tensor([40], dtype=torch.int32, device=DEV)
    f.run(epoch=7, ratio_row=1, ctr=ctr)
    f.check(cost_at=7, row=1)
    assert ctr.item() == 8  # the host epoch wins and the counter follows it


def test_step_finalize_without_ratios_or_counter(native_lib):
    f = Fin(torch.float32, seed=2)
    f.run(epoch=0, ratio_row=-1)
    f.check(cost_at=0, row=None)


@pytest.mark.parametrize("epoch,row", [(6, 2), (7, None)])
@pytest.mark.parametrize("device_epoch", [False, True])
def test_step_finalize_ratio_rule(native_lib, epoch, row, device_epoch):
    """ratio_row = -2: every third epoch writes row epoch / 3; epoch = -1 reads the device counter."""
    f = Fin(torch.float32, seed=3)
    ctr = torch.tensor([epoch if device_epoch else 0], dtype=torch.int32, device=DEV)
    f.run(epoch=-1 if device_epoch else epoch, ratio_row=-2, ctr=ctr, every=3)
    f.check(cost_at=epoch, row=row)
    assert ctr.item() == epoch + 1


def test_step_finalize_guards_the_ends_of_costs_and_ratios(native_lib):
    """A device epoch equal to len(costs) writes no cost, a rule row equal to the number of rows
    no ratios; costs and ratios are leading views, so even a broken guard stays in owned memory."""
    f = Fin(torch.float32, n_costs=9, n_rows=3, seed=4)
    ctr = torch.tensor([9], dtype=torch.int32, device=DEV)
    f.run(epoch=-1, ratio_row=-2, ctr=ctr, every=3)  # row 9 / 3 = 3 = the number of rows
    f.check(cost_at=None, row=None)
    assert ctr.item() == 10
    f = Fin(torch.float32, n_costs=9, n_rows=3, seed=4)  # the last valid cost and row are written
    ctr = torch.tensor([6], dtype=torch.int32, device=DEV)
    f.run(epoch=-1, ratio_row=-2, ctr=ctr, every=3)
    f.check(cost_at=6, row=2)
