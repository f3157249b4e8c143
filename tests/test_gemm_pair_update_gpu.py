"""pz::gemm_pair (two weight-gradient GEMMs in one launch) and pz::gemm_update (EPI_OPT: the optimizer
update inside the dW epilogue, epilogue_opt in csrc/gemm_mfma.hip), element by element.

gemm_pair. Integer operands in [-4, 4] (tests.helpers.exact_operands / exact_operands_fp8): every
accumulation order gives the same z, so both outputs must EQUAL bf16_rne(z) / fp32(z) / bf16_rne(z
scale_a scale_b) (fp8: per-problem power-of-two scales, problem 1's with a None). Split factors 1, 2,
4, 8 (and 1 with 240 + 1 tiles) are asserted through gemm_pair_split first; outputs start as NaN, every
case launches three times (ticket reuse) and runs in both orders of the two problems (the nwg0
boundary moves). Kernel names: pair/var30/256x256/ek1 (bf16), ek0 (fp32 out), pair/var14/256x256/ek1
(fp8), /split1|2|4|8; engine = 2: sk/var0/256x256/ek1/split1 on 37 and 200 CUs.

gemm_update. torch.ops.pz.gemm_update with integer bf16 operands: the gradient is z exactly.
  SGD with tests.helpers.SGD_EXACT (powers of two): p EQUALS the fp64 formula, the bf16 shadow is
  bf16(p), the fp32 shadow p, m and v keep their bits.
  Adam against opt_update_reference in fp64 with test_optimizer_gpu.check_update's bound, 4 max|fp32
  formula - fp64 formula| + 2^-23 |ref|; at b1 = b2 = 0.5 with power-of-two grad_scale and l2 the
  moment m = m0 + 0.5 (g - m0) rounds once however it is contracted: it EQUALS the fp32 formula.
  Statistics: the four doubles against fp64 sums over the resulting p (d = p - p0 subtracted in fp32,
  as the kernel does) within (M N + 1) 2^-53 (sum |term| + |previous value|), which bounds any summation
  order; amax exact; a second launch into the non-zero sums and an amax preloaded above / below;
  stats_every = 2 at an even and an odd epoch; stats = amax = None; the hp table's row `epoch`.
  Strided state: params, m, v and shadow as column slices [:, 8 : 8 + N] of buffers 16 columns wider and
  8 rows taller, every byte outside the slices unchanged.
Kernel names (gemm_choose, fp32 C): (256, 256, 64), (200, 136, 96) and (512, 4096, 512)
mfma/var6/128x128/ek0/split1; (4088, 3832, 64) mfma/var30/256x256/ek0/split1; (1536, 1280, 4096) and the
ragged-M (1528, 1280, 4096) mfma/var30/256x256/ek0/split8.

Measured on MI355X (the file takes about 5 s): every split factor and kernel name above as predicted,
no shape had to change; every gemm_pair output, every SGD update and the b1 = 0.5 first moment exact.
Worst err / bound: Adam p 0.168, m 0.228, v 0.253 (the kernel errs like the fp32 formula: the bound
allows four times that); the statistics 5.8e-5 of their bound (most sums come out exact).
"""
import functools
import math

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import (PAIR_SPLIT_CASES, SGD_EXACT, UPDATE_SPLIT_CASES, assert_gemm_exact, bit_equal, exact_operands,
                           exact_operands_fp8, opt_update_reference)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


# ================================================================================== gemm_pair
PAIR_KERNEL = {"bf16": "pair/var30/256x256/ek1", "f32": "pair/var30/256x256/ek0", "fp8": "pair/var14/256x256/ek1"}
# fp8: (scale_a, scale_b) of the first and of the second problem of a launch (None = 1)
PAIR_SCALES = ((0.25, 2.0 ** -6), (2.0 ** -3, None))


@functools.lru_cache(maxsize=None)
def pair_problem(M, N, K, fp8, seed):
    """dW-layout operands a [K, M], b [K, N] on the device and the fp64 z = a^T b."""
    if fp8:
        a, b, z = exact_operands_fp8(M, N, K, False, False, E4M3, E5M2, seed)
    else:
        a, b, z = exact_operands(M, N, K, False, False, seed)
    return a.to(DEV), b.to(DEV), z.to(DEV)


def scalar(v):
    return None if v is None else torch.tensor([v], device=DEV)


def run_pair(s0, s1, K, kind, split, *, engine=0, cus=0, name=None):
    fp8 = kind == "fp8"
    out = F32 if kind == "f32" else BF16
    a0, b0, z0 = pair_problem(*s0, K, fp8, 1)
    a1, b1, z1 = pair_problem(*s1, K, fp8, 2)
    c0 = torch.empty(s0, device=DEV, dtype=out)
    c1 = torch.empty(s1, device=DEV, dtype=out)
    assert PF.gemm_pair_split(a0, b0, c0, a1, b1, c1, engine=engine) == split
    kw = {}
    f0 = f1 = 1.0
    if fp8:
        (sa0, sb0), (sa1, sb1) = PAIR_SCALES
        kw = dict(scales0=(scalar(sa0), scalar(sb0)), scales1=(scalar(sa1), scalar(sb1)))
        f0, f1 = sa0 * sb0, sa1 * (sb1 or 1.0)
    for _ in range(3):
        c0.fill_(float("nan"))
        c1.fill_(float("nan"))
        PF.gemm_pair(a0, b0, c0, a1, b1, c1, engine=engine, cus=cus, **kw)
        assert PF.gemm_last_kernel() == (name or f"{PAIR_KERNEL[kind]}/split{split}")
        assert_gemm_exact(c0, z0 * f0)
        assert_gemm_exact(c1, z1 * f1)


@pytest.mark.parametrize("kind", ["bf16", "f32", "fp8"])
@pytest.mark.parametrize("s0,s1,K,split", PAIR_SPLIT_CASES, ids=[f"K{c[2]}-split{c[3]}-{c[0][0]}" for c in PAIR_SPLIT_CASES])
@pytest.mark.parametrize("swap", [False, True], ids=["order01", "order10"])
def test_gemm_pair_is_exact(native_lib, s0, s1, K, split, kind, swap):
    if swap:
        s0, s1 = s1, s0
    run_pair(s0, s1, K, kind, split)


@pytest.mark.parametrize("cus", [37, 200])
def test_gemm_pair_on_the_stream_k_engine_is_exact(native_lib, cus):
    """engine = 2: both problems' 120 tiles as one persistent schedule, on fewer workgroups than tiles
    (37) and on more (200: tiles cut along K and folded)."""
    (s0, s1, K, split) = PAIR_SPLIT_CASES[1]
    run_pair(s0, s1, K, "bf16", split, engine=2, cus=cus, name="sk/var0/256x256/ek1/split1")


def test_gemm_pair_refuses_unequal_or_unsupported_fp8_formats(native_lib):
    K, n = 64, 256
    g = torch.Generator(device="cpu").manual_seed(5)
    src = torch.randint(-4, 5, (K, n), generator=g).float().to(DEV)
    c0, c1 = (torch.empty(n, n, device=DEV, dtype=BF16) for _ in range(2))
    x4, x5 = src.to(E4M3), src.to(E5M2)
    assert PF.gemm_pair_split(x4, x5, c0, x4, x5, c1) == 1               # the supported pair: e4m3^T x e5m2
    for a1, b1 in ((x4, x4), (x5, x5), (x5, x4)):
        assert PF.gemm_pair_split(x4, x5, c0, a1, b1, c1) == 0
        assert PF.gemm_pair_split(a1, b1, c1, x4, x5, c0) == 0
    with pytest.raises(RuntimeError, match="cannot share a launch"):
        PF.gemm_pair(x4, x5, c0, x4, x4, c1)
    assert PF.gemm_pair_split(x4, x5, c0, x4, x5, torch.empty(n, n, device=DEV)) == 0   # fp8 pairs store bf16


# ================================================================================== gemm_update
UPDATE_KERNEL = {(256, 256, 64): "mfma/var6/128x128/ek0", (200, 136, 96): "mfma/var6/128x128/ek0",
                 (512, 4096, 512): "mfma/var6/128x128/ek0", (4088, 3832, 64): "mfma/var30/256x256/ek0",
                 (1536, 1280, 4096): "mfma/var30/256x256/ek0", (1528, 1280, 4096): "mfma/var30/256x256/ek0"}
UPDATE_SPLIT = dict(UPDATE_SPLIT_CASES)
U_TILE, U_128, U_256, U_PASS, U_SPLIT, U_SPLITR = [s for s, _ in UPDATE_SPLIT_CASES]
# test_optimizer_gpu's hyper-parameters (every term matters), and a set whose first moment is exact
HP = dict(lr=0.01, b1=0.9, b2=0.99, eps=1e-3, bc1=1 - 0.9 ** 3, bc2s=math.sqrt(1 - 0.99 ** 3), grad_scale=0.5, l2=1e-3)
HP_HALF = dict(HP, b1=0.5, b2=0.5, bc1=1 - 0.5 ** 3, bc2s=math.sqrt(1 - 0.5 ** 3), l2=2.0 ** -4)
HP_SGD = dict(HP, **SGD_EXACT)
PAD = 8


@functools.lru_cache(maxsize=None)
def update_problem(M, N, K):
    """x [K, M], dZ [K, N] (integers, bf16), the exact gradient z, and the state: p0 in multiples of
    1/8, m0 and v0 as in test_optimizer_gpu (fp32)."""
    a, b, z = exact_operands(M, N, K, False, False, seed=M + 3 * N + 7 * K)
    g = torch.Generator(device="cpu").manual_seed(M * 5 + N + K)
    p0 = torch.randint(-32, 33, (M, N), generator=g).float() / 8
    m0 = (0.01 * torch.randn(M, N, generator=g, dtype=F64)).float()
    v0 = (1e-4 + 1e-3 * torch.rand(M, N, generator=g, dtype=F64)).float()
    return tuple(t.to(DEV) for t in (a, b, z, p0, m0, v0))


class State:
    """params / m / v / shadow of one launch: contiguous, or column slices of wider buffers."""

    def __init__(self, shape, shadow, strided):
        M, N, K = shape
        self.shape, self.strided = shape, strided
        _, _, _, p0, m0, v0 = update_problem(*shape)
        g = torch.Generator(device="cpu").manual_seed(77)
        self.base, self.view = {}, {}
        for k, src, dt in (("p", p0, F32), ("m", m0, F32), ("v", v0, F32), ("shadow", None, shadow)):
            if dt is None:
                self.view[k] = None
                continue
            if strided:
                base = torch.randn(M + 8, N + 2 * PAD, generator=g).to(DEV, dt)
                view = base[:M, PAD:PAD + N]
            else:
                base = view = torch.full((M, N), 7.0, device=DEV, dtype=dt)
            if src is not None:
                view.copy_(src)
            self.base[k], self.view[k] = base, view
        self.before = {k: b.clone() for k, b in self.base.items()}

    def assert_frames_untouched(self):
        M, N, _ = self.shape
        for k, base in self.base.items():
            if self.strided:
                now, was = base.clone(), self.before[k].clone()
                now[:M, PAD:PAD + N] = 0
                was[:M, PAD:PAD + N] = 0
                assert bit_equal(now, was), k


def launch_update(shape, st, *, adam, hp, stats=None, amax=None, table=None, epoch=None, stats_every=1):
    M, N, K = shape
    a, b = update_problem(*shape)[:2]
    v = st.view
    torch.ops.pz.gemm_update(a, False, b, False, v["p"], M, N, K, 1.0, v["p"], v["m"], v["v"], v["shadow"], stats, amax,
                             adam, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["bc1"], hp["bc2s"], hp["grad_scale"],
                             hp["l2"], table, epoch, stats_every)
    assert PF.gemm_last_kernel() == f"{UPDATE_KERNEL[shape]}/split{UPDATE_SPLIT[shape]}"
    torch.cuda.synchronize()


def check_state(shape, st, *, adam, hp, label=""):
    """p / m / v / shadow of ``st`` after ONE update from the problem's initial state."""
    M, N, K = shape
    _, _, z, p0, m0, v0 = update_problem(*shape)
    v = st.view
    w = torch.ones(M, N, dtype=torch.bool, device=DEV)
    ref = opt_update_reference(p0.double(), z, m0.double(), v0.double(), w, F64, adam=adam, **hp)
    if not adam:
        assert torch.equal(ref[0].float().double(), ref[0]), "the reference is not exact in fp32"
        assert torch.equal(v["p"].double(), ref[0]), (label, (v["p"].double() - ref[0]).abs().max().item())
        assert bit_equal(v["m"], m0) and bit_equal(v["v"], v0)   # SGD has no moments
    else:
        f32 = opt_update_reference(p0, z.float(), m0, v0, w, F32, adam=True, **hp)
        for name, r, x, f in zip("pmv", ref, (v["p"], v["m"], v["v"]), f32):
            e = (f.double() - r).abs().max().item()
            err = (x.double() - r).abs()
            bound = 4 * e + 2.0 ** -23 * r.abs()
            print(f"gemm_update {shape} {label} {name}: max|kernel - fp64| = {err.max().item():.3e}, max|fp32 formula - "
                  f"fp64| = {e:.3e}, worst err/bound {(err / bound).max().item():.3f}")
            assert (err <= bound).all(), (name, err.max().item(), e)
        if hp["b1"] == 0.5:   # one rounding of g - m0, one of the sum: no contraction changes it
            assert torch.equal(v["m"], f32[1]), (label, "m")
    if v["shadow"] is not None:
        assert torch.equal(v["shadow"], v["p"].to(v["shadow"].dtype))
    st.assert_frames_untouched()


def stats_terms(p1, p0):
    """The terms of the four sums (fp64, [4, M, N]): d, d^2, w, w^2 with d = p1 - p0 subtracted in fp32."""
    d, w = (p1 - p0).double(), p1.double()
    return torch.stack([d, d * d, w, w * w])


def assert_stats(got, before, terms, which=(0, 1, 2, 3)):
    """``got`` = ``before`` + the sums of ``terms`` for the slots in ``which``, the others bit-unchanged."""
    n = terms[0].numel()
    for k in range(4):
        if k not in which:
            assert bit_equal(got[k:k + 1], before[k:k + 1]), k
            continue
        want = before[k].item() + terms[k].sum().item()
        bound = (n + 1) * 2.0 ** -53 * (terms[k].abs().sum().item() + abs(before[k].item()))
        err = abs(got[k].item() - want)
        print(f"stats[{k}]: err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)


SGD_CASES = [(U_TILE, BF16, False), (U_128, F32, True), (U_128, None, False), (U_256, BF16, False), (U_PASS, F32, False),
             (U_SPLIT, BF16, True), (U_SPLITR, None, False), (U_SPLITR, F32, True)]


def _id(v):
    """Readable ids: a shape, a shadow dtype, strided or not; anything else keeps pytest's default."""
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    if isinstance(v, bool):
        return "strided" if v else "flat"
    return {BF16: "shadow_bf16", F32: "shadow_f32", None: "no_shadow"}.get(v) if v is None or isinstance(v, torch.dtype) else None


@pytest.mark.parametrize("shape,shadow,strided", SGD_CASES, ids=_id)
def test_gemm_update_sgd_is_exact(native_lib, shape, shadow, strided):
    st = State(shape, shadow, strided)
    launch_update(shape, st, adam=False, hp=HP_SGD)
    check_state(shape, st, adam=False, hp=HP_SGD, label="sgd")


@pytest.mark.parametrize("hp", [HP, HP_HALF], ids=["b0.9_0.99", "b0.5_0.5"])
@pytest.mark.parametrize("shape,shadow,strided", [(U_TILE, BF16, False), (U_128, BF16, True), (U_256, F32, False),
                                                  (U_PASS, None, False), (U_SPLIT, F32, True), (U_SPLITR, BF16, True)], ids=_id)
def test_gemm_update_adam_matches_fp64(native_lib, shape, shadow, strided, hp):
    st = State(shape, shadow, strided)
    launch_update(shape, st, adam=True, hp=hp)
    check_state(shape, st, adam=True, hp=hp, label="adam")


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("shape,strided", [(U_TILE, False), (U_128, True), (U_256, False), (U_SPLITR, True)], ids=_id)
def test_gemm_update_statistics_accumulate(native_lib, shape, strided, adam):
    """Two launches into one stats record: from zero, then into the non-zero sums, with amax first
    zero, then preloaded above the maximum (it stays) and below it (it is raised)."""
    hp = HP if adam else HP_SGD
    p0 = update_problem(*shape)[3]
    st = State(shape, BF16, strided)
    big = torch.zeros(12, device=DEV, dtype=F64)
    big[:4], big[8:] = 3.25, -1.5
    stats, amax = big[4:8], torch.zeros(1, device=DEV)
    launch_update(shape, st, adam=adam, hp=hp, stats=stats, amax=amax)
    check_state(shape, st, adam=adam, hp=hp, label="stats")
    p1 = st.view["p"].clone()
    first = stats.clone()
    assert_stats(first, torch.zeros(4, device=DEV, dtype=F64), stats_terms(p1, p0))
    assert amax.item() == p1.abs().max().item()
    for preload in (1e6, 2.0 ** -10):
        amax.fill_(preload)
        before, p_in = stats.clone(), st.view["p"].clone()
        launch_update(shape, st, adam=adam, hp=hp, stats=stats, amax=amax)
        p2 = st.view["p"]
        assert_stats(stats, before, stats_terms(p2, p_in))
        assert amax.item() == max(preload, p2.abs().max().item())
    assert (big[:4] == 3.25).all() and (big[8:] == -1.5).all()
    st.assert_frames_untouched()


@pytest.mark.parametrize("epoch,which", [(4, (0, 1, 2, 3)), (5, (3,))])
@pytest.mark.parametrize("shape,strided", [(U_128, False), (U_SPLITR, True)], ids=_id)
def test_gemm_update_stats_every_second_epoch(native_lib, shape, strided, epoch, which):
    """stats_every = 2: an even epoch writes all four sums, an odd one only sum w^2."""
    p0 = update_problem(*shape)[3]
    st = State(shape, F32, strided)
    stats = torch.tensor([1.0, 2.0, 3.0, 4.0], device=DEV, dtype=F64)
    before, amax = stats.clone(), torch.zeros(1, device=DEV)
    ctr = torch.tensor([epoch], dtype=torch.int32, device=DEV)
    launch_update(shape, st, adam=True, hp=HP, stats=stats, amax=amax, epoch=ctr, stats_every=2)
    check_state(shape, st, adam=True, hp=HP, label=f"epoch {epoch}")
    assert_stats(stats, before, stats_terms(st.view["p"], p0), which)
    assert amax.item() == st.view["p"].abs().max().item() and ctr.item() == epoch


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("shape", [U_128, U_SPLIT], ids=_id)
def test_gemm_update_without_statistics_changes_nothing_else(native_lib, shape, adam):
    hp = HP if adam else HP_SGD
    outs = []
    for with_stats in (True, False):
        st = State(shape, BF16, True)
        stats = torch.zeros(4, device=DEV, dtype=F64) if with_stats else None
        amax = torch.zeros(1, device=DEV) if with_stats else None
        launch_update(shape, st, adam=adam, hp=hp, stats=stats, amax=amax)
        check_state(shape, st, adam=adam, hp=hp, label="with stats" if with_stats else "stats=None")
        outs.append(st)
    for k in ("p", "m", "v", "shadow"):
        assert bit_equal(outs[0].base[k], outs[1].base[k]), k


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("epoch", [1, 3])
@pytest.mark.parametrize("shape,strided", [(U_128, True), (U_SPLIT, False)], ids=_id)
def test_gemm_update_hp_table_row_of_the_epoch_wins(native_lib, shape, strided, epoch, adam):
    """An hp table (rows of lr, bc1, bc2s, 0 in fp64) and the device epoch counter, built as
    test_optimizer_gpu builds them: row `epoch` replaces the scalar lr / bc1 / bc2s arguments."""
    base = HP if adam else HP_SGD
    rows = [[base["lr"] * 2.0 ** -r, 1 - 0.9 ** (r + 1), math.sqrt(1 - 0.99 ** (r + 1)), 0.0] for r in range(6)]
    table = torch.tensor(rows, dtype=F64, device=DEV)
    ctr = torch.tensor([epoch], dtype=torch.int32, device=DEV)
    st = State(shape, BF16, strided)
    launch_update(shape, st, adam=adam, hp=dict(base, lr=1.0, bc1=0.5, bc2s=0.5), table=table, epoch=ctr)
    check_state(shape, st, adam=adam, hp=dict(base, lr=rows[epoch][0], bc1=rows[epoch][1], bc2s=rows[epoch][2]),
                label=f"hp row {epoch}")
    assert ctr.item() == epoch and torch.equal(table.cpu(), torch.tensor(rows, dtype=F64))
