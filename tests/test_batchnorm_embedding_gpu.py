"""pz::batchnorm_fwd / batchnorm_bwd and pz::embedding_fwd / embedding_bwd, raw ops, against fp64 torch.

The batchnorm kernels compute in fp64 and round once to the activation dtype T, so the references
are fp64 torch on the stored T values and the bounds are one ulp of T (plus 1e-9); outputs in the
parameter dtype (running statistics, dgain, dbias) get 4 ulp of it.
"""
import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import bit_equal, keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"

EPS, MOM = 1e-5, 0.1
ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8}
# activation dtype T, parameter dtype P
DTYPES = [(torch.float64, torch.float64), (torch.float32, torch.float32), (torch.bfloat16, torch.float32)]
DTYPE_IDS = ["f64", "f32", "bf16"]


def close_t(got, ref, what):
    """An output in the activation dtype against its fp64 reference."""
    err = (got.double().cpu() - ref).abs()
    bound = 1e-9 + (1e-9 if got.dtype == torch.float64 else ULP[got.dtype]) * ref.abs()
    assert (err <= bound).all(), (what, err.max().item())


def close_p(got, ref, what):
    """An output in the parameter dtype (or an fp64 workspace) against its fp64 reference."""
    err = (got.double().cpu() - ref).abs()
    bound = 1e-9 + (1e-9 if got.dtype == torch.float64 else 4 * ULP[got.dtype]) * ref.abs()
    assert (err <= bound).all(), (what, err.max().item())


class Bn:
    """Inputs of one batchnorm case (CPU fp64 views of the stored values) and the op workspaces."""

    def __init__(self, rows, cols, T, P, seed, rows_valid=None):
        g = torch.Generator(device="cpu").manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
        u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
        # column means near 3, standard deviations near 0.5: the mean and sum(x^2) - n mean^2 matter
        x = (3.0 + 0.3 * r(cols)) + (0.4 + 0.2 * u(cols)) * r(rows, cols)
        self.rows, self.cols, self.T, self.P = rows, cols, T, P
        self.n = rows if rows_valid is None else rows_valid
        self.x, self.g = x.to(T).to(DEV), r(rows, cols).to(T).to(DEV)
        self.gain, self.bias = (0.5 + u(cols)).to(P).to(DEV), r(cols).to(P).to(DEV)
        self.rm, self.rv = (2.0 + 0.5 * r(cols)).to(P).to(DEV), (0.5 + u(cols)).to(P).to(DEV)
        self.rm0, self.rv0 = self.rm.clone(), self.rv.clone()
        self.dgain0, self.dbias0 = r(cols).to(P), r(cols).to(P)
        self.y = torch.full((rows, cols), 7.0, dtype=T, device=DEV)
        self.dx = torch.full((rows, cols), 7.0, dtype=T, device=DEV)
        self.save_mean, self.save_inv = (torch.full((cols,), 7.0, dtype=torch.float64, device=DEV) for _ in range(2))
        self.partial = torch.full((2 * cols,), 7.0, dtype=torch.float64, device=DEV)
        self.x64, self.g64 = self.x.double().cpu(), self.g.double().cpu()
        self.gain64, self.bias64 = self.gain.double().cpu(), self.bias.double().cpu()

    def fwd(self, training=True, epi=PF.NO_EPI, idx_ld=0, phase=0, n_total=0):
        torch.ops.pz.batchnorm_fwd(self.x, self.y, self.gain, self.bias, self.rm, self.rv, EPS, MOM, training, self.n,
                                   self.save_mean, self.save_inv, self.partial, epi[0], epi[1], idx_ld, phase, n_total)
        torch.cuda.synchronize()

    def bwd(self, dgain, dbias, dx=True, epi=PF.NO_EPI, idx_ld=0, phase=0, n_total=0):
        torch.ops.pz.batchnorm_bwd(self.g, self.y, self.x, self.dx if dx else None, self.gain, self.bias,
                                   self.save_mean, self.save_inv, dgain, dbias, self.partial, self.n, epi[0], epi[1],
                                   idx_ld, phase, n_total)
        torch.cuda.synchronize()

    # ---- fp64 reference (valid rows only)
    def stats(self):
        xv = self.x64[:self.n]
        return xv.mean(0), xv.var(0, unbiased=True)

    def normalise(self, x, mean, var):
        return self.gain64 * (x - mean) / torch.sqrt(var + EPS) + self.bias64

    def grads(self, dyn):
        """torch.autograd through the training-mode formula for the upstream gradient `dyn`."""
        x = self.x64[:self.n].clone().requires_grad_()
        gain = self.gain64.clone().requires_grad_()
        bias = self.bias64.clone().requires_grad_()
        z = gain * (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=True) + EPS) + bias
        return torch.autograd.grad(z, (x, gain, bias), dyn[:self.n])

    def check_padding(self, *outs):
        for t in outs:
            assert (t[self.n:] == 0).all()  # exactly zero over the 7.0 pre-fill


@pytest.mark.parametrize("T,P", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("rows,cols,pad", [
    (600, 70, 0),     # two column strips (64 + 6), three row chunks, the last with 88 rows
    (600, 70, 85),    # padded rows: 515 valid, the last chunk has 3
    (300, 300, 0),    # five strips; the finalize / parameter-gradient kernels' second block
    (300, 300, 85),
    (5, 3, 0),
])
def test_batchnorm_training_forward_backward(native_lib, rows, cols, pad, T, P):
    b = Bn(rows, cols, T, P, seed=rows + cols + pad, rows_valid=rows - pad)
    n = b.n
    b.fwd()
    mean, var = b.stats()
    close_p(b.partial, torch.cat([b.x64[:n].sum(0), (b.x64[:n] ** 2).sum(0)]), "partial")
    close_p(b.save_mean, mean, "save_mean")
    close_p(b.save_inv, 1.0 / torch.sqrt(var + EPS), "save_invstd")
    close_p(b.rm, (1 - MOM) * b.rm0.double().cpu() + MOM * mean, "running_mean")
    close_p(b.rv, (1 - MOM) * b.rv0.double().cpu() + MOM * var, "running_var")
    close_t(b.y[:n], b.normalise(b.x64[:n], mean, var), "y")
    b.check_padding(b.y)

    dx, dgain, dbias = b.grads(b.g64)
    dg, db = b.dgain0.clone().to(DEV), b.dbias0.clone().to(DEV)  # non-zero: the kernel accumulates
    b.bwd(dg, db)
    close_t(b.dx[:n], dx, "dx")
    b.check_padding(b.dx)
    close_p(dg, b.dgain0.double() + dgain, "dgain")
    close_p(db, b.dbias0.double() + dbias, "dbias")
    # parameter gradients only
    dg, db = b.dgain0.clone().to(DEV), b.dbias0.clone().to(DEV)
    before = b.dx.clone()
    b.bwd(dg, db, dx=False)
    close_p(dg, b.dgain0.double() + dgain, "dgain (dx = None)")
    close_p(db, b.dbias0.double() + dbias, "dbias (dx = None)")
    assert bit_equal(b.dx, before)
    # one of the two alone
    dg = b.dgain0.clone().to(DEV)
    b.bwd(dg, None, dx=False)
    close_p(dg, b.dgain0.double() + dgain, "dgain alone")


@pytest.mark.parametrize("T,P", DTYPES, ids=DTYPE_IDS)
def test_batchnorm_eval_forward_uses_running_statistics(native_lib, T, P):
    b = Bn(600, 70, T, P, seed=11)
    b.fwd(training=False)
    assert bit_equal(b.rm, b.rm0) and bit_equal(b.rv, b.rv0)
    rm, rv = b.rm0.double().cpu(), b.rv0.double().cpu()
    close_t(b.y, b.normalise(b.x64, rm, rv), "y")
    close_p(b.save_mean, rm, "save_mean")
    close_p(b.save_inv, 1.0 / torch.sqrt(rv + EPS), "save_invstd")
    assert (b.partial == 7.0).all()  # no statistics pass in eval mode


@pytest.mark.parametrize("T,P", DTYPES, ids=DTYPE_IDS)
def test_batchnorm_eval_autograd(native_lib, T, P):
    """PF.batchnorm(training=False): y from the running statistics, which stay as they are, and the
    gradients of y = gain (x - rm) / sqrt(rv + eps) + bias.

    The eval backward is plain torch in the activation dtype T, not a kernel, so for fp32 / bf16 its
    bounds count that path's roundings (u = the unit roundoff of T, inv = 1 / sqrt(rv + eps)):
    dx = g * (gain_T * inv_T): four roundings, 4u |ref|;
    dbias = sum(g): n fp32-or-better additions, n 2^-24 sum|g|, and one rounding to T;
    dgain = sum(g * ((x - rm_T) * inv_T)): per term u |g| inv (|rm| + |x - rm|) for the rounded
    mean and the subtraction plus 3u |term|, then the additions and one rounding as for dbias.
    Second-order terms: a factor 1 + 16u."""
    b = Bn(600, 70, T, P, seed=12)
    x, gain, bias = (t.clone().requires_grad_() for t in (b.x, b.gain, b.bias))
    y, rm, rv = PF.batchnorm(x, gain, bias, b.rm, b.rv, EPS, MOM, False)
    assert bit_equal(rm, b.rm0) and bit_equal(rv, b.rv0) and bit_equal(b.rm, b.rm0) and bit_equal(b.rv, b.rv0)
    got = torch.autograd.grad(y, (x, gain, bias), b.g)
    assert [t.dtype for t in got] == [T, P, P]
    rm64, rv64 = b.rm0.double().cpu(), b.rv0.double().cpu()
    xr, gr, br = (t.clone().requires_grad_() for t in (b.x64, b.gain64, b.bias64))
    yr = gr * (xr - rm64) / torch.sqrt(rv64 + EPS) + br
    ref = torch.autograd.grad(yr, (xr, gr, br), b.g64)
    close_t(y.detach(), yr.detach(), "y")
    if T == torch.float64:
        close_t(got[0], ref[0], "dx")
        close_p(got[1], ref[1], "dgain")
        close_p(got[2], ref[2], "dbias")
        return
    u = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}[T]  # unit roundoff: 24 / 8 significand bits
    n, so = b.rows, 1 + 16 * u
    inv, g = 1.0 / torch.sqrt(rv64 + EPS), b.g64.abs()
    err = [(a.double().cpu() - r).abs() for a, r in zip(got, ref)]
    assert (err[0] <= so * 4 * u * ref[0].abs() + 1e-9).all(), ("dx", err[0].max().item())
    term = g * (b.x64 - rm64).abs() * inv
    per_term = (g * inv * u * (rm64.abs() + (b.x64 - rm64).abs()) + 3 * u * term).sum(0)
    bound = so * (per_term + n * 2.0 ** -24 * term.sum(0) + u * ref[1].abs()) + 1e-9
    assert (err[1] <= bound).all(), ("dgain", (err[1] / bound).max().item())
    bound = so * (n * 2.0 ** -24 * g.sum(0) + u * ref[2].abs()) + 1e-9
    assert (err[2] <= bound).all(), ("dbias", (err[2] / bound).max().item())


def _masks(b, idx_ld, p, seed):
    ld = idx_ld if idx_ld > 0 else b.cols
    pre = keep_mask(b.rows * ld, seed[0], seed[1], 3, p).reshape(b.rows, ld)[:, :b.cols]
    post = keep_mask(b.rows * ld, seed[0], seed[1], 4, p).reshape(b.rows, ld)[:, :b.cols]
    return torch.from_numpy(pre.copy()).double(), torch.from_numpy(post.copy()).double()


ACT = {PF.ACT_NONE: (lambda z: z, lambda a: torch.ones_like(a)),
       PF.ACT_RELU: (torch.relu, lambda a: (a > 0).double()),
       PF.ACT_TANH: (torch.tanh, lambda a: 1 - a * a),
       PF.ACT_SIGMOID: (torch.sigmoid, lambda a: a * (1 - a))}


@pytest.mark.parametrize("T,P", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("ld_extra", [0, 6], ids=["ld_cols", "ld_cols+6"])
@pytest.mark.parametrize("act", [PF.ACT_NONE, PF.ACT_RELU, PF.ACT_TANH, PF.ACT_SIGMOID],
                         ids=["none", "relu", "tanh", "sigmoid"])
def test_batchnorm_fused_epilogue(native_lib, act, ld_extra, T, P):
    """y = drop_post(act(drop_pre(bn(x)))) with the masks indexed r * idx_ld + c, and its backward,
    whose activation derivative comes from the stored y (checked separately), as in the kernel."""
    p, seed = 0.25, (1234 + act, 99)
    b = Bn(600, 70, T, P, seed=20 + act)
    idx_ld = b.cols + ld_extra if ld_extra else 0
    epi = PF.epi_spec(act, drop_pre=3, drop_post=4, p=p, seed=seed)
    pre, post = _masks(b, idx_ld, p, seed)
    sc = 1.0 / (1.0 - p)
    fwd, dact = ACT[act]
    b.fwd(epi=epi, idx_ld=idx_ld)
    mean, var = b.stats()
    close_t(b.y, fwd(b.normalise(b.x64, mean, var) * pre * sc) * post * sc, "y")
    assert 0.7 < pre.mean() < 0.8 and 0.7 < post.mean() < 0.8 and not torch.equal(pre, post)

    y = b.y.double().cpu()
    dyn = b.g64 * post * sc * dact(y * (1.0 - p)) * pre * sc
    dx, dgain, dbias = b.grads(dyn)
    dg, db = b.dgain0.clone().to(DEV), b.dbias0.clone().to(DEV)
    b.bwd(dg, db, epi=epi, idx_ld=idx_ld)
    close_t(b.dx, dx, "dx")
    close_p(dg, b.dgain0.double() + dgain, "dgain")
    close_p(db, b.dbias0.double() + dbias, "dbias")


@pytest.mark.parametrize("T,P", DTYPES, ids=DTYPE_IDS)
def test_batchnorm_two_phase_matches_one_launch(native_lib, T, P):
    """Synchronised form: phase 1 per half (local sums), the sums added, phase 2 per half with
    n_total = 600 — against the one-launch result over the whole batch and the fp64 reference."""
    w = Bn(600, 70, T, P, seed=30)
    w.fwd()
    zeros = lambda: torch.zeros(w.cols, dtype=P, device=DEV)  # noqa: E731
    wdg, wdb = zeros(), zeros()
    w.bwd(wdg, wdb)
    halves = []
    for h in range(2):
        b = Bn(300, 70, T, P, seed=30)
        b.x, b.g = w.x[300 * h:300 * h + 300].contiguous(), w.g[300 * h:300 * h + 300].contiguous()
        b.gain, b.bias, b.rm, b.rv = w.gain, w.bias, w.rm0.clone(), w.rv0.clone()
        b.fwd(phase=1)
        halves.append(b)
    assert all((b.y == 7.0).all() for b in halves)  # phase 1 only sums
    x64 = w.x64
    for h, b in enumerate(halves):
        xh = x64[300 * h:300 * h + 300]
        close_p(b.partial, torch.cat([xh.sum(0), (xh ** 2).sum(0)]), "local partial")
    total = halves[0].partial + halves[1].partial
    mean, var = w.stats()
    yr = w.normalise(x64, mean, var)
    for h, b in enumerate(halves):
        b.partial = total.clone()
        b.fwd(phase=2, n_total=600)
        close_t(b.y, yr[300 * h:300 * h + 300], "y")
        close_t(b.y, w.y[300 * h:300 * h + 300].double().cpu(), "y vs one launch")
        close_p(b.rm, (1 - MOM) * w.rm0.double().cpu() + MOM * mean, "running_mean")
        close_p(b.rv, (1 - MOM) * w.rv0.double().cpu() + MOM * var, "running_var")
        close_p(b.rm, w.rm.double().cpu(), "running_mean vs one launch")
        close_p(b.rv, w.rv.double().cpu(), "running_var vs one launch")
        close_p(b.save_mean, mean, "save_mean")
    # backward: local parameter gradients in phase 1, dx from the global sums in phase 2
    local = []
    for b in halves:
        dg, db = zeros(), zeros()
        b.bwd(dg, db, phase=1)
        assert (b.dx == 7.0).all()
        local.append((dg, db))
    total = halves[0].partial + halves[1].partial
    dx, dgain, dbias = w.grads(w.g64)
    for h, b in enumerate(halves):
        b.partial = total.clone()
        dg, db = local[h][0].clone(), local[h][1].clone()
        b.bwd(dg, db, phase=2, n_total=600)
        assert bit_equal(dg, local[h][0]) and bit_equal(db, local[h][1])  # phase 2 leaves them alone
        close_t(b.dx, dx[300 * h:300 * h + 300], "dx")
        close_t(b.dx, w.dx[300 * h:300 * h + 300].double().cpu(), "dx vs one launch")
    for k, ref, what in ((0, dgain, "dgain halves"), (1, dbias, "dbias halves")):  # each half rounded to P
        a, c = local[0][k].double().cpu(), local[1][k].double().cpu()
        rel = 1e-9 if P == torch.float64 else 4 * ULP[P]
        assert ((a + c - ref).abs() <= 1e-9 + rel * (a.abs() + c.abs())).all(), what
    close_p(wdg, dgain, "dgain")
    close_p(wdb, dbias, "dbias")


# ---------------------------------------------------------------------------------- embedding
VOCAB = 6
# truncation toward zero, then negative ids count from the end: 2, 0, 5, 5, 3, 0, 1
IDS = [2.9, -0.5, -1.0, 5.2, -3.7, 0.999, -5.99]


@pytest.mark.parametrize("id_dtype", [torch.int64, torch.float32, torch.float64], ids=["i64", "f32", "f64"])
@pytest.mark.parametrize("n_idx", [5, 7])
@pytest.mark.parametrize("dim", [10, 70, 130])
@pytest.mark.parametrize("tt,to", [(torch.float32, torch.float32), (torch.bfloat16, torch.float32),
                                   (torch.float32, torch.bfloat16), (torch.float64, torch.float64)],
                         ids=["f32-f32", "bf16-f32", "f32-bf16", "f64-f64"])
def test_embedding_forward_id_and_table_dtypes(native_lib, id_dtype, n_idx, dim, tt, to):
    g = torch.Generator(device="cpu").manual_seed(dim + n_idx)
    table = torch.randn(VOCAB, dim, generator=g, dtype=torch.float64).to(tt)
    raw = torch.tensor(IDS[:n_idx], dtype=torch.float64)
    ids = raw.long() if id_dtype == torch.int64 else raw.to(id_dtype)  # float ids keep their fractions
    assert raw.long().tolist() == [2, 0, -1, 5, -3, 0, -5][:n_idx]
    out = torch.full((n_idx, dim), 7.0, dtype=to, device=DEV)
    torch.ops.pz.embedding_fwd(table.to(DEV), ids.to(DEV), out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), table[raw.long()].to(to))


@pytest.mark.parametrize("tg,tt,id_dtype", [(torch.float32, torch.float32, torch.int64),
                                            (torch.bfloat16, torch.float32, torch.float32),
                                            (torch.float64, torch.float64, torch.float64)],
                         ids=["f32", "bf16", "f64"])
def test_embedding_backward_accumulates_duplicates(native_lib, tg, tt, id_dtype):
    """257 ids over 5 rows, 200 of them the same row, into a non-zero dtable. fp32 accumulation:
    count ordered additions err by at most count * 2^-24 * sum|terms| whatever the order the
    atomics arrive in; a row nobody indexes stays bit-identical."""
    vocab, dim, n = 5, 70, 257
    g = torch.Generator(device="cpu").manual_seed(7)
    ids = torch.cat([torch.full((200,), 3), torch.tensor([0, 1, 2, -4, -5])[torch.randint(0, 5, (57,), generator=g)]])
    ids = ids[torch.randperm(n, generator=g)]
    dout = torch.randn(n, dim, generator=g, dtype=torch.float64).to(tg)
    dtable0 = torch.randn(vocab, dim, generator=g, dtype=torch.float64).to(tt)
    fids = ids.to(id_dtype)
    if id_dtype != torch.int64:
        fids = fids + torch.where(ids >= 0, 0.4, -0.4)  # fractions that truncation drops
    dtable = dtable0.clone().to(DEV)
    torch.ops.pz.embedding_bwd(dout.to(DEV), fids.to(DEV), dtable)
    torch.cuda.synchronize()
    rows = ids % vocab
    ref = dtable0.double().index_add_(0, rows, dout.double())
    got = dtable.cpu()
    assert bit_equal(got[4], dtable0[4]) and (rows != 4).all()
    if tt == torch.float64:
        torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
        return
    count = torch.bincount(rows, minlength=vocab).double()
    mag = dtable0.double().abs().index_add_(0, rows, dout.double().abs())
    err = (got.double() - ref).abs()
    assert (err <= count[:, None] * 2.0 ** -24 * mag).all(), err.max().item()
