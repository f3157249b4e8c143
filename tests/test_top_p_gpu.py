"""Nucleus (top-p) and min-p sampling on the GPU: ``pz::sample_rows`` and ``pz::generate_resident``
(csrc/sample_core.h: ``nucleus_key``, ``Weigher``) against ``PF.sample_rows_reference``.

A token must be the fp64 reference's, unless (1) ``u`` lies within ``EPS`` of the fp64 CDF boundary
between the two and the token is the kept neighbour on the other side (the clause of
``test_sample_gpu.py``), or (2) the nucleus itself is ambiguous in fp64: some column's strictly-above
mass lies within ``eps_p * S0`` of ``top_p * S0`` or its weight within ``eps_p`` (relative) of
``min_p``; the token must then still come from the reference's nucleus widened by the ambiguous
columns. ``EPS = 1e-5``, ``eps_p(V) = 1e-5 + V * 2^-32``: ``tests/top_p_cases.py`` derives both from the
kernel's arithmetic and holds the fixed-seed inputs; ``test_top_p_cpu.py`` proves that the fp64
reference alone leaves at most 2 % of any case's draws and at most 5 % of the cases ambiguous, and a
clause can only be used on an ambiguous draw. The hand-checkable rows, reproducibility, row
independence, the off values, the stop token and the resident loop's tokens are exact."""
import pytest
import torch

from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import top_p_cases as C

pytestmark = pytest.mark.gpu

SEED = C.SEED
DEV = "cuda:0"
CHAR_SIZES = [27, 10, 30, 64, 27]
CHAR_ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]
WINDOWS = [[0, 0, 5], [1, 2, 3], [4, 5, 6]]
CASES = C.cases()
_used = {}  # case name -> draws passed by a boundary clause


def _draw(logits_dev, steps, stop_token=None, row0=0, done=None, first_step=0, **kw):
    rows = logits_dev.shape[0]
    seq = torch.full((rows, steps), -7, device=DEV, dtype=torch.int64)
    done = torch.zeros(rows, device=DEV, dtype=torch.int32) if done is None else done.to(DEV)
    for s in range(steps):
        PF.sample_rows(logits_dev, seq, done, s, seed=SEED, step=first_step + s, stop_token=stop_token, row0=row0, **kw)
    return seq.cpu(), done.cpu()


# --------------------------------------------------------------------------------------------
# PF.sample_rows against the reference
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sample_rows_agrees_with_the_fp64_reference(native_lib, case):
    name, kind, rows, cols, seed, kw = case
    lg = C.make_logits(kind, rows, cols, seed)
    got, _ = _draw(lg.to(DEV), C.STEPS, **kw)
    assert int(got.min()) >= 0 and int(got.max()) < cols
    near = C.check_draws(lg, got, kw)
    _used[name] = near
    print(f"{name}: {near} of {rows * C.STEPS} draws ({100.0 * near / (rows * C.STEPS):.2f} %) passed by a boundary clause")
    assert near <= C.CAP_DRAWS * rows * C.STEPS


def test_few_cases_use_a_boundary_clause(native_lib):
    for name, kind, rows, cols, seed, kw in CASES:  # (a case the run did not select is drawn here)
        if name not in _used:
            lg = C.make_logits(kind, rows, cols, seed)
            _used[name] = C.check_draws(lg, _draw(lg.to(DEV), C.STEPS, **kw)[0], kw)
    users = [name for name, _, *_ in CASES if _used[name] > 0]
    print(f"{len(users)} of {len(CASES)} cases used a boundary clause: {users}")
    assert len(users) <= C.CAP_CASES * len(CASES)


# --------------------------------------------------------------------------------------------
# exact cases
# --------------------------------------------------------------------------------------------
def _drawn(row, n=4096, **kw):
    got, _ = _draw(row.repeat(n // 2, 1).to(DEV), 2, **kw)
    return set(got.flatten().tolist())


def test_hand_checkable_rows(native_lib):
    row, order = C.hand_row(), C.HAND_ORDER  # probabilities 1/2, 1/4, 1/8, 1/16, 1/16 in a permuted column order
    assert _drawn(row, top_p=0.6) == set(order[:2])
    assert _drawn(row, top_p=0.5) == set(order[:1])
    assert _drawn(row, top_p=0.76) == set(order[:3])
    assert _drawn(row, top_p=0.9) == set(order)
    assert _drawn(row, min_p=0.2) == set(order[:3])
    assert _drawn(row, top_k=3, top_p=0.9) == set(order[:3])
    assert _drawn(row, top_k=3, top_p=0.85) == set(order[:2])
    assert _drawn(row, min_p=0.2, top_p=0.85) == set(order[:2])
    ties = torch.tensor([0.0, 2.0, -1.0, 2.0, 2.0, 0.5, 2.0])
    assert _drawn(ties, top_p=0.1) == {1, 3, 4, 6}
    # the same rows inside a wide row of -inf and of far lighter columns, on 4 and on 16 waves
    for cols in (8192, 8193):
        wide = torch.full((cols,), float("-inf"))
        wide[1::2] = -40.0
        at = torch.tensor([7, 4001, 64, cols - 1, 130])
        wide[at] = row
        assert _drawn(wide, n=1024, top_p=0.6) == set(at[order[:2]].tolist())
        assert _drawn(wide, n=1024, top_p=0.76) == set(at[order[:3]].tolist())
        assert _drawn(wide, n=1024, min_p=0.2) == set(at[order[:3]].tolist())


@pytest.mark.parametrize("cols", [1000, 8193])
def test_reproducible_and_independent_of_the_other_rows(native_lib, cols):
    kw = dict(temperature=0.9, top_k=300, top_p=0.8, min_p=0.001)
    dev = C.make_logits("gauss", 64, cols, 4).div(3.0).to(DEV)
    a, _ = _draw(dev, 3, **kw)
    b, _ = _draw(dev, 3, **kw)
    assert torch.equal(a, b)
    for r in range(0, 64, 7):  # the same logits sent alone, as row r of the request
        alone, _ = _draw(dev[r:r + 1].contiguous(), 3, row0=r, **kw)
        assert alone[0].tolist() == a[r].tolist(), r
    part, _ = _draw(dev[20:40].contiguous(), 3, row0=20, **kw)
    assert torch.equal(part, a[20:40])
    assert len(set(a[:, 0].tolist())) > 1


@pytest.mark.parametrize("kw", [{}, {"top_k": 40}, {"temperature": 0.0}])
def test_off_values_change_nothing(native_lib, kw):
    dev = C.make_logits("gauss", 64, 4097, 5).to(DEV)
    plain, _ = _draw(dev, 3, **kw)
    off, _ = _draw(dev, 3, top_p=1.0, min_p=0.0, **kw)
    assert torch.equal(plain, off)
    if kw.get("temperature") == 0.0:  # greedy ignores both options
        assert torch.equal(_draw(dev, 3, top_p=0.3, min_p=0.5, **kw)[0], plain)


def test_stop_token_and_done_under_top_p(native_lib):
    dev = C.make_logits("gauss", 64, 27, 5).div(3.0).to(DEV)
    free, _ = _draw(dev, 2, top_p=0.8)
    stop = int(free[0, 0])
    got, done = _draw(dev, 2, stop_token=stop, top_p=0.8)
    hit = free[:, 0] == stop
    assert hit.any() and not hit.all()
    assert got[:, 0].tolist() == free[:, 0].tolist()
    assert torch.equal(got[hit, 1], torch.full_like(got[hit, 1], stop))
    assert torch.equal(got[~hit, 1], free[~hit, 1])
    assert done.bool().tolist() == (hit | (free[:, 1] == stop)).tolist()


# --------------------------------------------------------------------------------------------
# the bindings
# --------------------------------------------------------------------------------------------
BAD = [{"top_p": float("nan")}, {"top_p": 0.0}, {"top_p": 1.5}, {"min_p": float("nan")}, {"min_p": -0.1}, {"min_p": 1.0}]


def test_the_ops_refuse_bad_values_before_any_launch(native_lib, models):
    lg = C.make_logits("gauss", 4, 27, 0).to(DEV)
    seq = torch.zeros(4, 6, device=DEV, dtype=torch.int64)
    done = torch.zeros(4, device=DEV, dtype=torch.int32)
    PF.sample_rows(lg, seq, done, 5, seed=SEED, step=0, top_p=0.9, min_p=0.1)
    pred = models["float32"]._predictor
    for bad in BAD:
        with pytest.raises(RuntimeError, match="top_p|min_p"):
            PF.sample_rows(lg, seq, done, 0, seed=SEED, step=0, **bad)
        with pytest.raises(RuntimeError, match="top_p|min_p"):
            pred.generate_resident(torch.tensor(WINDOWS), 4, seed=SEED, **bad)
    torch.cuda.synchronize()
    assert seq[:, :5].abs().sum() == 0  # the refused calls wrote nothing


# --------------------------------------------------------------------------------------------
# the resident loop and the public API
# --------------------------------------------------------------------------------------------
def _char_model(dtype):
    torch.manual_seed(9)
    model = NeuralNetworkModel("chars", CHAR_SIZES, activation_algos=CHAR_ALGOS, bias_algo="random", dtype=dtype,
                               device="cuda:0")
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 27, (100, 3), generator=g)
    model.compute_output(ids.tolist(), [[int(i)] for i in torch.randint(0, 27, (100,), generator=g)])
    model.generate(WINDOWS, 1, seed=1)  # (the predictor exists)
    return model


@pytest.fixture(scope="module")
def models(native_lib):
    return {dtype: _char_model(dtype) for dtype in ("float32", "bfloat16")}


@pytest.mark.parametrize("kw", [dict(top_p=0.8), dict(top_p=0.8, top_k=5, min_p=0.05)], ids=["p", "pkm"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_resident_tokens_are_what_sample_rows_draws_from_the_kernels_logits(models, dtype, kw):
    pred = models[dtype]._predictor
    buf = torch.zeros(3, 16, 27, device=pred.dev, dtype=torch.float32)
    tokens = pred.generate_resident(torch.tensor(WINDOWS), 16, seed=SEED, logits_out=buf, **kw).cpu()
    assert tokens.shape == (3, 16) and torch.isfinite(buf).all() and float(buf.abs().max()) > 0
    seq = torch.full((3, 16), -7, device=pred.dev, dtype=torch.int64)
    done = torch.zeros(3, device=pred.dev, dtype=torch.int32)
    for s in range(16):
        PF.sample_rows(buf[:, s].contiguous(), seq, done, s, seed=SEED, step=s, **kw)
    assert torch.equal(tokens, seq.cpu())
    plain = pred.generate_resident(torch.tensor(WINDOWS), 16, seed=SEED).cpu()
    assert not torch.equal(tokens, plain)  # the options reached the kernel
    assert torch.equal(plain, pred.generate_resident(torch.tensor(WINDOWS), 16, seed=SEED, top_p=1.0, min_p=0.0).cpu())


@pytest.mark.parametrize("loop", [None, "resident"])
def test_generate_with_top_p_follows_the_reference_on_every_window(models, loop):
    """float32 model, teacher-forced against the fp64 rule on the per-token loop's own logits
    (``_logits``, the exact input of the sampling launch). The resident kernel's logits differ from
    those by fp32 summation order: 3.3e-7 + 6.2e-7 against fp64 as measured in
    test_generate_resident_gpu.py's header, under 1e-6 in a weight and 2e-6 in a normalised sum, which
    is the slack its bounds get."""
    model = models["float32"]
    extra = {} if loop is None else {"loop": loop}
    seed = 11 + (22 << 32)
    out = model.generate(WINDOWS, 16, seed=seed, top_p=0.8, **extra)
    assert out == model.generate(WINDOWS, 16, seed=seed, top_p=0.8, **extra)
    assert out["tokens"] != model.generate(WINDOWS, 16, seed=seed, **extra)["tokens"]
    tokens = torch.tensor(out["tokens"])
    near = 0
    for s in range(16):
        windows = [(w + row)[s:s + 3] for w, row in zip(WINDOWS, out["tokens"])]
        lg = model._predictor._logits(torch.tensor(windows)).reshape(3, 27).float().cpu()
        near += C.check_draws(lg, tokens[:, s:s + 1], dict(temperature=1.0, top_p=0.8), first_step=s,
                              slack=0.0 if loop is None else 2e-6)
    print(f"loop={loop}: {near} of 48 tokens passed by a boundary clause")
    assert near <= C.CAP_DRAWS * 48  # (2 % of 48 draws is less than one draw: none)


def test_the_loop_still_reads_nothing_back_under_top_p(models, monkeypatch):
    model = models["bfloat16"]
    reads, launches = [], []
    real_tolist, real_item, real_cpu, real_sample = torch.Tensor.tolist, torch.Tensor.item, torch.Tensor.cpu, PF.sample_rows

    def spy(name, real):
        def wrapped(self, *a, **kw):
            if self.is_cuda:
                reads.append(name)
            return real(self, *a, **kw)
        return wrapped

    def spy_sample(*a, **kw):
        launches.append((len(reads), kw.get("top_p"), kw.get("min_p")))
        return real_sample(*a, **kw)

    monkeypatch.setattr(torch.Tensor, "tolist", spy("tolist", real_tolist))
    monkeypatch.setattr(torch.Tensor, "item", spy("item", real_item))
    monkeypatch.setattr(torch.Tensor, "cpu", spy("cpu", real_cpu))
    monkeypatch.setattr(PF, "sample_rows", spy_sample)
    out = model.generate(WINDOWS, 16, seed=5, top_p=0.8, min_p=0.05, weights="fp8")
    assert [len(r) for r in out["tokens"]] == [16, 16, 16]
    assert launches == [(0, 0.8, 0.05)] * 16  # one sampling launch per token, no host read before the last
    assert reads == ["tolist"]                # the one download
