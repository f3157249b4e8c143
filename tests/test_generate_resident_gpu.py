"""``generate(loop="resident")``: the whole request as one launch of ``pz::generate_resident``
(csrc/generate_resident.hip), the model held in every row's workgroup LDS.

Two facts are checked separately. (1) The tokens are the sampler's: for every step the kernel's
token equals what ``PF.sample_rows`` draws from the kernel's own logits (``logits_out``), exactly,
because both run the code of csrc/sample_core.h on the same bits. (2) The logits are the model's:
teacher-forced, each step's logits against an fp64 torch forward of the window that preceded it; the
resident error may be at most twice the error of ``FusedPredictor._logits`` (the per-token loop's
forward, not code under test) on the same windows, plus 1e-6 — the factor covers bf16 rounding flips
on a small sample.

Measured on an MI355X (max abs error against fp64, resident / ``_logits``):
    A [27, 10, 30, 64, 27] float32    3.274e-07 / 6.197e-07      bfloat16  7.158e-03 / 7.158e-03
    B [27, 4, 8, 16, 32, 27] float32  3.016e-07 / 5.903e-07
    C [300, 6, 18, 40, 300] bfloat16  1.611e-02 / 1.611e-02
    D (A without biases) float32      2.648e-07 / 5.743e-07
    E [27, 5, 15, 100, 27] bfloat16   3.940e-03 / 3.940e-03
"""
import pytest
import torch

from penr_oz_neural_network_torch_amd.engine.resident import H_TOTAL, HEAD
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF

pytestmark = pytest.mark.gpu

SEED = 11 + (22 << 32)
KEY = (11, 22)
STEPS = 20
CHAR_SIZES = [27, 10, 30, 64, 27]
CHAR_ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]
SPECS = {  # name: (sizes, algos, bias_algo, dtype, contexts)
    "A32": (CHAR_SIZES, CHAR_ALGOS, "random", "float32", [[0, 0, 5], [1, 2, 3], [4, 5, 6]]),
    "A16": (CHAR_SIZES, CHAR_ALGOS, "random", "bfloat16", [[0, 0, 5], [1, 2, 3], [4, 5, 6]]),
    "B": ([27, 4, 8, 16, 32, 27], ["embedding", "flatten", "linear", "tanh", "flatten", "linear", "softmax"], "random",
          "float32", [[0, 0, 5, 7], [1, 2, 3, 4], [26, 5, 6, 0]]),
    "C": ([300, 6, 18, 40, 300], ["embedding", "linear", "relu", "linear", "softmax"], "random", "bfloat16",
          [[0, 299, 5], [100, 2, 3], [4, 150, 6]]),
    "D": (CHAR_SIZES, CHAR_ALGOS, None, "float32", [[0, 0, 5], [1, 2, 3], [4, 5, 6]]),
    # beyond the issue's list: 100 outputs (two K groups over an odd K = 15, ranges of 8 and 7) and sigmoid
    "E": ([27, 5, 15, 100, 27], ["embedding", "linear", "sigmoid", "linear", "softmax"], "random", "bfloat16",
          [[0, 0, 5], [1, 2, 3], [4, 5, 6]]),
}
MODES = {"greedy": dict(temperature=0.0), "t0.8": dict(temperature=0.8), "top7": dict(temperature=1.0, top_k=7),
         "top1": dict(temperature=1.0, top_k=1)}


def _build(name):
    sizes, algos, bias_algo, dtype, contexts = SPECS[name]
    torch.manual_seed(9)
    model = NeuralNetworkModel(name, sizes, activation_algos=algos, bias_algo=bias_algo, dtype=dtype, device="cuda:0")
    if "batchnorm" in algos:  # a training-mode forward first, so the running statistics are not the initial 0 / 1
        g = torch.Generator().manual_seed(4)
        ids = torch.randint(0, sizes[0], (100, len(contexts[0])), generator=g)
        model.compute_output(ids.tolist(), [[int(i)] for i in torch.randint(0, sizes[-1], (100,), generator=g)])
    model.generate(contexts, 1, seed=1)  # (the predictor exists)
    return model


@pytest.fixture(scope="module")
def models(native_lib):
    return {name: _build(name) for name in SPECS}


def _run(model, contexts, steps=STEPS, with_logits=True, **kw):
    """(tokens [rows, steps] on the host, logits [rows, steps, V] or None) of one resident launch."""
    pred = model._predictor
    buf = None
    if with_logits:
        buf = torch.zeros(len(contexts), steps, pred.stages[-1].out_width, device=pred.dev, dtype=torch.float32)
    kw.setdefault("seed", KEY)
    tokens = pred.generate_resident(torch.tensor(contexts), steps, logits_out=buf, **kw)
    return tokens.cpu(), buf


def _sampler_tokens(buf, row0=0, **kw):
    """What PF.sample_rows draws from each step's logits."""
    rows, steps, _ = buf.shape
    seq = torch.full((rows, steps), -7, device=buf.device, dtype=torch.int64)
    done = torch.zeros(rows, device=buf.device, dtype=torch.int32)
    for s in range(steps):
        PF.sample_rows(buf[:, s].contiguous(), seq, done, s, seed=KEY, step=s, row0=row0, **kw)
    return seq.cpu()


# ---------------------------------------------------------------------------------------------
# 1. the tokens are the sampler's
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["A32", "A16", "B", "C", "E"])
def test_tokens_are_what_sample_rows_draws_from_the_kernels_logits(models, name, mode):
    model, contexts = models[name], SPECS[name][4]
    tokens, buf = _run(model, contexts, **MODES[mode])
    assert tokens.shape == (3, STEPS) and int(tokens.min()) >= 0 and int(tokens.max()) < SPECS[name][0][-1]
    assert torch.isfinite(buf).all() and float(buf.abs().max()) > 0
    assert torch.equal(tokens, _sampler_tokens(buf, **MODES[mode]))
    if mode in ("greedy", "top1") and name != "C":  # (bf16 logits of 300 classes may tie at the maximum: top-1 keeps ties)
        assert torch.equal(tokens, buf.argmax(-1).cpu())


# ---------------------------------------------------------------------------------------------
# 2. the logits are the model's
# ---------------------------------------------------------------------------------------------
def _reference_logits(model, x) -> torch.Tensor:
    """fp64 torch forward from the master parameters, layers in eval mode, stopping before the softmax."""
    h = torch.as_tensor(x)
    for layer in model.layers:
        a = layer.algo
        if a == "embedding":
            h = layer.weights.detach().double().cpu()[h.long()]
        elif a == "flatten":
            h = layer.forward(h)
        elif a == "linear":
            h = h.double() @ layer.weights.detach().double().cpu()
            if layer.bias is not None:
                h = h + layer.bias.detach().double().cpu()
        elif a == "batchnorm":
            mean, var = layer.mean.detach().double().cpu().reshape(-1), layer.variance.detach().double().cpu().reshape(-1)
            h = layer.gain.detach().double().cpu() * (h - mean) / torch.sqrt(var + layer.eps) + layer.bias.detach().double().cpu()
        elif a == "softmax":
            break
        else:
            h = getattr(h, a)()
    return h


@pytest.mark.parametrize("name", list(SPECS))
def test_logits_are_the_models_teacher_forced(models, name):
    model, contexts = models[name], SPECS[name][4]
    length, classes = len(contexts[0]), SPECS[name][0][-1]
    tokens, buf = _run(model, contexts, temperature=0.8)
    got = buf.double().cpu()
    err_res = err_loop = 0.0
    for s in range(STEPS):
        windows = [(c + row)[s:s + length] for c, row in zip(contexts, tokens.tolist())]
        ref = _reference_logits(model, windows).reshape(3, classes)
        loop = model._predictor._logits(torch.tensor(windows)).double().cpu().reshape(3, classes)
        err_res = max(err_res, (got[:, s] - ref).abs().max().item())
        err_loop = max(err_loop, (loop - ref).abs().max().item())
    print(f"\n[resident logits] {name} {SPECS[name][3]}: resident {err_res:.3e}  _logits {err_loop:.3e}")
    assert err_res <= 2.0 * err_loop + 1e-6


# ---------------------------------------------------------------------------------------------
# 3 - 5. reproducibility, row independence, row counts, one token
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A16", "B"])
def test_two_calls_are_bit_identical_and_rows_are_independent(models, name):
    model, contexts = models[name], SPECS[name][4]
    t1, b1 = _run(model, contexts, temperature=0.8, top_k=9)
    t2, b2 = _run(model, contexts, temperature=0.8, top_k=9)
    assert torch.equal(t1, t2) and torch.equal(b1.view(torch.int32), b2.view(torch.int32))
    other = [contexts[0], contexts[2][::-1], contexts[1][::-1]]
    t3, b3 = _run(model, other, temperature=0.8, top_k=9)
    assert torch.equal(t3[0], t1[0]) and torch.equal(b3[0].view(torch.int32), b1[0].view(torch.int32))
    assert not torch.equal(t3[1:], t1[1:])


def test_row_counts_agree_row_by_row(models):
    model = models["A16"]
    g = torch.Generator().manual_seed(3)
    contexts = torch.randint(0, 27, (70, 3), generator=g).tolist()
    t70, b70 = _run(model, contexts)
    for rows in (1, 3):
        t, b = _run(model, contexts[:rows])
        assert torch.equal(t, t70[:rows]) and torch.equal(b.view(torch.int32), b70[:rows].view(torch.int32))
    assert len({tuple(r) for r in t70.tolist()}) > 60  # (rows draw their own numbers)


def test_negative_context_ids_count_from_the_end(models):
    model = models["A32"]
    want, want_buf = _run(model, [[26, 2, 3], [1, 25, 0]])
    got, got_buf = _run(model, [[-1, 2, 3], [1, -2, -27]])
    assert torch.equal(got, want) and torch.equal(got_buf.view(torch.int32), want_buf.view(torch.int32))
    assert model.generate([[-1, 2, 3]], 5, seed=SEED, loop="resident") == model.generate([[26, 2, 3]], 5, seed=SEED, loop="resident")


def test_one_new_token(models):
    model, contexts = models["A32"], SPECS["A32"][4]
    t1, b1 = _run(model, contexts, steps=1)
    t20, b20 = _run(model, contexts)
    assert t1.shape == (3, 1) and torch.equal(t1, t20[:, :1]) and torch.equal(b1.view(torch.int32), b20[:, :1].view(torch.int32))
    out = model.generate(contexts, 1, seed=SEED, loop="resident")
    assert out["tokens"] == t1.tolist()


# ---------------------------------------------------------------------------------------------
# 6. stop_token
# ---------------------------------------------------------------------------------------------
def test_stop_token_cuts_rows_inclusively(models):
    model, contexts = models["A16"], SPECS["A16"][4]
    free = model.generate(contexts, 40, seed=SEED, loop="resident")["tokens"]
    stop = free[0][3]
    cut = model.generate(contexts, 40, seed=SEED, stop_token=stop, loop="resident")["tokens"]
    assert len(cut[0]) <= 4 and cut[0][-1] == stop
    raw, _ = _run(model, contexts, steps=40, with_logits=False, stop_token=stop)
    for before, after, full in zip(free, cut, raw.tolist()):
        if stop in before:
            at = before.index(stop)
            assert after == before[:at + 1]
            assert full == before[:at + 1] + [stop] * (39 - at)   # the raw tensor repeats it to the end
        else:
            assert after == before == full
    assert any(len(r) < 40 for r in cut)


# ---------------------------------------------------------------------------------------------
# 7. one launch
# ---------------------------------------------------------------------------------------------
def test_the_request_is_one_launch_and_one_download(models, monkeypatch):
    model, contexts = models["A16"], [[5], [1, 2, 3], [9, 9, 4, 5, 6]]
    model.generate(contexts, 2, seed=1, loop="resident")  # (plan made)
    reads, calls = [], {"resident": 0, "sample": 0, "skinny": 0, "checks": []}
    real = {n: getattr(torch.Tensor, n) for n in ("tolist", "item", "cpu")}
    real_res, real_check = PF.generate_resident, PF.check_index_range

    def spy(name):
        def wrapped(self, *a, **kw):
            if self.is_cuda:
                reads.append(name)
            return real[name](self, *a, **kw)
        return wrapped

    def counted(key, fn=None):
        def wrapped(*a, **kw):
            calls[key] += 1
            assert not reads  # nothing was read before the launch
            return fn(*a, **kw) if fn else None
        return wrapped

    def spy_check(idx, *a, **kw):
        calls["checks"].append(idx.is_cuda)
        return real_check(idx, *a, **kw)

    for n in real:
        monkeypatch.setattr(torch.Tensor, n, spy(n))
    monkeypatch.setattr(PF, "generate_resident", counted("resident", real_res))
    monkeypatch.setattr(PF, "sample_rows", counted("sample"))
    monkeypatch.setattr(PF, "gemm_skinny", counted("skinny"))
    monkeypatch.setattr(PF, "check_index_range", spy_check)
    out = model.generate(contexts, 16, seed=SEED, loop="resident")
    assert [len(r) for r in out["tokens"]] == [16, 16, 16]
    assert calls["resident"] == 1 and calls["sample"] == 0 and calls["skinny"] == 0
    assert calls["checks"].count(True) == 1  # the context's range check, once
    assert reads == ["tolist"]               # the one download


# ---------------------------------------------------------------------------------------------
# 8. the embedding table in global memory
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A32", "A16"])
def test_table_in_global_memory_gives_the_same_bits(models, name):
    model, contexts = models[name], SPECS[name][4]
    pred = model._predictor
    full = pred.resident_plan()
    lean = pred.resident_plan(budget=full.total - 1)
    assert full.table_in_lds and not lean.table_in_lds and lean.total < full.total
    want_t, want_b = _run(model, contexts, temperature=0.8)
    seq = torch.zeros(3, 3 + STEPS, device=pred.dev, dtype=torch.int64)
    seq[:, :3] = torch.tensor(contexts)
    done = torch.zeros(3, device=pred.dev, dtype=torch.int32)
    buf = torch.zeros_like(want_b)
    PF.generate_resident(seq, done, pred.resident_params(lean), lean.ints, STEPS, seed=KEY, temperature=0.8, logits_out=buf)
    assert torch.equal(seq[:, 3:].cpu(), want_t) and torch.equal(buf.view(torch.int32), want_b.view(torch.int32))


# ---------------------------------------------------------------------------------------------
# 9. weights="fp8"
# ---------------------------------------------------------------------------------------------
def test_fp8_weights(models):
    model, contexts = models["A16"], SPECS["A16"][4]
    tokens, buf = _run(model, contexts, temperature=0.8, weights="fp8")
    assert torch.equal(tokens, _sampler_tokens(buf, temperature=0.8))
    plain, plain_buf = _run(model, contexts, temperature=0.8)
    assert not torch.equal(buf, plain_buf)  # (other weights)
    assert model.generate(contexts, STEPS, temperature=0.8, seed=SEED, weights="fp8", loop="resident")["tokens"] == tokens.tolist()
    with pytest.raises(ValueError, match="fp8"):
        models["A32"].generate(contexts, 4, weights="fp8", loop="resident")


# ---------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(models, monkeypatch):
    launches = []
    real = PF.generate_resident
    monkeypatch.setattr(PF, "generate_resident", lambda *a, **kw: (launches.append(1), real(*a, **kw))[1])
    dense = NeuralNetworkModel("dense", [9, 18, 9], activation_algos=["relu", "sigmoid"], device="cuda:0")
    with pytest.raises(ValueError, match="embedding"):
        dense.generate([[1, 2, 3]], 4, loop="resident")
    headless = NeuralNetworkModel("headless", [27, 10, 30, 27], activation_algos=["embedding", "linear", "tanh"],
                                  device="cuda:0")
    with pytest.raises(ValueError, match="softmax"):
        headless.generate([[1, 2, 3]], 4, loop="resident")
    big = NeuralNetworkModel("big", [27, 64, 192, 1024, 27], activation_algos=["embedding", "linear", "tanh", "linear", "softmax"],
                             dtype="float32", device="cuda:0")
    with pytest.raises(ValueError, match=r"loop='resident' is not available.*needs \d+ bytes of LDS.*budget of 163840"):
        big.generate([[1, 2, 3]], 4, loop="resident")
    assert len(big.generate([[1, 2, 3]], 4)["tokens"][0]) == 4  # (the per-token loop takes it)
    with pytest.raises(ValueError, match="unknown loop"):
        models["A32"].generate([[1, 2, 3]], 4, loop="lds")
    with pytest.raises(IndexError):
        models["A32"].generate([[1, 2, 27]], 4, loop="resident")
    with pytest.raises(IndexError):
        models["A32"]._predictor.generate_resident(torch.tensor([[1, 2, 27]]), 4)
    assert not launches


def test_the_op_refuses_a_plan_that_does_not_fit(models):
    pred = models["A32"]._predictor
    plan = pred.resident_plan()
    params = pred.resident_params(plan)

    def call(ints=plan.ints, tensors=params, steps=4, cols=7, **kw):
        seq = torch.full((2, cols), -7, device=pred.dev, dtype=torch.int64)
        seq[:, :3] = 1
        done = torch.zeros(2, device=pred.dev, dtype=torch.int32)
        try:
            PF.generate_resident(seq, done, tensors, ints, steps, seed=KEY, **kw)
        finally:
            torch.cuda.synchronize()
        return seq

    assert int(call()[:, 3:].min()) >= 0  # (the plan as made runs)
    bad = {}
    bad["total beyond the device"] = dict(ints=[10 ** 6 if i == H_TOTAL else v for i, v in enumerate(plan.ints)])
    bad["offset beyond the total"] = dict(ints=[plan.total if i == HEAD + 3 else v for i, v in enumerate(plan.ints)])
    bad["misaligned offset"] = dict(ints=[v + 4 if i == HEAD + 3 else v for i, v in enumerate(plan.ints)])
    bad["overlapping regions"] = dict(ints=[plan.ints[HEAD + 6] if i == HEAD + 3 else v for i, v in enumerate(plan.ints)])
    bad["short parameter"] = dict(tensors=[params[0], params[1].reshape(-1)[:-1].clone()] + params[2:])
    bad["wrong dtype"] = dict(tensors=[params[0], params[1].bfloat16()] + params[2:])
    bad["missing parameter"] = dict(tensors=params[:-1])
    bad["seq width"] = dict(cols=8)
    bad["no steps"] = dict(steps=0, cols=3)
    bad["too many steps"] = dict(steps=4097, cols=4100)
    bad["truncated plan"] = dict(ints=plan.ints[:-1])
    bad["logits_out shape"] = dict(logits_out=torch.zeros(2, 4, 28, device=pred.dev))
    for what, kw in bad.items():
        with pytest.raises(RuntimeError):
            call(**kw)
            pytest.fail(f"accepted: {what}")
    # a refused call wrote nothing
    seq = torch.full((2, 7), -7, device=pred.dev, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        PF.generate_resident(seq, torch.zeros(2, device=pred.dev, dtype=torch.int32), params[:-1], plan.ints, 4, seed=KEY)
    torch.cuda.synchronize()
    assert int(seq.max()) == -7
