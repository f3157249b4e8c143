"""``NeuralNetworkModel.generate`` on the GPU: the device-resident loop of
``FusedPredictor.generate`` (forward kernels on the window ``seq[:, s : s + L]`` plus one
``pz::sample_rows`` launch per token).

The teacher-forced check recomputes, for every generated position, the distribution of the window
that preceded it and requires the token to satisfy the inverse-CDF rule in fp64: it is the token of
``PF.sample_rows_reference``, or ``u`` lies within ``eps`` of the fp64 CDF boundary between the two
and the token is the neighbour on the other side. ``eps`` = 1e-5 (the sampling kernel's summation
bound, tests/test_sample_gpu.py) plus, for the float32 model checked through ``predict()``, the
1.4e-7 by which that model's predictions differ from fp64 (tests/test_predict_gpu.py's header). The
bfloat16 model is checked against the predictor's own fp32 logits (``_logits``), the exact input of
the sampling launch, with eps = 1e-5."""
import pytest
import torch

from penr_oz_neural_network_torch_amd.engine.predictor import FusedPredictor
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF

pytestmark = pytest.mark.gpu

CHAR_SIZES = [27, 10, 30, 64, 27]
CHAR_ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]
CONTEXTS = [[5], [1, 2, 3], [9, 9, 4, 5, 6]]     # padded, exact, truncated
WINDOWS = [[0, 0, 5], [1, 2, 3], [4, 5, 6]]
SEED = 11 + (22 << 32)
KEY = (11, 22)


def _char_model(dtype):
    torch.manual_seed(9)
    model = NeuralNetworkModel("chars", CHAR_SIZES, activation_algos=CHAR_ALGOS, bias_algo="random", dtype=dtype,
                               device="cuda:0")
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 27, (100, 3), generator=g)
    # a training-mode forward first, so the running statistics are not the initial 0 / 1
    model.compute_output(ids.tolist(), [[int(i)] for i in torch.randint(0, 27, (100,), generator=g)])
    return model


@pytest.fixture(scope="module")
def models(native_lib):
    return {dtype: _char_model(dtype) for dtype in ("float32", "bfloat16")}


def _teacher_forced(model, tokens, eps, from_logits, weights=None):
    near = 0
    for s in range(len(tokens[0])):
        windows = [(w + row)[s:s + 3] for w, row in zip(WINDOWS, tokens)]
        if from_logits:
            lg = model._predictor._logits(torch.tensor(windows), weights == "fp8").double().cpu()
        else:
            lg = torch.tensor(model.predict(windows), dtype=torch.float64).log()
        ref = PF.sample_rows_reference(lg, KEY, s)
        cdf = lg.softmax(-1).cumsum(-1)
        for r in range(len(tokens)):
            t, want = tokens[r][s], int(ref[r])
            assert 0 <= t < 27
            if t != want:
                assert abs(t - want) == 1, (s, r, t, want)
                u = PF.sample_uniform(KEY, r, s)
                assert abs(float(cdf[r, min(t, want)]) - u) <= eps, (s, r, t, want)
                near += 1
    return near


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_generate_follows_the_rule_on_every_window(models, dtype):
    model = models[dtype]
    out = model.generate(CONTEXTS, 20, seed=SEED)
    assert isinstance(model._predictor, FusedPredictor) and model._predictor.context_length == 3
    assert out["seed"] == SEED and [len(r) for r in out["tokens"]] == [20, 20, 20]
    if dtype == "float32":
        near = _teacher_forced(model, out["tokens"], 1e-5 + 1.4e-7, from_logits=False)
    else:
        near = _teacher_forced(model, out["tokens"], 1e-5, from_logits=True)
    print(f"{dtype}: {near} of 60 tokens passed by the boundary clause")
    assert near <= 3


def test_seeds_name_their_output(models):
    model = models["float32"]
    a = model.generate(CONTEXTS, 20, seed=SEED)
    assert a == model.generate(CONTEXTS, 20, seed=SEED)
    assert a["tokens"] != model.generate(CONTEXTS, 20, seed=SEED + 1)["tokens"]
    greedy = model.generate(CONTEXTS, 8, temperature=0, seed=1)["tokens"]
    assert greedy == model.generate(CONTEXTS, 8, temperature=0, seed=2)["tokens"]
    assert greedy == model.generate(CONTEXTS, 8, top_k=1, seed=3)["tokens"]
    for r, w in enumerate(WINDOWS):  # the first greedy token is predict()'s most likely class
        probs = torch.tensor(model.predict([w])[0])
        assert probs[greedy[r][0]] == probs.max()


def test_stop_token_cuts_rows_inclusively(models):
    model = models["float32"]
    free = model.generate(CONTEXTS, 40, seed=SEED)["tokens"]
    stop = free[0][3]
    cut = model.generate(CONTEXTS, 40, seed=SEED, stop_token=stop)["tokens"]
    for before, after in zip(free, cut):
        assert after == (before[:before.index(stop) + 1] if stop in before else before)
    assert len(cut[0]) <= 4 and cut[0][-1] == stop
    raw = model._predictor.generate(torch.tensor(WINDOWS), 40, seed=KEY, stop_token=stop)
    assert raw.shape == (3, 40) and raw.dtype == torch.int64 and raw.is_cuda
    assert raw[0, len(cut[0]) - 1:].tolist() == [stop] * (41 - len(cut[0]))  # a finished row repeats the stop token


def test_fp8_weights_on_bf16_models_only(models):
    out = models["bfloat16"].generate(CONTEXTS, 20, seed=SEED, weights="fp8")
    assert [len(r) for r in out["tokens"]] == [20, 20, 20]
    assert _teacher_forced(models["bfloat16"], out["tokens"], 1e-5, from_logits=True, weights="fp8") <= 3
    assert models["bfloat16"]._predictor.weights8  # the e4m3 copies were built and used
    with pytest.raises(ValueError, match="fp8"):
        models["float32"].generate(CONTEXTS, 4, weights="fp8")


def test_models_that_cannot_generate_and_bad_ids_raise(models):
    dense = NeuralNetworkModel("dense", [9, 18, 9], activation_algos=["relu", "sigmoid"], dtype="float32", device="cuda:0")
    with pytest.raises(ValueError, match="embedding"):
        dense.generate([[1, 2, 3]], 4)
    with pytest.raises(ValueError, match="embedding"):
        FusedPredictor(dense).generate(torch.tensor([[1, 2, 3]]), 4)
    headless = NeuralNetworkModel("headless", [27, 10, 30, 27], activation_algos=["embedding", "linear", "tanh"],
                                  dtype="float32", device="cuda:0")
    with pytest.raises(ValueError, match="softmax"):
        headless.generate([[1, 2, 3]], 4)
    with pytest.raises(ValueError, match="softmax"):
        FusedPredictor(headless).generate(torch.tensor([[1, 2, 3]]), 4)
    with pytest.raises(IndexError):
        models["float32"].generate([[1, 2, 27]], 4)
    predictor = models["float32"]._fused_predictor()
    with pytest.raises(IndexError):
        predictor.generate(torch.tensor([[1, 2, 27]]), 4)
    with pytest.raises(ValueError):
        predictor.generate(torch.tensor([[1, 2]]), 4)  # not context_length ids per row


def test_the_loop_reads_nothing_back(models, monkeypatch):
    model = models["bfloat16"]
    model.generate(CONTEXTS, 2, seed=1)  # (predictor and weight copies exist)
    reads, checks, launches = [], [], []
    real_tolist, real_item, real_cpu = torch.Tensor.tolist, torch.Tensor.item, torch.Tensor.cpu
    real_check, real_sample = PF.check_index_range, PF.sample_rows

    def spy(name, real):
        def wrapped(self, *a, **kw):
            if self.is_cuda:
                reads.append(name)
            return real(self, *a, **kw)
        return wrapped

    def spy_check(idx, *a, **kw):
        checks.append(idx.is_cuda)
        return real_check(idx, *a, **kw)

    def spy_sample(*a, **kw):
        launches.append(len(reads))
        return real_sample(*a, **kw)

    monkeypatch.setattr(torch.Tensor, "tolist", spy("tolist", real_tolist))
    monkeypatch.setattr(torch.Tensor, "item", spy("item", real_item))
    monkeypatch.setattr(torch.Tensor, "cpu", spy("cpu", real_cpu))
    monkeypatch.setattr(PF, "check_index_range", spy_check)
    monkeypatch.setattr(PF, "sample_rows", spy_sample)
    out = model.generate(CONTEXTS, 16, seed=SEED)
    assert [len(r) for r in out["tokens"]] == [16, 16, 16]
    assert checks.count(True) == 1            # the context's range check, once, before the loop
    assert len(launches) == 16 and launches == [0] * 16  # one sampling launch per token, no host read before the last
    assert reads == ["tolist"]                # the one download
