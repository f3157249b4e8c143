"""``NeuralNetworkModel.predict`` on the GPU: the forward-only schedule of
``engine/predictor.py`` (GEMM-dtype weights converted once, ``PF.gemm_skinny`` below 64 rows, the
tiled GEMMs with fused epilogues from 64 rows on).

Accuracy rule: against an fp64 torch forward from the fp32 masters, ``predict``'s max abs error
must be at most 2x the error of the existing ``compute_output`` on the same inputs, plus 1e-6 —
both are pipelines of the same precision, and a factor of 2 covers rounding flips on a small
sample.

Measured on an MI355X (max abs error of predict / of compute_output against fp64), bf16
[64,128,72,16] relu, tanh + softmax head: rows 1: 4.1e-4 / 7.9e-4, 5: 9.6e-4 / 1.6e-3, 16: 1.2e-3 / 2.4e-3,
40: 1.2e-3 / 3.1e-3, 64: 1.2e-3 / 3.1e-3, 200: 1.3e-3 / 3.9e-3; + sigmoid head: 1: 9.5e-4 / 1.3e-3,
5: 1.3e-3 / 2.7e-3, 16: 1.7e-3 / 2.7e-3, 40: 1.7e-3 / 2.9e-3, 64: 1.7e-3 / 3.3e-3, 200: 1.7e-3 / 3.3e-3;
float32 embedding + batchnorm model: rows 1: 1.2e-8 / 6.5e-8, 5: 2.5e-8 / 6.5e-8, 40: 8.5e-8 / 1.4e-7,
100: 1.4e-7 / 1.4e-7.
"""
import pytest
import torch

from penr_oz_neural_network_torch_amd.engine.predictor import FusedPredictor
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF

pytestmark = pytest.mark.gpu

ROWS = [1, 5, 16, 40, 64, 200]  # one vector; one chunk; a full chunk; three chunks; the tiled GEMMs


def _reference(model, x) -> torch.Tensor:
    """fp64 torch forward from the master parameters, layers in eval mode."""
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
            h = h.softmax(-1)
        else:
            h = getattr(h, a)()
    return h


def _errors(model, x):
    ref = _reference(model, x)
    got = torch.tensor(model.predict(x), dtype=torch.float64)
    old = torch.tensor(model.compute_output(x)[0], dtype=torch.float64)
    assert got.shape == ref.shape == old.shape
    return got, (got - ref).abs().max().item(), (old - ref).abs().max().item()


@pytest.fixture(scope="module")
def inputs():
    return torch.randn(200, 64, generator=torch.Generator().manual_seed(11))


@pytest.mark.parametrize("head", ["softmax", "sigmoid"])
def test_predict_is_as_accurate_as_compute_output(native_lib, inputs, head):
    torch.manual_seed(5)
    model = NeuralNetworkModel("acc", [64, 128, 72, 16], activation_algos=["relu", "tanh", head], bias_algo="random",
                               dtype="bfloat16", device="cuda:0")
    for rows in ROWS:
        x = inputs[0].tolist() if rows == 1 else inputs[:rows].tolist()
        got, err_new, err_old = _errors(model, x)
        print(f"{head} head, rows {rows}: predict err {err_new:.3e}, compute_output err {err_old:.3e}")
        assert err_new <= 2.0 * err_old + 1e-6, (rows, err_new, err_old)
        if head == "softmax":
            assert (got.sum(-1) - 1.0).abs().max().item() <= 1e-5
    assert isinstance(model._predictor, FusedPredictor)


def test_rows_below_64_run_the_skinny_kernel(native_lib, inputs, monkeypatch):
    """A silent fall-back to another GEMM must fail here: the calls are counted."""
    calls = {"skinny": [], "gemm": []}
    real_skinny, real_gemm = PF.gemm_skinny, PF.gemm

    def spy_skinny(x, w, out, **kw):
        calls["skinny"].append((x.shape[0], w.shape[1]))
        return real_skinny(x, w, out, **kw)

    def spy_gemm(a, a_kc, b, b_kc, out, **kw):
        calls["gemm"].append((out.shape[0], out.shape[1]))
        return real_gemm(a, a_kc, b, b_kc, out, **kw)

    monkeypatch.setattr(PF, "gemm_skinny", spy_skinny)
    monkeypatch.setattr(PF, "gemm", spy_gemm)
    torch.manual_seed(6)
    model = NeuralNetworkModel("spy", [64, 128, 72, 16], activation_algos=["relu", "tanh", "softmax"],
                               dtype="bfloat16", device="cuda:0")
    model.predict(inputs[0].tolist())
    assert calls == {"skinny": [(1, 128), (1, 72), (1, 16)], "gemm": []}
    calls["skinny"].clear()
    model.predict(inputs[:40].tolist())  # chunks of 16, 16 and 8 rows per layer
    assert calls["skinny"] == [(r, n) for n in (128, 72, 16) for r in (16, 16, 8)] and calls["gemm"] == []
    calls["skinny"].clear()
    model.predict(inputs[:64].tolist())  # 64 rows: one tiled GEMM per layer
    assert calls == {"skinny": [], "gemm": [(64, 128), (64, 72), (64, 16)]}
    # a layer the kernel does not take (2 bf16 columns = 4 B rows) runs PF.gemm for that layer only
    calls["gemm"].clear()
    narrow = NeuralNetworkModel("narrow", [64, 128, 2], activation_algos=["relu", "softmax"], bias_algo="random",
                                dtype="bfloat16", device="cuda:0")
    x = inputs[:20].tolist()
    got, err_new, err_old = _errors(narrow, x)
    assert calls["skinny"] == [(16, 128), (4, 128)]
    assert (16, 2) in calls["gemm"] and (4, 2) in calls["gemm"]
    assert err_new <= 2.0 * err_old + 1e-6


def test_predictor_never_serves_stale_weights(native_lib, models_tmpdir):
    torch.manual_seed(8)
    model = NeuralNetworkModel("stale", [8, 16, 4], activation_algos=["relu", "softmax"], dtype="bfloat16",
                               device="cuda:0")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(12, 8, generator=g).tolist()
    data = [(torch.randn(8, generator=g).tolist(), [i % 4]) for i in range(256)]
    before = model.predict(x)
    first = model._predictor
    assert isinstance(first, FusedPredictor)
    model.train(data, epochs=4, learning_rate=0.05, batch_size=64)  # the fused engine
    assert model.status == "Trained"
    after = model.predict(x)
    assert after != before and model._predictor is not first
    assert after == FusedPredictor(model).forward(torch.tensor(x)).tolist()  # bit for bit a fresh predictor's
    # the autograd training path
    second = model._predictor
    model._train_autograd(data, epochs=2, learning_rate=0.05, sample_size=64, decay_rate=1.0, dropout_rate=0.0,
                          l2_lambda=0.0)
    again = model.predict(x)
    assert again != after and model._predictor is not second
    assert again == FusedPredictor(model).forward(torch.tensor(x)).tolist()
    # new parameters through set_model_data (a re-placement)
    state = model.get_model_data()
    for layer_state in state["layers"]:
        layer_state["params"] = [torch.zeros_like(torch.tensor(p)).tolist() for p in layer_state.get("params", [])]
    model.set_model_data(state)
    uniform = model.predict(x)
    assert all(abs(v - 0.25) < 1e-6 for row in uniform for v in row)


def test_embedding_flatten_batchnorm_model_goes_through_the_predictor(native_lib):
    """The reference's character-model shape family (vocab 27, blocks of 3 ids). float32: behind an
    embedding the layer loop computes in fp32 whatever the policy, so only there do both paths
    have one precision and the error rule applies."""
    torch.manual_seed(9)
    model = NeuralNetworkModel("emb", [27, 10, 30, 64, 27],
                               activation_algos=["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"],
                               bias_algo="random", dtype="float32", device="cuda:0")
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 27, (100, 3), generator=g)
    # a training-mode forward first, so the running statistics are not the initial 0 / 1
    model.compute_output(ids.tolist(), [[int(i)] for i in torch.randint(0, 27, (100,), generator=g)])
    for rows in (1, 5, 40, 100):
        x = ids[0].tolist() if rows == 1 else ids[:rows].tolist()
        got, err_new, err_old = _errors(model, x)
        print(f"embedding model, rows {rows}: predict err {err_new:.3e}, compute_output err {err_old:.3e}")
        assert err_new <= 2.0 * err_old + 1e-6, (rows, err_new, err_old)
        assert (got.sum(-1) - 1.0).abs().max().item() <= 1e-5
    assert isinstance(model._predictor, FusedPredictor)
    with pytest.raises(IndexError):  # the same range check as PF.embedding
        model.predict([[0, 1, 27]])


def test_float64_gpu_model_falls_back_to_the_layer_loop(native_lib):
    torch.manual_seed(10)
    model = NeuralNetworkModel("f64", [6, 8, 3], activation_algos=["tanh", "sigmoid"], bias_algo="random",
                               dtype="float64", device="cuda:0")
    x = torch.randn(7, 6, generator=torch.Generator().manual_seed(5)).tolist()
    assert model.predict(x) == model.compute_output(x)[0]
    assert model.predict(x[0]) == model.compute_output(x[0])[0]
    assert model._predictor is False  # asked once, unsupported, not rebuilt per call
