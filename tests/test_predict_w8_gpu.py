"""``predict(..., weights="fp8")`` on the GPU: weight-only quantised inference through
``engine/predictor.py`` (e4m3 weight copies with one power-of-two scale per output column,
``PF.gemm_skinny_w8`` below 64 rows, the bf16 kernels on dequantised copies elsewhere).

Accuracy rule, mirroring ``test_predict_gpu.py``: model A predicts from e4m3 weights; its twin B is
the same model with its fp32 masters SET to A's dequantised weights, predicting through the
default path (code that knows nothing of fp8). Dequantised weights are exact in bf16, so both
compute the same function of the same weight values in the same precisions; against the fp64
forward of B's masters

    err(A.predict(x, weights="fp8")) <= 2 * err(B.predict(x)) + 1e-6

(a factor of 2 covers rounding flips on a small sample, as there).

Measured on an MI355X (max abs error of A with fp8 weights / of B through the default path; the
two agree to the printed digits, the bf16 roundings of the activations hide the different
summation orders), [64,128,80,16] relu, tanh + softmax head: rows 1: 2.8e-4 / 2.8e-4, 5: 2.8e-4,
16: 4.9e-4, 40: 6.8e-4, 64: 6.8e-4, 200: 8.2e-4; + sigmoid head: 1: 8.5e-4, 5-40: 9.8e-4, 64: 1.1e-3,
200: 1.3e-3; [64,128,72,16] at 20 rows: 5.2e-4; embedding + batchnorm model: rows 1: 2.4e-4, 40: 5.2e-4.
"""
import pytest
import torch
from fastapi.testclient import TestClient

import main
from penr_oz_neural_network_torch_amd.engine.predictor import FusedPredictor
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
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


def _twin(model, make):
    """``make()`` builds a model of the same structure; its masters become ``model``'s dequantised
    linear weights (everything else copied as it is), through ``set_model_data``."""
    twin = make()
    state = model.get_model_data()
    for layer, layer_state in zip(model.layers, state["layers"]):
        if layer.algo == "linear":
            w8, scale = PF.quantize_cols(layer.weights.detach().to(DEV, torch.float32).contiguous())
            layer_state["params"][0] = (w8.float() * scale).cpu().tolist()
    twin.set_model_data(state)
    for src, dst in zip(model.layers, twin.layers):
        if src.algo == "batchnorm":  # the running statistics are no parameters: carried over by hand
            dst.mean, dst.variance = src.mean.detach().clone(), src.variance.detach().clone()
    return twin


def _check_rule(model, twin, x, what):
    ref = _reference(twin, x)
    got = torch.tensor(model.predict(x, weights="fp8"), dtype=torch.float64)
    base = torch.tensor(twin.predict(x), dtype=torch.float64)
    assert got.shape == ref.shape == base.shape
    err_new, err_old = (got - ref).abs().max().item(), (base - ref).abs().max().item()
    print(f"{what}: fp8 err {err_new:.3e}, twin default err {err_old:.3e}")
    assert err_new <= 2.0 * err_old + 1e-6, (what, err_new, err_old)
    return got


@pytest.fixture(scope="module")
def inputs():
    return torch.randn(200, 64, generator=torch.Generator().manual_seed(11))


def _mlp(name, sizes, head="softmax"):
    return NeuralNetworkModel(name, sizes, activation_algos=["relu", "tanh", head], bias_algo="random",
                              dtype="bfloat16", device=DEV)


@pytest.mark.parametrize("head", ["softmax", "sigmoid"])
def test_fp8_weights_are_as_accurate_as_the_default_path_on_the_same_weight_values(native_lib, inputs, head):
    torch.manual_seed(5)
    model = _mlp("acc8", [64, 128, 80, 16], head)
    twin = _twin(model, lambda: _mlp("acc8twin", [64, 128, 80, 16], head))
    for rows in ROWS:
        x = inputs[0].tolist() if rows == 1 else inputs[:rows].tolist()
        got = _check_rule(model, twin, x, f"{head} head, rows {rows}")
        if head == "softmax":
            assert (got.sum(-1) - 1.0).abs().max().item() <= 1e-5
    assert isinstance(model._predictor, FusedPredictor)


def test_dispatch_below_64_rows_is_the_e4m3_kernel(native_lib, inputs, monkeypatch):
    """A silent fall-back to unquantised weights or to another GEMM must fail here: the calls are counted."""
    calls = {"w8": [], "skinny": [], "gemm": []}
    real_w8, real_skinny, real_gemm = PF.gemm_skinny_w8, PF.gemm_skinny, PF.gemm

    def spy_w8(x, w8, scale, out, **kw):
        assert w8.dtype == torch.float8_e4m3fn
        calls["w8"].append((x.shape[0], w8.shape[1]))
        return real_w8(x, w8, scale, out, **kw)

    def spy_skinny(x, w, out, **kw):
        calls["skinny"].append((x.shape[0], w.shape[1]))
        return real_skinny(x, w, out, **kw)

    def spy_gemm(a, a_kc, b, b_kc, out, **kw):
        calls["gemm"].append((out.shape[0], out.shape[1]))
        return real_gemm(a, a_kc, b, b_kc, out, **kw)

    def clear():
        for v in calls.values():
            v.clear()

    monkeypatch.setattr(PF, "gemm_skinny_w8", spy_w8)
    monkeypatch.setattr(PF, "gemm_skinny", spy_skinny)
    monkeypatch.setattr(PF, "gemm", spy_gemm)
    torch.manual_seed(6)
    model = _mlp("spy8", [64, 128, 80, 16])
    model.predict(inputs[0].tolist(), weights="fp8")
    assert calls == {"w8": [(1, 128), (1, 80), (1, 16)], "skinny": [], "gemm": []}
    clear()
    model.predict(inputs[:40].tolist(), weights="fp8")  # chunks of 16, 16 and 8 rows per layer
    assert calls == {"w8": [(r, n) for n in (128, 80, 16) for r in (16, 16, 8)], "skinny": [], "gemm": []}
    clear()
    model.predict(inputs[:64].tolist(), weights="fp8")  # 64 rows: one tiled GEMM per layer, dequantised copies
    assert calls == {"w8": [], "skinny": [], "gemm": [(64, 128), (64, 80), (64, 16)]}
    clear()
    # a layer the e4m3 kernel does not take (72 columns: no multiple of 16) runs the bf16 skinny
    # kernel on its dequantised copy, that layer only
    narrow = _mlp("narrow8", [64, 128, 72, 16])
    twin = _twin(narrow, lambda: _mlp("narrow8twin", [64, 128, 72, 16]))
    clear()
    narrow.predict(inputs[:20].tolist(), weights="fp8")
    assert calls == {"w8": [(16, 128), (4, 128), (16, 16), (4, 16)], "skinny": [(16, 72), (4, 72)], "gemm": []}
    deq = narrow._predictor.weights_deq
    assert [(t.dtype, tuple(t.shape)) for t in deq.values()] == [(torch.bfloat16, (128, 72))]
    clear()
    narrow.predict(inputs[:64].tolist(), weights="fp8")
    assert calls == {"w8": [], "skinny": [], "gemm": [(64, 128), (64, 72), (64, 16)]}
    _check_rule(narrow, twin, inputs[:20].tolist(), "72-wide layer, rows 20")


def _holds_e4m3(obj) -> bool:
    if isinstance(obj, torch.Tensor):
        return obj.dtype == torch.float8_e4m3fn
    if isinstance(obj, dict):
        return any(_holds_e4m3(v) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return any(_holds_e4m3(v) for v in obj)
    return False


def test_default_path_is_untouched_by_fp8_requests(native_lib, inputs):
    torch.manual_seed(7)
    model = _mlp("dflt8", [64, 128, 80, 16])
    small, large = inputs[:5].tolist(), inputs[:64].tolist()
    before = (model.predict(small), model.predict(large))
    predictor = model._predictor
    assert isinstance(predictor, FusedPredictor)
    # never asked for fp8: no e4m3 tensor, no dequantised copy
    assert predictor.weights8 == {} and predictor.weights_deq == {}
    assert not any(_holds_e4m3(v) for v in vars(predictor).values())
    fp8 = (model.predict(small, weights="fp8"), model.predict(large, weights="fp8"))
    assert model._predictor is predictor and _holds_e4m3(predictor.weights8)
    assert (model.predict(small), model.predict(large)) == before  # bit for bit
    assert fp8[0] != before[0]                                     # and the option did something
    assert fp8[1][:5] != before[1][:5]


def test_refusals_on_gpu_models_raise_value_error(native_lib):
    x = [[0.5] * 16] * 3
    for dtype in ("float32", "float64"):
        torch.manual_seed(1)
        model = NeuralNetworkModel("exact", [16, 16, 4], activation_algos=["relu", "softmax"], dtype=dtype, device=DEV)
        expected = model.predict(x)
        with pytest.raises(ValueError, match="fp8"):
            model.predict(x, weights="fp8")
        with pytest.raises(ValueError, match="int4"):
            model.predict(x, weights="int4")
        assert model.predict(x) == expected


def test_fp8_predictions_follow_new_weights(native_lib, models_tmpdir):
    def make(name="stale8"):
        return NeuralNetworkModel(name, [16, 32, 16], activation_algos=["relu", "softmax"], bias_algo="random",
                                  dtype="bfloat16", device=DEV)

    torch.manual_seed(8)
    model = make()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(12, 16, generator=g).tolist()
    # (train() waits for as many samples as the model has parameters: 1072)
    data = [(row, [i % 16]) for i, row in enumerate(torch.randn(1100, 16, generator=g).tolist())]
    before = model.predict(x, weights="fp8")
    first = model._predictor
    assert _holds_e4m3(first.weights8)
    model.train(data, epochs=1, learning_rate=0.05, batch_size=64)  # the fused engine
    assert model.status == "Trained"
    after = model.predict(x, weights="fp8")
    assert after != before and model._predictor is not first
    assert after == FusedPredictor(model).forward(torch.tensor(x), weights="fp8").tolist()
    _check_rule(model, _twin(model, lambda: make("stale8twin")), x, "after train")
    # new parameters through set_model_data (a re-placement)
    second = model._predictor
    state = model.get_model_data()
    gen = torch.Generator().manual_seed(4)
    for layer_state in state["layers"]:
        layer_state["params"] = [torch.randn(torch.tensor(p).shape, generator=gen).tolist()
                                 for p in layer_state.get("params", [])]
    model.set_model_data(state)
    replaced = model.predict(x, weights="fp8")
    assert replaced != after and model._predictor is not second
    _check_rule(model, _twin(model, lambda: make("stale8twin2")), x, "after set_model_data")


def test_embedding_flatten_batchnorm_model_takes_fp8_weights(native_lib):
    def make(name):
        return NeuralNetworkModel(name, [27, 10, 30, 64, 32],
                                  activation_algos=["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"],
                                  bias_algo="random", dtype="bfloat16", device=DEV)

    torch.manual_seed(9)
    model = make("emb8")
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 27, (100, 3), generator=g)
    # a training-mode forward first, so the running statistics are not the initial 0 / 1
    model.compute_output(ids.tolist(), [[int(i)] for i in torch.randint(0, 27, (100,), generator=g)])
    twin = _twin(model, lambda: make("emb8twin"))
    for rows in (1, 40):
        x = ids[0].tolist() if rows == 1 else ids[:rows].tolist()
        got = _check_rule(model, twin, x, f"embedding model, rows {rows}")
        assert (got.sum(-1) - 1.0).abs().max().item() <= 1e-5
    assert isinstance(model._predictor, FusedPredictor) and len(model._predictor.weights8) == 2


def test_rest_predict_with_fp8_weights_returns_what_the_model_returns(native_lib, models_tmpdir):
    main._predict_cache.clear()
    x = torch.randn(5, 16, generator=torch.Generator().manual_seed(2)).tolist()
    with TestClient(main.app) as client:
        body = {"model_id": "rest8", "layer_sizes": [16, 32, 16], "activation_algos": ["relu", "softmax"],
                "dtype": "bfloat16", "device": DEV}
        assert client.post("/model/", json=body).status_code == 200
        r = client.post("/predict/", json={"model_id": "rest8", "inputs": x, "weights": "fp8"})
        assert r.status_code == 200, r.text
        plain = client.post("/predict/", json={"model_id": "rest8", "inputs": x})
        assert plain.status_code == 200, plain.text
    main._predict_cache.clear()
    model = NeuralNetworkModel.deserialize("rest8")
    assert r.json()["output_vectors"] == model.predict(x, weights="fp8")
    assert plain.json()["output_vectors"] == model.predict(x)
    assert r.json() != plain.json()
