"""``NeuralNetworkModel.predict`` off the GPU: the layer loop under ``no_grad`` — bit-identical to
``compute_output`` without a target — for the reference runtime (fp64) and fp32 / bf16 CPU models."""
import pytest
import torch

from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel


def _model(dtype, algos=("relu", "tanh", "softmax"), sizes=(6, 12, 9, 4)):
    torch.manual_seed(7)
    return NeuralNetworkModel("p", list(sizes), activation_algos=list(algos), bias_algo="random", dtype=dtype,
                              device="cpu")


@pytest.mark.parametrize("dtype", [None, "float32", "bfloat16"])
def test_predict_equals_compute_output_for_a_vector_and_a_batch(dtype):
    model = _model(dtype)
    g = torch.Generator().manual_seed(1)
    vector = torch.randn(6, generator=g).tolist()
    batch = torch.randn(5, 6, generator=g).tolist()
    for x in (vector, batch):
        expected, cost = model.compute_output(x)
        assert cost is None
        got = model.predict(x)
        assert got == expected  # exactly: the same ops in the same order
    assert len(model.predict(vector)) == 4 and len(model.predict(batch)) == 5


def test_predict_is_eval_mode_and_records_nothing_for_autograd():
    model = _model(None, algos=("linear", "batchnorm", "sigmoid", "sigmoid"), sizes=(6, 8, 3))
    for p in model.params:
        p.requires_grad_()
    x = torch.randn(4, 6, generator=torch.Generator().manual_seed(2)).tolist()
    bn = next(layer for layer in model.layers if layer.algo == "batchnorm")
    mean_before = bn.mean.clone()
    model.compute_output(x, [[0.0, 1.0, 0.0]] * 4)  # a training-mode forward: layers left in training mode
    assert any(layer.training for layer in model.layers)
    mean_trained = bn.mean.clone()
    assert not torch.equal(mean_before.reshape(-1), mean_trained.reshape(-1))
    out = model.predict(x)
    assert all(not layer.training for layer in model.layers)
    assert torch.equal(bn.mean, mean_trained)  # eval mode: running statistics untouched
    assert out == model.compute_output(x)[0]
    assert all(p.grad is None for p in model.params)


def test_predict_after_training_and_reload_follows_the_weights(models_tmpdir):
    model = _model("float32", algos=("tanh", "softmax"), sizes=(3, 5, 2))
    x = [[0.5, -1.0, 2.0], [1.0, 0.0, -0.5]]
    before = model.predict(x)
    data = [([float(i % 2), float(i % 3), 1.0], [i % 2]) for i in range(40)]
    model.train(data, epochs=5, learning_rate=0.1, batch_size=8)
    after = model.predict(x)
    assert after != before and after == model.compute_output(x)[0]
    again = NeuralNetworkModel.deserialize("p")
    assert again.predict(x) == again.compute_output(x)[0]


def test_cpu_models_have_no_fused_predictor_and_a_built_one_is_reused(monkeypatch):
    from penr_oz_neural_network_torch_amd.engine import predictor as predictor_mod

    model = _model("float32")
    assert model._fused_predictor() is None and model._predictor is False  # unsupported: asked once
    built = []

    class Stub:
        def __init__(self, m):
            built.append(m)

    monkeypatch.setattr(predictor_mod, "FusedPredictor", Stub)
    model._place()  # a re-placement drops whatever was cached
    assert model._predictor is None
    first = model._fused_predictor()
    assert isinstance(first, Stub) and model._fused_predictor() is first and built == [model]
