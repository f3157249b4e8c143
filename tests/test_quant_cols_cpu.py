"""Weight-only e4m3 inference off the GPU: the pure-torch definition of the column quantiser
(``PF.quantize_cols_reference`` — the yardstick of the GPU kernel's tests) and the refusals of
``predict(..., weights=...)`` / ``POST /predict/`` for models that cannot take e4m3 weights.

Error bound of the quantiser, per element, with ``v = w / scale`` (exact, ``|v| <= 448``): e4m3 has
4 significant bits, so a normal ``v`` rounds within half an ulp, ``2^-4 |v|``; below ``2^-6`` the
grid is the subnormal step ``2^-9``, half of which is ``2^-10``. Hence
``|deq - w| <= 2^-4 |w| + 2^-10 scale[n]``."""
import pytest
import torch
from fastapi.testclient import TestClient

import main
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF

ZERO, EXACT, ABOVE, ONE, MIXED = 18, 19, 20, 21, 22  # the special columns of special_matrix()


def special_matrix() -> torch.Tensor:
    """[40, 24] fp32: random columns on different binades, an all-zero column, amax exactly at and
    one ulp above a scale's limit (448 * 2^-3), amax 1.0, and a column mixing 1.0 with values down
    to 2^-12 and a tiny negative."""
    g = torch.Generator().manual_seed(21)
    w = 0.5 * torch.randn(40, 24, generator=g)
    w = w * torch.ldexp(torch.ones(24), torch.arange(24, dtype=torch.int32) % 12 - 6)
    w[:, ZERO] = 0.0
    limit = torch.tensor(448.0 * 2.0 ** -3)
    for col, top in ((EXACT, limit), (ABOVE, torch.nextafter(limit, torch.tensor(1e9)))):
        w[:, col] = 40.0 * torch.rand(40, generator=g) - 20.0
        w[7, col] = -top
    w[:, ONE] = torch.rand(40, generator=g) - 0.5
    w[39, ONE] = 1.0
    w[:, MIXED] = torch.ldexp(torch.ones(40), -(torch.arange(40, dtype=torch.int32) % 13))
    w[5, MIXED] = -1e-30
    w[6, MIXED] = -(2.0 ** -12)
    return w


def test_reference_scales_are_the_smallest_powers_of_two_that_fit():
    w = special_matrix()
    w8, scale = PF.quantize_cols_reference(w)
    assert w8.dtype == torch.float8_e4m3fn and w8.shape == w.shape and scale.shape == (24,) and scale.dtype == torch.float32
    mant, _ = torch.frexp(scale)
    assert (mant == 0.5).all()                                  # every scale is a power of two
    amax = w.abs().amax(0)
    ratio = (amax / scale)[amax > 0]
    assert (ratio > 224).all() and (ratio <= 448).all()         # the smallest such power
    assert scale[ZERO] == 1.0 and (w8[:, ZERO].float() == 0).all()
    assert scale[EXACT] == 2.0 ** -3 and scale[ABOVE] == 2.0 ** -2 and scale[ONE] == 2.0 ** -8
    assert w8[7, EXACT].float() == -448.0


def test_reference_values_are_within_half_an_e4m3_step_and_exact_in_bf16():
    w = special_matrix()
    w8, scale = PF.quantize_cols_reference(w)
    deq = w8.float() * scale
    assert torch.isfinite(deq).all()
    bound = 2.0 ** -4 * w.abs() + 2.0 ** -10 * scale
    assert ((deq - w).abs() <= bound).all()
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)
    assert torch.equal(PF.dequantize_cols(w8, scale).float(), deq)
    assert w8[5, MIXED].float() == 0.0 and w8[39, ONE].float() * scale[ONE] == 1.0


def test_reference_refuses_non_finite_weights_and_takes_any_shape():
    for bad in (float("nan"), float("inf")):
        w = torch.ones(3, 5)
        w[1, 2] = bad
        with pytest.raises(ValueError, match="non-finite"):
            PF.quantize_cols_reference(w)
    for shape in [(1, 1), (1, 16), (77, 7), (3, 72)]:
        w = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[0]))
        w8, scale = PF.quantize_cols_reference(w)
        assert ((w8.float() * scale - w).abs() <= 2.0 ** -4 * w.abs() + 2.0 ** -10 * scale).all()
    tiny = torch.full((2, 2), 1e-42)                            # a subnormal amax: the scale stays normal
    w8, scale = PF.quantize_cols_reference(tiny)
    assert (scale == 2.0 ** -126).all() and torch.isfinite(w8.float()).all()


X = [[0.5, -1.0, 2.0, 0.25], [1.0, 0.0, -0.5, 3.0]]


@pytest.mark.parametrize("dtype", ["bfloat16", None], ids=["cpu_bf16", "cpu_float64"])
def test_predict_refuses_fp8_weights_where_no_kernel_can_serve_them(dtype):
    torch.manual_seed(3)
    model = NeuralNetworkModel("q", [4, 8, 2], activation_algos=["relu", "softmax"], dtype=dtype, device="cpu")
    expected = model.predict(X)
    with pytest.raises(ValueError, match="fp8"):
        model.predict(X, weights="fp8")
    with pytest.raises(ValueError, match="int4"):
        model.predict(X, weights="int4")
    assert model.predict(X) == expected and model.predict(X, weights=None) == expected


@pytest.fixture
def client(models_tmpdir):
    main._predict_cache.clear()
    with TestClient(main.app) as c:
        yield c
    main._predict_cache.clear()


def test_rest_predict_answers_400_for_weights_it_cannot_serve_and_is_unchanged_without_the_field(client):
    body = {"model_id": "m", "layer_sizes": [4, 8, 2], "activation_algos": ["relu", "softmax"], "optimizer": "stochastic"}
    assert client.post("/model/", json=body).status_code == 200
    for weights in ("fp8", "int4"):
        r = client.post("/predict/", json={"model_id": "m", "inputs": X, "weights": weights})
        assert r.status_code == 400, r.text
        assert "Value error occurred" in r.json()["detail"] and weights in r.json()["detail"]
    plain = client.post("/predict/", json={"model_id": "m", "inputs": X})
    assert plain.status_code == 200, plain.text
    out = client.post("/output/", json={"model_id": "m", "input": {"activation_vector": X}})
    assert plain.json()["output_vectors"] == out.json()["output_vector"]
    null = client.post("/predict/", json={"model_id": "m", "inputs": X, "weights": None})
    assert null.status_code == 200 and null.json() == plain.json()
    spec = client.get("/openapi.json").json()
    assert "fp8" in str(spec["components"]["schemas"]["PredictRequest"]["properties"]["weights"])
