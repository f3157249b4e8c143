"""Token generation without a GPU: the host mirror of the sampling kernel's random numbers, the
pure-torch sampling rule (``PF.sample_rows_reference``), ``NeuralNetworkModel.generate`` through the
layer loop, and ``POST /generate/``."""
import math

import pytest
import torch
from fastapi.testclient import TestClient

import main
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF

SEED = (11, 22)
CHAR_SIZES = [27, 10, 30, 64, 27]
CHAR_ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]


def _logits(rows, cols, seed=0):
    return 2.0 * torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))


# --------------------------------------------------------------------------------------------
# PF.sample_uniform
# --------------------------------------------------------------------------------------------
def test_sample_uniform_range_pin_and_mean():
    assert PF.sample_uniform(SEED, 0, 0) == 14444861 * 2.0 ** -24 == 0.8609808087348938
    values = [PF.sample_uniform(SEED, row, step) for row in range(256) for step in range(256)]
    assert all(0.0 <= v < 1.0 for v in values)
    assert abs(sum(values) / len(values) - 0.5) < 0.01
    assert len(set(values[:256])) > 250  # steps of one row draw different numbers
    # the vectorised form the reference sampler uses is the same integers
    batch = PF._sample_uniforms(SEED, 256, 7, 3, "cpu")
    assert batch.tolist() == [PF.sample_uniform(SEED, 3 + r, 7) for r in range(256)]


# --------------------------------------------------------------------------------------------
# PF.sample_rows_reference
# --------------------------------------------------------------------------------------------
def test_reference_greedy_is_the_lowest_argmax():
    lg = _logits(33, 101)
    lg[5, 17] = lg[5, 60] = lg[5].max() + 1.0  # a tie: the lowest index wins
    got = PF.sample_rows_reference(lg, SEED, 0, temperature=0.0)
    assert got.dtype == torch.int64 and got.tolist() == lg.argmax(-1).tolist() and got[5] == 17
    assert PF.sample_rows_reference(lg[3], SEED, 0, temperature=0.0).tolist() == [int(lg[3].argmax())]


def test_reference_token_is_searchsorted_on_the_fp64_cdf():
    lg = _logits(64, 1000, seed=1)
    for step, temperature in [(0, 1.0), (3, 0.7)]:
        got = PF.sample_rows_reference(lg, SEED, step, temperature=temperature)
        t32 = float(torch.tensor(temperature, dtype=torch.float32))
        for r in range(64):
            w = torch.exp((lg[r].double() - lg[r].double().max()) / t32)
            cdf = w.cumsum(0)
            want = int(torch.searchsorted(cdf, torch.tensor(PF.sample_uniform(SEED, r, step) * cdf[-1].item(),
                                                            dtype=torch.float64), right=True))
            assert got[r] == min(want, 999), (step, r)
    # row0 shifts the row index of the draw
    shifted = PF.sample_rows_reference(lg[10:11], SEED, 0, row0=10)
    assert shifted[0] == PF.sample_rows_reference(lg, SEED, 0)[10]


def test_reference_top_k_keeps_ties_and_nothing_below():
    row = torch.tensor([0.0, 3.0, 1.0, 2.0, 2.0, -1.0, 0.5])  # k = 2: the 2nd and 3rd largest tie at 2.0
    lg = row.repeat(4096, 1)
    got = PF.sample_rows_reference(lg, SEED, 0, temperature=50.0, top_k=2)
    assert set(got.tolist()) == {1, 3, 4}
    assert set(PF.sample_rows_reference(lg, SEED, 1, temperature=50.0, top_k=1).tolist()) == {1}
    assert set(PF.sample_rows_reference(lg, SEED, 2, temperature=50.0, top_k=7).tolist()) == set(range(7))
    assert set(PF.sample_rows_reference(lg, SEED, 2, temperature=50.0, top_k=99).tolist()) == set(range(7))


def test_reference_follows_the_distribution():
    n = 16384
    one = _logits(1, 27, seed=2)
    p = one[0].double().softmax(0)
    counts = torch.bincount(PF.sample_rows_reference(one.repeat(n, 1), SEED, 0), minlength=27).double()
    assert counts.sum() == n
    for c in range(27):
        if p[c] >= 1e-3:
            assert abs(counts[c] - n * p[c]) <= 5.0 * math.sqrt(n * p[c] * (1 - p[c])), (c, counts[c], n * p[c])


def test_reference_rejects_bad_arguments():
    with pytest.raises(ValueError):
        PF.sample_rows_reference(_logits(2, 5), SEED, 0, temperature=-1.0)
    with pytest.raises(ValueError):
        PF.sample_rows_reference(_logits(2, 5), SEED, 0, temperature=float("nan"))


# --------------------------------------------------------------------------------------------
# NeuralNetworkModel.generate through the layer loop
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def char_model():
    torch.manual_seed(3)
    model = NeuralNetworkModel("chars", CHAR_SIZES, activation_algos=CHAR_ALGOS, bias_algo="random")
    ids = torch.randint(0, 27, (64, 3), generator=torch.Generator().manual_seed(4))
    model.compute_output(ids.tolist(), [[int(i)] for i in ids[:, 0]])  # batchnorm statistics off their initial values
    return model


def test_cpu_generate_shapes_padding_and_truncation(char_model):
    assert char_model.context_length == 3
    out = char_model.generate([[1], [1, 2, 3], [9, 9, 4, 5, 6]], 12, seed=5)
    assert out["seed"] == 5 and [len(r) for r in out["tokens"]] == [12, 12, 12]
    assert all(0 <= t < 27 for r in out["tokens"] for t in r)
    # padding and truncation: each row alone, spelled out, gives the same tokens only in row 0 (the
    # draw depends on the row index), so compare through a batch in the same positions
    spelled = char_model.generate([[0, 0, 1], [1, 2, 3], [4, 5, 6]], 12, seed=5)
    assert spelled["tokens"] == out["tokens"]
    other_pad = char_model.generate([[1], [1, 2, 3], [9, 9, 4, 5, 6]], 12, seed=5, pad_token=7)
    assert other_pad["tokens"][1:] == out["tokens"][1:]
    assert other_pad["tokens"][0] == char_model.generate([[7, 7, 1]], 12, seed=5)["tokens"][0]
    single = char_model.generate([1, 2, 3], 4, seed=5)  # one id list: one row
    assert len(single["tokens"]) == 1 and len(single["tokens"][0]) == 4
    # every token follows the rule: teacher-forced check of the window bookkeeping
    key = (5, 0)
    for r, (ctx, row) in enumerate(zip([[0, 0, 1], [1, 2, 3], [4, 5, 6]], out["tokens"])):
        seq = ctx + row
        for s, token in enumerate(row):
            probs = torch.tensor(char_model.predict([seq[s:s + 3]])[0], dtype=torch.float64)
            want = PF.sample_rows_reference(probs.log().unsqueeze(0), key, s, row0=r)
            assert token == int(want), (r, s)


def test_cpu_generate_is_reproducible_and_seed_sensitive(char_model):
    ctx = [[1], [1, 2, 3], [4, 5, 6, 7]]
    a = char_model.generate(ctx, 20, seed=2 ** 40 + 17)
    assert a == char_model.generate(ctx, 20, seed=2 ** 40 + 17)
    assert a["tokens"] != char_model.generate(ctx, 20, seed=2 ** 40 + 18)["tokens"]
    drawn = char_model.generate(ctx, 20)  # a seed from os.urandom, returned
    assert 0 <= drawn["seed"] < 2 ** 64
    assert char_model.generate(ctx, 20, seed=drawn["seed"]) == drawn
    greedy = char_model.generate(ctx, 6, temperature=0, seed=1)
    assert greedy["tokens"] == char_model.generate(ctx, 6, temperature=0, seed=2)["tokens"]
    top1 = char_model.generate(ctx, 6, top_k=1, seed=3)
    assert top1["tokens"] == greedy["tokens"]


def test_cpu_generate_cuts_rows_after_the_stop_token(char_model):
    ctx = [[1], [1, 2, 3], [4, 5, 6]]
    free = char_model.generate(ctx, 40, seed=9)["tokens"]
    stop = free[0][3]
    cut = char_model.generate(ctx, 40, seed=9, stop_token=stop)["tokens"]
    assert len(cut[0]) <= 4 and cut[0][-1] == stop
    for before, after in zip(free, cut):
        if stop in before:
            assert after == before[:before.index(stop) + 1]
        else:
            assert after == before
    assert any(len(r) < 40 for r in cut)


@pytest.mark.parametrize("kwargs", [
    {"max_new_tokens": 0}, {"max_new_tokens": 4097}, {"temperature": -0.5}, {"top_k": 0}, {"stop_token": 27},
    {"stop_token": -1}, {"pad_token": 27}, {"context": []}, {"weights": "fp8"}, {"weights": "int4"}, {"seed": -1},
])
def test_cpu_generate_argument_errors(char_model, kwargs):
    args = {"context": [[1, 2, 3]], "max_new_tokens": 4, **kwargs}
    with pytest.raises(ValueError):
        char_model.generate(**args)


def test_cpu_generate_refuses_models_that_are_no_next_token_models(char_model):
    dense = NeuralNetworkModel("dense", [9, 18, 9], activation_algos=["relu", "sigmoid"])
    with pytest.raises(ValueError, match="embedding"):
        dense.generate([[1, 2, 3]], 4)
    headless = NeuralNetworkModel("headless", [27, 10, 30, 27], activation_algos=["embedding", "linear", "tanh"])
    with pytest.raises(ValueError, match="softmax"):
        headless.generate([[1, 2, 3]], 4)
    with pytest.raises(IndexError):
        char_model.generate([[1, 2, 27]], 4)


# --------------------------------------------------------------------------------------------
# POST /generate/
# --------------------------------------------------------------------------------------------
@pytest.fixture
def client(models_tmpdir):
    main._predict_cache.clear()
    with TestClient(main.app) as c:
        yield c
    main._predict_cache.clear()


def _create_chars(client, model_id="chars"):
    body = {"model_id": model_id, "layer_sizes": CHAR_SIZES, "activation_algos": CHAR_ALGOS}
    assert client.post("/model/", json=body).status_code == 200


def test_rest_generate_answers_tokens_and_a_seed_that_reproduces_them(client):
    _create_chars(client)
    r = client.post("/generate/", json={"model_id": "chars", "context": [[1], [1, 2, 3, 4]], "max_new_tokens": 9})
    assert r.status_code == 200, r.text
    first = r.json()
    assert set(first) == {"tokens", "seed"} and [len(t) for t in first["tokens"]] == [9, 9]
    again = client.post("/generate/", json={"model_id": "chars", "context": [[1], [1, 2, 3, 4]], "max_new_tokens": 9,
                                            "seed": first["seed"]})
    assert again.status_code == 200 and again.json() == first
    opts = client.post("/generate/", json={"model_id": "chars", "context": [1, 2], "max_new_tokens": 5, "temperature": 0.5,
                                           "top_k": 3, "seed": 7, "stop_token": 0, "pad_token": 2})
    assert opts.status_code == 200 and opts.json()["seed"] == 7 and len(opts.json()["tokens"]) == 1


def test_rest_generate_error_mapping(client):
    _create_chars(client)
    assert client.post("/model/", json={"model_id": "dense", "layer_sizes": [9, 18, 9],
                                        "activation_algos": ["relu", "sigmoid"]}).status_code == 200
    ok = {"model_id": "chars", "context": [[1, 2, 3]], "max_new_tokens": 4}
    for body in ({**ok, "model_id": "dense"}, {**ok, "context": [[1, 2, 27]]}, {**ok, "max_new_tokens": 0},
                 {**ok, "weights": "fp8"}):
        r = client.post("/generate/", json=body)
        assert r.status_code == 400, (body, r.text)
        assert "Value error occurred" in r.json()["detail"]
    assert client.post("/generate/", json={**ok, "model_id": "never"}).status_code == 404
    assert client.post("/generate/", json={"model_id": "chars"}).status_code == 422
    spec = client.get("/openapi.json").json()
    examples = spec["paths"]["/generate/"]["post"]["requestBody"]["content"]["application/json"]["examples"]
    assert set(examples) == {"single", "batch"}


def test_rest_generate_shares_the_predict_cache(client, monkeypatch):
    real = NeuralNetworkModel.deserialize.__func__
    loads = []

    def counted(cls, model_id, meta_only=False):
        if not meta_only:
            loads.append(model_id)
        return real(cls, model_id, meta_only=meta_only)

    monkeypatch.setattr(NeuralNetworkModel, "deserialize", classmethod(counted))
    _create_chars(client)
    assert client.post("/predict/", json={"model_id": "chars", "inputs": [[1, 2, 3]]}).status_code == 200
    assert client.post("/generate/", json={"model_id": "chars", "context": [[1, 2, 3]], "max_new_tokens": 3}).status_code == 200
    assert loads == ["chars"]
