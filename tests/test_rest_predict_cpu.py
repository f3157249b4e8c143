"""``POST /predict/``: outputs only, models kept loaded in a small LRU that follows the checkpoint
file (reloaded after a training rewrote it, evicted by ``DELETE /model/``)."""
import time

import pytest
from fastapi.testclient import TestClient

import main
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel

BATCH = [[1.0, 0.5, 0.0, -1.0], [0.0, 2.0, 1.0, 0.25], [-1.0, -0.5, 3.0, 0.0]]


@pytest.fixture
def client(models_tmpdir):
    main._predict_cache.clear()
    with TestClient(main.app) as c:
        yield c
    main._predict_cache.clear()


@pytest.fixture
def count_loads(monkeypatch):
    real = NeuralNetworkModel.deserialize.__func__
    calls = []

    def counted(cls, model_id, meta_only=False):
        if not meta_only:
            calls.append(model_id)
        return real(cls, model_id, meta_only=meta_only)

    monkeypatch.setattr(NeuralNetworkModel, "deserialize", classmethod(counted))
    return calls


def _create(client, model_id="m", **extra):
    body = {"model_id": model_id, "layer_sizes": [4, 8, 2], "activation_algos": ["relu", "softmax"],
            "optimizer": "stochastic", **extra}
    assert client.post("/model/", json=body).status_code == 200


def _output(client, model_id, x):
    r = client.post("/output/", json={"model_id": model_id, "input": {"activation_vector": x}})
    assert r.status_code == 200, r.text
    return r.json()["output_vector"]


def _predict(client, model_id, x):
    r = client.post("/predict/", json={"model_id": model_id, "inputs": x})
    assert r.status_code == 200, r.text
    return r.json()["output_vectors"]


def _wait_trained(client, model_id, timeout=60.0):
    t0 = time.time()
    while time.time() - t0 < timeout:
        r = client.get("/progress/", params={"model_id": model_id})
        assert r.status_code == 200, r.text
        if r.json()["status"] == "Trained":
            return
        time.sleep(0.02)
    raise AssertionError("training did not finish")


def test_predict_returns_what_output_returns(client):
    _create(client)
    assert _predict(client, "m", BATCH) == _output(client, "m", BATCH)
    assert _predict(client, "m", BATCH[0]) == _output(client, "m", BATCH[0])  # one vector: one output vector


def test_second_request_reuses_the_loaded_model(client, count_loads):
    _create(client)
    first = _predict(client, "m", BATCH)
    assert count_loads == ["m"]
    assert _predict(client, "m", BATCH) == first
    assert _predict(client, "m", BATCH[1]) == first[1]
    assert count_loads == ["m"]  # served from the cache: the checkpoint was parsed once


def test_cache_holds_four_models_and_evicts_the_least_recently_used(client, count_loads):
    for i in range(5):
        _create(client, f"m{i}")
    for i in range(4):
        _predict(client, f"m{i}", BATCH)
    _predict(client, "m0", BATCH)          # m0 is now the most recently used
    _predict(client, "m4", BATCH)          # a fifth model: m1 (least recently used) leaves
    assert list(main._predict_cache) == ["m2", "m3", "m0", "m4"]
    del count_loads[:]
    _predict(client, "m0", BATCH)
    assert count_loads == []
    _predict(client, "m1", BATCH)
    assert count_loads == ["m1"]


def test_checkpoint_rewritten_by_training_is_reloaded(client, count_loads):
    _create(client)
    before = _predict(client, "m", BATCH)
    data = [{"activation_vector": [i % 3, 1, 0, -1], "target_vector": [i % 2]} for i in range(64)]
    r = client.put("/train/", json={"model_id": "m", "training_data": data, "epochs": 10, "batch_size": 16,
                                    "learning_rate": 0.1, "decay_rate": 1.0})
    assert r.status_code == 202
    _wait_trained(client, "m")
    del count_loads[:]
    after = _predict(client, "m", BATCH)
    assert "m" in count_loads  # the entry no longer matched the file: loaded again
    assert after != before
    assert after == _output(client, "m", BATCH)


def test_deleted_model_is_evicted_and_answers_404(client):
    _create(client)
    _predict(client, "m", BATCH)
    assert "m" in main._predict_cache
    assert client.delete("/model/", params={"model_id": "m"}).status_code == 204
    assert "m" not in main._predict_cache
    r = client.post("/predict/", json={"model_id": "m", "inputs": BATCH})
    assert r.status_code == 404 and "not created yet" in r.json()["detail"]
    assert client.post("/predict/", json={"model_id": "never", "inputs": BATCH}).status_code == 404


@pytest.mark.parametrize("bad", [
    [[1.0, 2.0, 3.0, 4.0], [1.0, 2.0]],      # ragged
    [1.0, 2.0, 3.0],                          # wrong width
    [[1.0, 2.0, 3.0, 4.0, 5.0]],              # wrong width, 2-D
    [[[1.0, 2.0, 3.0, 4.0]]],                 # 3-D
    [],                                       # empty
    [[1.0, 2.0, 3.0, 4.0], 5.0],              # a scalar among the rows
])
def test_malformed_inputs_answer_400(client, bad):
    _create(client)
    r = client.post("/predict/", json={"model_id": "m", "inputs": bad})
    assert r.status_code == 400, r.text
    assert "Value error occurred" in r.json()["detail"]


def test_embedding_id_outside_the_vocabulary_answers_400(client):
    body = {"model_id": "e", "layer_sizes": [5, 4, 8, 6, 3], "activation_algos": ["embedding", "tanh", "softmax"]}
    assert client.post("/model/", json=body).status_code == 200
    assert client.post("/predict/", json={"model_id": "e", "inputs": [[0, 4], [1, 2]]}).status_code == 200
    r = client.post("/predict/", json={"model_id": "e", "inputs": [[0, 5]]})
    assert r.status_code == 400, r.text


def test_missing_fields_answer_422_and_the_route_is_documented(client):
    assert client.post("/predict/", json={"model_id": "m"}).status_code == 422
    spec = client.get("/openapi.json").json()
    examples = spec["paths"]["/predict/"]["post"]["requestBody"]["content"]["application/json"]["examples"]
    assert set(examples) == {"single", "batch"}
