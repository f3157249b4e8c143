"""Top-k answers without a GPU: the rule of ``PF.topk_rows_reference`` against ``PF.token_logprob_reference``,
``NeuralNetworkModel.classify`` against ``predict``, ``score(top_logprobs=k)`` and ``generate(top_logprobs=k)``
through the layer loop, ``POST /classify/`` and the ``top_logprobs`` option of ``/score/`` and ``/generate/``."""
import math

import pytest
import torch
from fastapi.testclient import TestClient

import main
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import score_cases as C

CHAR_SIZES = [27, 10, 30, 64, 27]
CHAR_ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]


# --------------------------------------------------------------------------------------------
# the rule
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 2, 27, 64, 65, 257, 1025])
@pytest.mark.parametrize("kind", C.KINDS)
def test_reference_column_j_has_rank_j(kind, cols):
    rows = 5
    x = C.make_logits(kind, rows, cols, 31 * cols + 7)
    for k in sorted({1, min(cols, 2), min(cols, 5), min(cols, 64)}):
        idx, logprob = PF.topk_rows_reference(x, k)
        assert idx.dtype == torch.int64 and logprob.dtype == torch.float64 and idx.shape == logprob.shape == (rows, k)
        for j in range(k):
            lp, rank = PF.token_logprob_reference(x, idx[:, j])
            assert rank.tolist() == [j] * rows, (kind, cols, k, j)
            both_inf = torch.isinf(lp) & (lp == logprob[:, j])
            assert bool((both_inf | ((lp - logprob[:, j]).abs() <= 1e-12)).all()), (kind, cols, k, j)
        if kind == "flat":
            assert torch.equal(idx, torch.arange(k).repeat(rows, 1))
            assert logprob.reshape(-1).tolist() == pytest.approx([-math.log(cols)] * (k * rows), rel=1e-14, abs=1e-15)


def test_reference_ties_zeros_infinities_and_dtypes():
    row = torch.tensor([0.5, 2.0, -0.0, 2.0, 0.0, 2.0, -math.inf])
    idx, logprob = PF.topk_rows_reference(row, 7)  # a vector is one row
    assert idx.tolist() == [[1, 3, 5, 0, 2, 4, 6]]  # ties by column; -0.0 before the +0.0 to its right
    assert logprob[0, 6] == -math.inf and float(logprob[0, :6].exp().sum()) == pytest.approx(1.0, rel=1e-14)
    swapped = torch.tensor([[0.0, -0.0, 1.0, -0.0, 0.0]])
    assert PF.topk_rows_reference(swapped, 5)[0].tolist() == [[2, 0, 1, 3, 4]]
    assert PF.topk_rows_reference(swapped.double(), 3)[0].tolist() == [[2, 0, 1]]
    # compared in the logits' own dtype: two bf16-equal logits tie, the lower column first
    lg = torch.tensor([[1.0, 1.0 + 2 ** -10, 0.0]])
    assert PF.topk_rows_reference(lg.bfloat16(), 2)[0].tolist() == [[0, 1]]
    assert PF.topk_rows_reference(lg, 2)[0].tolist() == [[1, 0]]
    few = torch.tensor([[-math.inf, 1.0, -math.inf, -math.inf]])
    idx, logprob = PF.topk_rows_reference(few, 3)
    assert idx.tolist() == [[1, 0, 2]] and logprob.tolist() == [[0.0, -math.inf, -math.inf]]
    batch = torch.randn(2, 3, 9, generator=torch.Generator().manual_seed(1))  # leading dimensions are rows
    assert PF.topk_rows_reference(batch, 4)[0].shape == (6, 4)


def test_reference_refuses_k_out_of_range():
    x = torch.zeros(3, 9)
    for k in (0, 10, -1, True, 2.0, None):
        with pytest.raises(ValueError):
            PF.topk_rows_reference(x, k)
    wide = torch.zeros(2, 100)
    assert PF.topk_rows_reference(wide, 64)[0].shape == (2, 64)
    with pytest.raises(ValueError):
        PF.topk_rows_reference(wide, 65)
    with pytest.raises(ValueError):
        PF.topk_rows_reference(torch.zeros(2, 0), 1)


# --------------------------------------------------------------------------------------------
# NeuralNetworkModel.classify / score / generate
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def char_model():
    torch.manual_seed(3)
    model = NeuralNetworkModel("chars", CHAR_SIZES, activation_algos=CHAR_ALGOS, bias_algo="random")
    ids = torch.randint(0, 27, (64, 3), generator=torch.Generator().manual_seed(4))
    model.compute_output(ids.tolist(), [[int(i)] for i in ids[:, 0]])
    return model


@pytest.fixture(scope="module")
def dense_model():
    torch.manual_seed(5)
    return NeuralNetworkModel("dense", [9, 18, 12], activation_algos=["relu", "softmax"], bias_algo="random")


def _check_against_predict(model, rows, k):
    out = model.classify(rows, top_k=k)
    assert sorted(out) == ["classes", "probabilities"]
    probs = torch.tensor(model.predict(rows), dtype=torch.float64)
    assert len(out["classes"]) == len(rows) == len(out["probabilities"])
    for p, classes, got in zip(probs, out["classes"], out["probabilities"]):
        assert classes == torch.sort(p, descending=True, stable=True).indices[:k].tolist()
        assert all(isinstance(c, int) for c in classes)
        assert got == pytest.approx(p[classes].tolist(), rel=1e-12, abs=1e-300)
    return out


def test_cpu_classify_is_the_stable_argsort_of_predict(char_model, dense_model):
    g = torch.Generator().manual_seed(9)
    boards = torch.randint(-1, 2, (6, 9), generator=g).double().tolist()
    for k in (1, 3, 12):
        _check_against_predict(dense_model, boards, k)
    ids = torch.randint(0, 27, (7, 3), generator=g).tolist()
    for k in (1, 5, 27):
        _check_against_predict(char_model, ids, k)
    # a vector gives flat lists, a batch of one gives one list per row
    batch = dense_model.classify(boards[:1], top_k=4)
    single = dense_model.classify(boards[0], top_k=4)
    assert single == {"classes": batch["classes"][0], "probabilities": batch["probabilities"][0]}
    assert len(single["classes"]) == 4 and isinstance(single["classes"][0], int)
    assert char_model.classify(ids[0], top_k=2) == {k: v[0] for k, v in char_model.classify(ids[:1], top_k=2).items()}
    assert dense_model.classify(boards[0]) == dense_model.classify(boards[0], top_k=1)  # the default
    assert sum(dense_model.classify(boards[0], top_k=12)["probabilities"]) == pytest.approx(1.0, rel=1e-12)


def test_cpu_classify_refusals(char_model, dense_model):
    board = [0.0] * 9
    for bad in (0, 13, -1, True, 2.0, "3", None):
        with pytest.raises(ValueError):
            dense_model.classify(board, top_k=bad)
    for kw in ({"weights": "int4"}, {"weights": "fp8"}):
        with pytest.raises(ValueError):
            dense_model.classify(board, **kw)
    sigmoid = NeuralNetworkModel("sig", [9, 18, 9], activation_algos=["relu", "sigmoid"])
    with pytest.raises(ValueError, match="softmax"):
        sigmoid.classify(board)
    with pytest.raises(IndexError):
        char_model.classify([[1, 2, 27]])


def test_cpu_score_top_logprobs_agree_with_the_scores(char_model, monkeypatch):
    greedy = char_model.generate([5], 4, temperature=0.0, seed=0)["tokens"][0]  # ids of rank 0 after [5]
    rows = [[5], [1, 2, 3], [9, 9, 4, 5, 6, 0, 26], [5] + greedy]  # ragged: 1, 3, 7 and 5 ids
    plain = char_model.score(rows)
    k = 4
    out = char_model.score(rows, top_logprobs=k)
    assert sorted(out) == sorted(list(plain) + ["top_tokens", "top_logprobs"])
    assert {key: out[key] for key in plain} == plain
    assert [len(r) for r in out["top_tokens"]] == [1, 3, 7, 5] == [len(r) for r in out["top_logprobs"]]
    seen_first = seen_inside = 0
    for row, lps, ranks, tt, tl in zip(rows, out["logprobs"], out["ranks"], out["top_tokens"], out["top_logprobs"]):
        for token, lp, rank, top_t, top_l in zip(row, lps, ranks, tt, tl):
            assert len(top_t) == len(top_l) == k and top_l == sorted(top_l, reverse=True)
            assert (top_t[0] == token) == (rank == 0)
            seen_first += rank == 0
            if rank < k:
                assert top_t[rank] == token and top_l[rank] == pytest.approx(lp, rel=1e-12)
                seen_inside += 1
            else:
                assert token not in top_t
    assert seen_first >= 4 and seen_inside > seen_first  # every branch was taken
    full = char_model.score(rows[1], top_logprobs=27)
    assert [sorted(t) for t in full["top_tokens"][0]] == [list(range(27))] * 3
    with pytest.raises(ValueError, match="details"):
        char_model.score(rows, details=False, top_logprobs=2)
    for bad in (0, 28, 65, True, 2.0):
        with pytest.raises(ValueError):
            char_model.score(rows, top_logprobs=bad)
    monkeypatch.setattr(NeuralNetworkModel, "SCORE_MAX_IDS", 16)
    assert char_model.score([[1, 2, 3, 4], [5]], top_logprobs=2)["tokens"] == 5  # 2 rows of up to 4, 2 each
    with pytest.raises(ValueError, match="too many"):
        char_model.score([[1, 2, 3, 4], [5]], top_logprobs=3)


def test_cpu_score_top_logprobs_run_in_the_same_chunks(char_model, monkeypatch):
    rows = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11]]
    want = char_model.score(rows, top_logprobs=3)
    monkeypatch.setattr(NeuralNetworkModel, "SCORE_LAYERS_BYTES", 8 * 27 * 5)  # 5 windows per chunk
    got = char_model.score(rows, top_logprobs=3)
    assert got["top_tokens"] == want["top_tokens"]
    for a, b in zip(got["top_logprobs"], want["top_logprobs"]):
        assert [v for e in a for v in e] == pytest.approx([v for e in b for v in e], rel=1e-12)


def test_cpu_generate_top_logprobs(char_model, monkeypatch):
    ctx = [[5], [1, 2, 3], [9, 9, 4, 5, 6]]
    plain = char_model.generate(ctx, 12, seed=5, top_k=5, temperature=0.7)
    out = char_model.generate(ctx, 12, seed=5, top_k=5, temperature=0.7, top_logprobs=3)
    assert sorted(out) == ["seed", "tokens", "top_logprobs", "top_tokens"] and out["tokens"] == plain["tokens"]
    both = char_model.generate(ctx, 12, seed=5, top_k=5, temperature=0.7, top_logprobs=3, logprobs=True)
    assert sorted(both) == ["logprobs", "seed", "tokens", "top_logprobs", "top_tokens"]
    assert both["top_tokens"] == out["top_tokens"] and both["top_logprobs"] == out["top_logprobs"]
    for c, row, lps, tt, tl in zip(ctx, both["tokens"], both["logprobs"], both["top_tokens"], both["top_logprobs"]):
        assert len(tt) == len(tl) == len(row) == 12
        scored = char_model.score(c + row, top_logprobs=3)
        assert tt == scored["top_tokens"][0][len(c):]
        assert [v for e in tl for v in e] == pytest.approx([v for e in scored["top_logprobs"][0][len(c):] for v in e], rel=1e-12)
        for token, lp, top_t, top_l in zip(row, lps, tt, tl):
            if token in top_t:
                assert top_l[top_t.index(token)] == pytest.approx(lp, rel=1e-12)
    greedy = char_model.generate(ctx, 8, temperature=0.0, seed=1, top_logprobs=2)
    assert greedy["tokens"] == [[e[0] for e in row] for row in greedy["top_tokens"]]
    stop = plain["tokens"][0][3]
    cut = char_model.generate(ctx, 12, seed=5, top_k=5, temperature=0.7, stop_token=stop, top_logprobs=3)
    assert [len(r) for r in cut["top_tokens"]] == [len(r) for r in cut["tokens"]] == [len(r) for r in cut["top_logprobs"]]
    assert len(cut["tokens"][0]) <= 4 and cut["top_tokens"][0] == out["top_tokens"][0][:len(cut["tokens"][0])]
    for bad in (0, 28, True, 1.5):
        with pytest.raises(ValueError, match="top_logprobs"):
            char_model.generate(ctx, 2, top_logprobs=bad)

    calls = []
    real = PF.topk_rows_reference
    monkeypatch.setattr(PF, "topk_rows_reference", lambda *a: calls.append(1) or real(*a))
    again = char_model.generate(ctx, 12, seed=5, top_k=5, temperature=0.7, logprobs=True)
    assert "top_tokens" not in again and calls == []  # unset: no key, no selection
    char_model.generate(ctx, 12, seed=5, top_logprobs=2)
    assert calls == [1]  # one batched pass, not one per token


# --------------------------------------------------------------------------------------------
# REST
# --------------------------------------------------------------------------------------------
@pytest.fixture
def client(models_tmpdir):
    main._predict_cache.clear()
    with TestClient(main.app) as c:
        yield c
    main._predict_cache.clear()


def test_rest_classify_round_trip_and_errors(client):
    body = {"model_id": "moves", "layer_sizes": [9, 18, 9], "activation_algos": ["relu", "softmax"]}
    assert client.post("/model/", json=body).status_code == 200
    model = NeuralNetworkModel.deserialize("moves")
    boards = [[1, -1, 0, 0, -1, 0, 0, 0, 0], [0] * 9, [1, 1, -1, -1, 0, 0, 1, 0, -1]]
    r = client.post("/classify/", json={"model_id": "moves", "inputs": boards, "top_k": 3})
    assert r.status_code == 200, r.text
    assert r.json() == model.classify(boards, top_k=3) and [len(c) for c in r.json()["classes"]] == [3, 3, 3]
    r = client.post("/classify/", json={"model_id": "moves", "inputs": boards[0]})
    assert r.status_code == 200 and r.json() == model.classify(boards[0]) and len(r.json()["classes"]) == 1
    for bad in ({"inputs": boards, "top_k": 0}, {"inputs": boards, "top_k": 10}, {"inputs": [[1, 2]]}, {"inputs": []},
                {"inputs": boards, "weights": "fp8"}, {"inputs": boards, "weights": "int4"}):
        r = client.post("/classify/", json={"model_id": "moves", **bad})
        assert r.status_code == 400, (bad, r.text)
        assert "Value error occurred" in r.json()["detail"]
    assert client.post("/classify/", json={"model_id": "nobody", "inputs": boards}).status_code == 404
    assert client.post("/classify/", json={"model_id": "moves"}).status_code == 422
    assert client.post("/classify/", json={"model_id": "moves", "inputs": boards, "top_k": "many"}).status_code == 422
    body = {"model_id": "sig", "layer_sizes": [9, 18, 9], "activation_algos": ["relu", "sigmoid"]}
    assert client.post("/model/", json=body).status_code == 200
    assert client.post("/classify/", json={"model_id": "sig", "inputs": boards}).status_code == 400
    body = {"model_id": "chars", "layer_sizes": CHAR_SIZES, "activation_algos": CHAR_ALGOS}
    assert client.post("/model/", json=body).status_code == 200
    r = client.post("/classify/", json={"model_id": "chars", "inputs": [[1, 2, 3], [4, 5, 6]], "top_k": 2})
    assert r.status_code == 200 and [len(c) for c in r.json()["classes"]] == [2, 2]
    assert client.post("/classify/", json={"model_id": "chars", "inputs": [[1, 2, 27]]}).status_code == 400  # a bad id


def test_rest_classify_passes_weights_down_only_when_sent(client, monkeypatch):
    body = {"model_id": "moves", "layer_sizes": [9, 18, 9], "activation_algos": ["relu", "softmax"]}
    assert client.post("/model/", json=body).status_code == 200
    seen = []
    monkeypatch.setattr(NeuralNetworkModel, "classify",
                        lambda self, *a, **k: seen.append(k) or {"classes": [0], "probabilities": [1.0]})
    assert client.post("/classify/", json={"model_id": "moves", "inputs": [0] * 9}).status_code == 200
    assert client.post("/classify/", json={"model_id": "moves", "inputs": [0] * 9, "top_k": 2, "weights": "fp8"}).status_code == 200
    assert seen == [{"top_k": 1}, {"top_k": 2, "weights": "fp8"}]


def test_rest_top_logprobs_reach_score_and_generate_only_when_sent(client, monkeypatch):
    body = {"model_id": "chars", "layer_sizes": CHAR_SIZES, "activation_algos": CHAR_ALGOS}
    assert client.post("/model/", json=body).status_code == 200
    seen = {"score": [], "generate": []}
    real = {"score": NeuralNetworkModel.score, "generate": NeuralNetworkModel.generate}

    def spy(name):
        def call(self, *args, **kwargs):
            seen[name].append(kwargs)
            return real[name](self, *args, **kwargs)
        return call

    monkeypatch.setattr(NeuralNetworkModel, "score", spy("score"))
    monkeypatch.setattr(NeuralNetworkModel, "generate", spy("generate"))
    model = NeuralNetworkModel.deserialize("chars")
    rows = [[5, 13, 13, 1, 0], [1, 22, 1, 0]]
    plain = client.post("/score/", json={"model_id": "chars", "sequences": rows})
    top = client.post("/score/", json={"model_id": "chars", "sequences": rows, "top_logprobs": 3})
    assert plain.status_code == 200 and top.status_code == 200, top.text
    assert "top_logprobs" not in seen["score"][0] and seen["score"][1]["top_logprobs"] == 3
    assert "top_tokens" not in plain.json() and top.json() == real["score"](model, rows, top_logprobs=3)
    assert [len(r) for r in top.json()["top_tokens"]] == [5, 4] and len(top.json()["top_tokens"][0][0]) == 3
    for bad in ({"top_logprobs": 0}, {"top_logprobs": 28}, {"top_logprobs": 2, "details": False}):
        assert client.post("/score/", json={"model_id": "chars", "sequences": rows, **bad}).status_code == 400, bad

    ok = {"model_id": "chars", "context": [[1, 2, 3]], "max_new_tokens": 6, "seed": 3}
    plain = client.post("/generate/", json=ok)
    top = client.post("/generate/", json={**ok, "top_logprobs": 2})
    assert plain.status_code == 200 and top.status_code == 200, top.text
    assert "top_logprobs" not in seen["generate"][0] and seen["generate"][1]["top_logprobs"] == 2
    assert "top_tokens" not in plain.json() and top.json()["tokens"] == plain.json()["tokens"]
    assert top.json() == real["generate"](model, [[1, 2, 3]], 6, seed=3, top_logprobs=2)
    assert client.post("/generate/", json={**ok, "top_logprobs": 65}).status_code == 400


def test_openapi_describes_the_new_route_and_options(client):
    spec = client.get("/openapi.json").json()
    props = spec["components"]["schemas"]["ClassifyRequest"]["properties"]
    assert all("description" in props[k] for k in ("model_id", "inputs", "top_k", "weights"))
    assert props["top_k"]["default"] == 1
    for path in ("/classify/", "/predict/", "/generate/", "/score/"):
        examples = spec["paths"][path]["post"]["requestBody"]["content"]["application/json"]["examples"]
        assert set(examples) == {"single", "batch"}, path
    for schema in ("ScoreRequest", "GenerateRequest"):
        assert "description" in spec["components"]["schemas"][schema]["properties"]["top_logprobs"]
