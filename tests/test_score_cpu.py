"""Sequence scoring without a GPU: the fp64 rule of ``PF.token_logprob_reference``,
``NeuralNetworkModel.score`` and ``generate(logprobs=True)`` through the layer loop, ``POST /score/``, and the
inputs of ``test_token_logprob_gpu.py`` (``tests/score_cases.py``)."""
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
def test_reference_on_hand_computed_rows():
    lp, rank = PF.token_logprob_reference(torch.tensor([[3.25]]), torch.tensor([0]))
    assert lp.dtype == torch.float64 and rank.dtype == torch.int64
    assert lp.tolist() == [0.0] and rank.tolist() == [0]
    flat = torch.full((5, 7), -2.5)
    lp, rank = PF.token_logprob_reference(flat, torch.arange(5))
    assert lp.tolist() == pytest.approx([-math.log(7)] * 5, rel=1e-15) and rank.tolist() == [0, 1, 2, 3, 4]
    row = torch.tensor([1.0, 3.0, 2.0], dtype=torch.float64)
    lse = math.log(math.exp(1.0) + math.exp(3.0) + math.exp(2.0))
    lp, rank = PF.token_logprob_reference(row.repeat(3, 1), torch.tensor([0, 1, 2]))
    assert lp.tolist() == pytest.approx([1.0 - lse, 3.0 - lse, 2.0 - lse], rel=1e-14) and rank.tolist() == [2, 0, 1]
    lp, rank = PF.token_logprob_reference(row, torch.tensor([1]))  # a vector is one row
    assert lp.tolist() == pytest.approx([3.0 - lse], rel=1e-14) and rank.tolist() == [0]


def test_reference_ties_infinities_and_bad_targets():
    row = torch.tensor([0.5, 2.0, -0.0, 2.0, 0.0, 2.0, -math.inf])
    lp, rank = PF.token_logprob_reference(row.repeat(7, 1), torch.arange(7))
    # ties rank by index; -0 == +0; rank 0 is the lowest index among the maxima (greedy sampling's pick)
    assert rank.tolist() == [3, 0, 4, 1, 5, 2, 6]
    assert int(PF.sample_rows_reference(row, (1, 2), 0, temperature=0.0)) == 1
    assert lp[6] == -math.inf and bool(torch.isfinite(lp[:6]).all())
    assert float(lp[:6].exp().sum()) == pytest.approx(1.0, rel=1e-14)  # the -inf column holds no mass
    lp, rank = PF.token_logprob_reference(row.repeat(4, 1), torch.tensor([7, -1, 1, 100]))
    assert [math.isnan(v) for v in lp.tolist()] == [True, True, False, True] and rank.tolist() == [-1, -1, 0, -1]
    far = torch.tensor([[100.0, 0.0, -60.0]])
    assert float(PF.token_logprob_reference(far, torch.tensor([2]))[0]) == pytest.approx(-160.0, rel=1e-12)
    # the rank is taken in the logits' own dtype: two bf16-equal logits tie
    lg = torch.tensor([[1.0, 1.0 + 2 ** -10]]).bfloat16()
    assert PF.token_logprob_reference(lg, torch.tensor([1]))[1].tolist() == [1]
    with pytest.raises(ValueError):
        PF.token_logprob_reference(torch.zeros(2, 3), torch.tensor([0]))


# --------------------------------------------------------------------------------------------
# NeuralNetworkModel.score / generate(logprobs=True)
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def char_model():
    torch.manual_seed(3)
    model = NeuralNetworkModel("chars", CHAR_SIZES, activation_algos=CHAR_ALGOS, bias_algo="random")
    ids = torch.randint(0, 27, (64, 3), generator=torch.Generator().manual_seed(4))
    model.compute_output(ids.tolist(), [[int(i)] for i in ids[:, 0]])
    return model


def _by_predict(model, row, pad=0):
    """log of predict() on each window at the target, and the rank in the same probabilities."""
    padded = [pad] * 3 + row
    probs = torch.tensor(model.predict([padded[j:j + 3] for j in range(len(row))]), dtype=torch.float64)
    lps, ranks = [], []
    for j, t in enumerate(row):
        p = probs[j]
        lps.append(math.log(float(p[t])))
        ranks.append(int((p > p[t]).sum() + (p[:t] == p[t]).sum()))
    return lps, ranks


def test_cpu_score_is_the_log_of_predict_on_every_window(char_model):
    rows = [[5], [1, 2, 3], [9, 9, 4, 5, 6, 0, 26]]  # ragged: 1, 3 and 7 ids
    out = char_model.score(rows)
    assert sorted(out) == ["logprobs", "nll", "perplexity", "ranks", "tokens", "top1"]
    assert out["tokens"] == 11 and [len(r) for r in out["logprobs"]] == [1, 3, 7] == [len(r) for r in out["ranks"]]
    flat_lp, flat_rank = [], []
    for row, lps, ranks in zip(rows, out["logprobs"], out["ranks"]):
        want_lp, want_rank = _by_predict(char_model, row)
        assert lps == pytest.approx(want_lp, rel=1e-12) and ranks == want_rank
        flat_lp += lps
        flat_rank += ranks
    assert out["nll"] == pytest.approx(-math.fsum(flat_lp) / 11, rel=1e-12)
    assert out["perplexity"] == pytest.approx(math.exp(out["nll"]), rel=1e-12)
    assert out["top1"] == flat_rank.count(0) / 11
    brief = char_model.score(rows, details=False)
    assert brief == {k: out[k] for k in ("tokens", "nll", "perplexity", "top1")}
    assert char_model.score(rows[1]) == char_model.score([rows[1]])  # one list is one row
    # the left padding is an input like any other
    assert char_model.score([[5]], pad_token=7)["logprobs"][0] == pytest.approx(_by_predict(char_model, [5], 7)[0], rel=1e-12)
    assert char_model.score([[5]], pad_token=7)["logprobs"] != char_model.score([[5]])["logprobs"]


def test_cpu_score_runs_in_chunks_of_windows(char_model, monkeypatch):
    rows = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11]]
    want = char_model.score(rows)
    calls = []
    real = PF.token_logprob_reference

    def spy(logits, targets):
        calls.append(logits.shape[0])
        return real(logits, targets)

    monkeypatch.setattr(PF, "token_logprob_reference", spy)
    monkeypatch.setattr(NeuralNetworkModel, "SCORE_LAYERS_BYTES", 8 * 27 * 5)  # 5 windows per chunk
    got = char_model.score(rows)
    assert calls == [5, 5, 5, 1]  # 2 rows x 8 columns with the padding
    assert got["ranks"] == want["ranks"] and got["nll"] == pytest.approx(want["nll"], rel=1e-12)
    for a, b in zip(got["logprobs"], want["logprobs"]):
        assert a == pytest.approx(b, rel=1e-12)


@pytest.mark.parametrize("bad", [[], [[]], [[1], []], "abc", [[1, "a"]], [[1.5]], [[True]], [1, [2]], None])
def test_score_refuses_malformed_sequences(char_model, bad):
    with pytest.raises(ValueError):
        char_model.score(bad)


def test_score_refuses_bad_options_ids_and_models(char_model, monkeypatch):
    monkeypatch.setattr(NeuralNetworkModel, "SCORE_MAX_IDS", 8)
    assert char_model.score([[1, 2, 3, 4], [5]])["tokens"] == 5  # 2 rows of up to 4
    with pytest.raises(ValueError, match="too many"):
        char_model.score([[1, 2, 3, 4, 5], [5]])
    for kw in ({"pad_token": 27}, {"pad_token": -1}, {"pad_token": 1.0}, {"weights": "int4"}, {"weights": "fp8"},
               {"details": 1}):
        with pytest.raises(ValueError):
            char_model.score([[1, 2]], **kw)
    for ids in ([[1, 27]], [[-1]], [[0, 5], [5, 100]]):
        with pytest.raises(IndexError):
            char_model.score(ids)
    dense = NeuralNetworkModel("dense", [9, 18, 9], activation_algos=["relu", "sigmoid"])
    with pytest.raises(ValueError, match="embedding"):
        dense.score([[1, 2, 3]])
    headless = NeuralNetworkModel("headless", [27, 10, 30, 27], activation_algos=["embedding", "linear", "tanh"])
    with pytest.raises(ValueError, match="softmax"):
        headless.score([[1, 2, 3]])


def test_cpu_generate_logprobs_are_the_scores_of_its_tokens(char_model, monkeypatch):
    ctx = [[5], [1, 2, 3], [9, 9, 4, 5, 6]]
    plain = char_model.generate(ctx, 12, seed=5, top_k=5, temperature=0.7)
    out = char_model.generate(ctx, 12, seed=5, top_k=5, temperature=0.7, logprobs=True)
    assert sorted(out) == ["logprobs", "seed", "tokens"] and out["tokens"] == plain["tokens"] and out["seed"] == 5
    for c, row, lps in zip(ctx, out["tokens"], out["logprobs"]):
        assert len(lps) == len(row) == 12
        seq = ([0] * 3 + c)[-3:] + row
        for s, (token, lp) in enumerate(zip(row, lps)):  # teacher-forced, temperature 1, the whole vocabulary
            p = torch.tensor(char_model.predict([seq[s:s + 3]])[0], dtype=torch.float64)
            assert lp == pytest.approx(math.log(float(p[token])), rel=1e-12), (s, token)
        assert lps == pytest.approx(char_model.score(c + row)["logprobs"][0][len(c):], rel=1e-12)
    stop = plain["tokens"][0][3]
    cut = char_model.generate(ctx, 12, seed=5, top_k=5, temperature=0.7, stop_token=stop, logprobs=True)
    assert [len(r) for r in cut["logprobs"]] == [len(r) for r in cut["tokens"]] and len(cut["tokens"][0]) <= 4
    assert cut["logprobs"][0] == out["logprobs"][0][:len(cut["tokens"][0])]
    with pytest.raises(ValueError, match="logprobs"):
        char_model.generate(ctx, 2, logprobs=1)

    calls = []
    real = PF.token_logprob_reference
    monkeypatch.setattr(PF, "token_logprob_reference", lambda *a: calls.append(1) or real(*a))
    again = char_model.generate(ctx, 12, seed=5, top_k=5, temperature=0.7)
    assert again == plain and "logprobs" not in again and calls == []  # unset: no key, no scoring call
    char_model.generate(ctx, 12, seed=5, logprobs=True)
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


def test_rest_score_round_trip_and_errors(client, monkeypatch):
    body = {"model_id": "chars", "layer_sizes": CHAR_SIZES, "activation_algos": CHAR_ALGOS}
    assert client.post("/model/", json=body).status_code == 200
    rows = [[5, 13, 13, 1, 0], [1, 22, 1, 0]]
    model = NeuralNetworkModel.deserialize("chars")
    r = client.post("/score/", json={"model_id": "chars", "sequences": rows})
    assert r.status_code == 200, r.text
    assert r.json() == model.score(rows)
    r = client.post("/score/", json={"model_id": "chars", "sequences": rows[0], "pad_token": 3, "details": False})
    assert r.status_code == 200 and r.json() == model.score(rows[0], pad_token=3, details=False)
    assert sorted(r.json()) == ["nll", "perplexity", "tokens", "top1"]
    for bad in ([[1, 27]], [[1], []], [], [[1, "a"]]):  # a bad id, an empty row, nothing, a non-id
        r = client.post("/score/", json={"model_id": "chars", "sequences": bad})
        assert r.status_code == 400, (bad, r.text)
        assert "Value error occurred" in r.json()["detail"]
    assert client.post("/score/", json={"model_id": "chars", "sequences": rows, "weights": "fp8"}).status_code == 400
    assert client.post("/score/", json={"model_id": "nobody", "sequences": rows}).status_code == 404
    monkeypatch.setattr(NeuralNetworkModel, "score", lambda *a, **k: pytest.fail("an oversized request reached the model"))
    big = client.post("/score/", json={"model_id": "chars", "sequences": [[1] * 1024] * 1025})  # 1,049,600 ids
    assert big.status_code == 400 and "1048576" in big.json()["detail"]
    spec = client.get("/openapi.json").json()
    props = spec["components"]["schemas"]["ScoreRequest"]["properties"]
    assert all("description" in props[k] for k in ("model_id", "sequences", "pad_token", "weights", "details"))
    examples = spec["paths"]["/score/"]["post"]["requestBody"]["content"]["application/json"]["examples"]
    assert set(examples) == {"single", "batch"}
    assert "description" in spec["components"]["schemas"]["GenerateRequest"]["properties"]["logprobs"]


def test_rest_generate_passes_logprobs_down_only_when_sent(client, monkeypatch):
    body = {"model_id": "chars", "layer_sizes": CHAR_SIZES, "activation_algos": CHAR_ALGOS}
    assert client.post("/model/", json=body).status_code == 200
    seen = []
    real = NeuralNetworkModel.generate

    def spy(self, *args, **kwargs):
        seen.append(kwargs)
        return real(self, *args, **kwargs)

    monkeypatch.setattr(NeuralNetworkModel, "generate", spy)
    ok = {"model_id": "chars", "context": [[1, 2, 3]], "max_new_tokens": 6, "seed": 3}
    plain = client.post("/generate/", json=ok)
    scored = client.post("/generate/", json={**ok, "logprobs": True})
    off = client.post("/generate/", json={**ok, "logprobs": False})
    assert plain.status_code == 200 and scored.status_code == 200 and off.status_code == 200, scored.text
    assert "logprobs" not in seen[0] and seen[1]["logprobs"] is True and seen[2]["logprobs"] is False
    assert "logprobs" not in plain.json() and off.json() == plain.json()
    want = real(NeuralNetworkModel.deserialize("chars"), [[1, 2, 3]], 6, seed=3, logprobs=True)
    assert scored.json() == want and scored.json()["tokens"] == plain.json()["tokens"]
    assert len(scored.json()["logprobs"][0]) == 6


# --------------------------------------------------------------------------------------------
# the inputs of test_token_logprob_gpu.py
# --------------------------------------------------------------------------------------------
def test_gpu_inputs_cover_what_they_must():
    cases = C.cases()
    have = {(kind, cols) for _, kind, _, cols, _ in cases}
    widths = (1, 2, 27, 63, 64, 65, 255, 256, 257, 1024, 1025, 4097, 8193)
    assert have >= {(kind, cols) for kind in ("normal", "flat", "peaked", "wide", "ties", "neginf") for cols in widths}
    assert have >= {("normal", 65613), ("ties", 65613)}
    for cols in widths:
        want = {1, 3, 4, 5, 257} if cols <= 1025 else {3}
        assert {rows for _, kind, rows, c, _ in cases if c == cols and kind == "normal"} == want
    underflowing = 0
    for name, kind, rows, cols, seed in cases:
        lg, t = C.make_logits(kind, rows, cols, seed), C.make_targets(kind, rows, cols, seed)
        assert lg.dtype == torch.float32 and lg.shape == (rows, cols) and t.dtype == torch.int64 and t.shape == (rows,)
        assert 0 <= int(t.min()) and int(t.max()) < cols, name
        if rows > 5:
            continue
        lp, rank = PF.token_logprob_reference(lg, t)
        if kind == "flat":
            assert rank.tolist() == t.tolist() and lp.tolist() == pytest.approx([-math.log(cols)] * rows, rel=1e-14)
        if kind == "ties":  # the fp32 and the fp64 rank rules agree, and at any width worth the name there are ties
            assert torch.equal(PF.token_logprob_reference(lg.double(), t)[1], rank), name
            if cols >= 27:
                assert int((lg == lg.gather(1, t.unsqueeze(1))).sum()) > rows, name
        if kind == "wide":  # targets below exp's fp32 underflow: their weight is 0, their score is not -inf
            underflowing += int((lp < -104).sum())
        if kind == "neginf" and cols >= 2:
            finite = torch.isfinite(lg.gather(1, t.unsqueeze(1))).reshape(-1)
            assert finite.tolist() == [True] * (rows - 1) + [rows < 2], name
            assert int(torch.isinf(lg[0]).sum()) == len(range(1, cols, 3))
            assert rows < 2 or lp.tolist()[-1] == -math.inf
    assert underflowing >= 20
