"""Top-k answers on the GPU: ``FusedPredictor.classify`` (forward kernels plus one ``pz::topk_rows`` launch),
``NeuralNetworkModel.classify``, ``score(top_logprobs=k)`` and ``generate(top_logprobs=k)`` on the character
model of ``test_score_gpu.py`` and on a ``[64, 128, 4096]`` relu / softmax model.

Classes are compared with the rule applied to the predictor's own fp32 logits (``_logits`` on the same rows, the
exact input of the launch), so the rounding of a bf16 forward cannot flip a near-tie; probabilities with the
kernel's bound of ``tests/score_cases.py`` carried through ``exp`` (``|d exp(l)| <= exp(l) * (e^tol - 1)``,
plus one fp32 rounding of the result)."""
import math

import pytest
import torch

from penr_oz_neural_network_torch_amd.engine.predictor import FusedPredictor
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import score_cases as C

pytestmark = pytest.mark.gpu

CHAR_SIZES = [27, 10, 30, 64, 27]
CHAR_ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]
CONTEXTS = [[5], [1, 2, 3], [9, 9, 4, 5, 6]]     # padded, exact, truncated
SEED = 11 + (22 << 32)


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
    torch.manual_seed(10)
    wide = NeuralNetworkModel("wide", [64, 128, 4096], activation_algos=["relu", "softmax"], bias_algo="random",
                              dtype="bfloat16", device="cuda:0")
    return {"float32": _char_model("float32"), "bfloat16": _char_model("bfloat16"), "wide": wide}


def _inputs(name, rows):
    g = torch.Generator().manual_seed(rows)
    if name == "wide":
        return torch.randn(rows, 64, generator=g).tolist()
    return torch.randint(0, 27, (rows, 3), generator=g).tolist()


def _check_classify(model, x, k, out, **weights):
    predictor = model._fused_predictor()
    assert isinstance(predictor, FusedPredictor)
    fp8 = weights.get("weights") == "fp8"
    logits = predictor._logits(model._input_tensor(x), fp8).reshape(len(x), -1).cpu()
    classes = logits.shape[1]
    ref_idx, ref_lp = PF.topk_rows_reference(logits, k)
    assert out["classes"] == ref_idx.tolist()
    got = torch.tensor(out["probabilities"], dtype=torch.float64)
    tol = ref_lp.exp() * torch.expm1(C.tolerance(classes, ref_lp)) + 2.0 ** -24 * ref_lp.exp()
    err = (got - ref_lp.exp()).abs()
    assert bool((err <= tol).all()), float((err / tol).max())
    return float((err / tol).max())


@pytest.mark.parametrize("rows", [1, 16, 70])  # the skinny forward below 64 rows, the tiled one from there
@pytest.mark.parametrize("name", ["float32", "bfloat16", "wide"])
def test_classify_is_the_rule_on_the_predictors_logits(models, name, rows, monkeypatch):
    model = models[name]
    x = _inputs(name, rows)
    launches, softmaxes = [], []
    real = PF.topk_rows
    monkeypatch.setattr(PF, "topk_rows", lambda lg, k, *a: launches.append((tuple(lg.shape), k)) or real(lg, k, *a))
    out = model.classify(x, top_k=5)
    classes = 4096 if name == "wide" else 27
    assert launches == [((rows, classes), 5)]  # one launch for the request
    monkeypatch.setattr(PF, "topk_rows", real)
    assert sorted(out) == ["classes", "probabilities"] and len(out["classes"]) == rows
    assert all(len(c) == 5 and all(isinstance(v, int) for v in c) for c in out["classes"])
    worst = _check_classify(model, x, 5, out)
    print(f"{name} {rows} rows: worst error / bound = {worst:.3f}")
    idx, logprob = model._fused_predictor().classify(model._input_tensor(x), 5)
    assert idx.is_cuda and idx.dtype == torch.int32 and logprob.dtype == torch.float32 and idx.shape == logprob.shape == (rows, 5)
    assert idx.tolist() == out["classes"]
    # a vector is one row: flat lists
    single = model.classify(x[0], top_k=5)
    assert single["classes"] == out["classes"][0] or rows >= 64  # (another GEMM from 64 rows on: bits may differ)
    assert len(single["probabilities"]) == 5 and isinstance(single["probabilities"][0], float)


def test_classify_options_and_refusals(models):
    model = models["bfloat16"]
    x = _inputs("bfloat16", 16)
    out = model.classify(x, top_k=3, weights="fp8")
    _check_classify(model, x, 3, out, weights="fp8")
    full = model.classify(x, top_k=27)
    assert [sorted(c) for c in full["classes"]] == [list(range(27))] * 16
    assert [sum(p) for p in full["probabilities"]] == pytest.approx([1.0] * 16, rel=1e-5)
    wide = models["wide"].classify(_inputs("wide", 3), top_k=64)
    assert [len(c) for c in wide["classes"]] == [64] * 3
    with pytest.raises(ValueError, match="fp8"):
        models["float32"].classify(x, weights="fp8")
    for bad in (0, 28, 65, True, 2.0):
        with pytest.raises(ValueError):
            model.classify(x, top_k=bad)
        with pytest.raises(ValueError):
            model._fused_predictor().classify(torch.tensor(x), bad)
    with pytest.raises(ValueError):
        models["wide"].classify(_inputs("wide", 2), top_k=65)
    with pytest.raises(IndexError):
        model.classify([[1, 2, 27]])
    sigmoid = NeuralNetworkModel("sig", [9, 18, 9], activation_algos=["relu", "sigmoid"], dtype="float32", device="cuda:0")
    with pytest.raises(ValueError, match="softmax"):
        sigmoid.classify([0.0] * 9)
    with pytest.raises(ValueError, match="softmax"):
        FusedPredictor(sigmoid).classify(torch.zeros(2, 9), 1)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_score_top_logprobs_leave_the_scores_alone(models, dtype):
    model = models[dtype]
    greedy = model.generate([5], 4, temperature=0.0, seed=0)["tokens"][0]
    rows = [[5], [1, 2, 3], [9, 9, 4, 5, 6, 0, 26], [5] + greedy]
    plain = model.score(rows)
    out = model.score(rows, top_logprobs=3)
    assert {key: out[key] for key in plain} == plain  # logprobs and ranks bit for bit
    assert [len(r) for r in out["top_tokens"]] == [1, 3, 7, 5] == [len(r) for r in out["top_logprobs"]]
    first = inside = 0
    for row, lps, ranks, tt, tl in zip(rows, out["logprobs"], out["ranks"], out["top_tokens"], out["top_logprobs"]):
        for token, lp, rank, top_t, top_l in zip(row, lps, ranks, tt, tl):
            assert len(top_t) == len(top_l) == 3 and top_l == sorted(top_l, reverse=True)
            assert (top_t[0] == token) == (rank == 0)
            first += rank == 0
            if rank < 3:
                assert top_t[rank] == token and top_l[rank] == lp  # the same bits (pz::token_logprob's)
                inside += 1
            else:
                assert token not in top_t
    assert first >= 4 and inside >= first
    with pytest.raises(ValueError, match="details"):
        model.score(rows, details=False, top_logprobs=3)
    with pytest.raises(ValueError):
        model.score(rows, top_logprobs=28)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_predictor_score_chunks_give_the_same_bits(models, dtype, monkeypatch):
    predictor = models[dtype]._fused_predictor()
    seq = torch.randint(0, 27, (8, 43), generator=torch.Generator().manual_seed(21))  # 320 windows
    launches = []
    real = PF.topk_rows
    monkeypatch.setattr(PF, "topk_rows", lambda lg, k, *a: launches.append(lg.shape[0]) or real(lg, k, *a))
    one = predictor.score(seq, chunk_rows=320, top_logprobs=4)
    many = predictor.score(seq, chunk_rows=64, top_logprobs=4)
    assert launches == [320] + [64] * 5  # one more launch per chunk
    assert len(one) == len(many) == 4 and one[2].shape == one[3].shape == (8, 40, 4)
    assert one[2].dtype == torch.int32 and one[3].dtype == torch.float32 and one[2].is_cuda
    for a, b in zip(one, many):  # (64 windows and 320 both take the tiled GEMMs)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    launches.clear()
    plain = predictor.score(seq, chunk_rows=64)
    assert launches == [] and len(plain) == 2  # unset: the launches and the result of before
    assert torch.equal(plain[0].view(torch.int32), many[0].view(torch.int32)) and torch.equal(plain[1], many[1])
    # against the rule on the chunk's own logits
    windows = seq.unfold(1, 3, 1)[:, :40].reshape(320, 3)
    logits = predictor._logits(windows).reshape(-1, 27).cpu()
    ref_idx, ref_lp = PF.topk_rows_reference(logits, 4)
    assert torch.equal(one[2].view(-1, 4).cpu().long(), ref_idx)
    err = (one[3].view(-1, 4).cpu().double() - ref_lp).abs()
    assert bool((err <= C.tolerance(27, ref_lp)).all())
    for bad in (0, 28, True):
        with pytest.raises(ValueError):
            predictor.score(seq, top_logprobs=bad)
    empty = predictor.score(torch.zeros(0, 5, dtype=torch.int64), top_logprobs=2)
    assert empty[2].shape == empty[3].shape == (0, 2, 2)


@pytest.mark.parametrize("dtype,kw", [("float32", {}), ("float32", {"loop": "resident"}), ("bfloat16", {}),
                                      ("bfloat16", {"loop": "resident"}), ("bfloat16", {"weights": "fp8"})],
                         ids=["f32", "f32-resident", "bf16", "bf16-resident", "bf16-fp8"])
def test_generate_top_logprobs(models, dtype, kw):
    model = models[dtype]
    weights = {k: v for k, v in kw.items() if k == "weights"}
    plain = model.generate(CONTEXTS, 8, seed=SEED, **kw)
    out = model.generate(CONTEXTS, 8, seed=SEED, top_logprobs=3, **kw)
    assert sorted(out) == ["seed", "tokens", "top_logprobs", "top_tokens"] and out["tokens"] == plain["tokens"]
    assert [len(r) for r in out["top_tokens"]] == [8, 8, 8] and all(len(e) == 3 for r in out["top_logprobs"] for e in r)
    both = model.generate(CONTEXTS, 8, seed=SEED, top_logprobs=3, logprobs=True, **kw)
    assert both["tokens"] == plain["tokens"] and both["top_tokens"] == out["top_tokens"]
    assert both["top_logprobs"] == out["top_logprobs"]
    for row, lps, tt, tl in zip(both["tokens"], both["logprobs"], both["top_tokens"], both["top_logprobs"]):
        for token, lp, top_t, top_l in zip(row, lps, tt, tl):
            if token in top_t:
                assert top_l[top_t.index(token)] == lp
    scored = model.score([c + row for c, row in zip(CONTEXTS, out["tokens"])], top_logprobs=3, **weights)
    assert out["top_tokens"] == [t[len(c):] for c, t in zip(CONTEXTS, scored["top_tokens"])]
    assert out["top_logprobs"] == [t[len(c):] for c, t in zip(CONTEXTS, scored["top_logprobs"])]
    assert all(v <= 0 and math.isfinite(v) for row in out["top_logprobs"] for e in row for v in e)
    stop = plain["tokens"][0][3]
    cut = model.generate(CONTEXTS, 8, seed=SEED, stop_token=stop, top_logprobs=3, **kw)
    assert [len(r) for r in cut["top_tokens"]] == [len(r) for r in cut["tokens"]] and len(cut["tokens"][0]) <= 4
    assert cut["top_tokens"][0] == out["top_tokens"][0][:len(cut["tokens"][0])]
    greedy = model.generate(CONTEXTS, 8, temperature=0, seed=1, top_logprobs=2, **kw)
    assert greedy["tokens"] == model.generate(CONTEXTS, 8, temperature=0, seed=1, **kw)["tokens"]
    # (the resident loop's logits differ from the scoring pass's by fp32 summation order only: on these fixed
    # contexts no two leading logits are that close, so its greedy tokens are the scoring pass's first choices too)
    assert greedy["tokens"] == [[e[0] for e in row] for row in greedy["top_tokens"]]
