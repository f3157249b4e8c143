"""Sequence scoring on the GPU: ``FusedPredictor.score`` (batched forward kernels plus one
``pz::token_logprob`` launch per chunk of windows), ``NeuralNetworkModel.score`` and
``generate(logprobs=True)`` on the character model of ``test_generate_gpu.py``.

The predictor is checked against its own fp32 logits (``_logits`` on the rows of each chunk, the exact input
of the launch) with the kernel's bound of ``tests/score_cases.py``; ranks exactly.

Accuracy rule, as ``test_predict_gpu.py``'s: against an fp64 torch forward from the masters, the float32
model's ``score()`` log-probabilities have a max abs error of at most 2x the error of the layer-loop scorer
(``_score_layers``) on the same GPU model, plus 1e-6 plus the kernel's bound.

Measured on an MI355X (max abs error of score() / of the layer-loop scorer against fp64, float32 character
model, 120 scored ids): 7.3e-7 / 3.6e-7, with a kernel bound of 8.8e-6; the kernel against its own logits used
at most 0.08 of its bound on these models (0.37 on the widest-spread inputs of test_token_logprob_gpu.py).
"""
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
    return {dtype: _char_model(dtype) for dtype in ("float32", "bfloat16")}


def _sequences(rows, width, seed):
    return torch.randint(0, 27, (rows, width), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("rows,scored,chunk", [(3, 20, None), (8, 40, 64)])
def test_predictor_scores_its_own_logits(models, dtype, rows, scored, chunk, monkeypatch):
    predictor = models[dtype]._fused_predictor()
    assert isinstance(predictor, FusedPredictor) and predictor.context_length == 3
    seq = _sequences(rows, 3 + scored, 21)
    launches = []
    real = PF.token_logprob
    monkeypatch.setattr(PF, "token_logprob", lambda lg, *a: launches.append(lg.shape[0]) or real(lg, *a))
    logprob, rank = predictor.score(seq) if chunk is None else predictor.score(seq, chunk_rows=chunk)
    total = rows * scored
    assert launches == ([total] if chunk is None else [64] * (total // 64))  # 320 windows: 5 chunks, tiled GEMMs
    assert logprob.shape == rank.shape == (rows, scored) and logprob.is_cuda and rank.is_cuda
    assert logprob.dtype == torch.float32 and rank.dtype == torch.int32
    windows = seq.unfold(1, 3, 1)[:, :scored].reshape(total, 3)
    targets = seq[:, 3:].reshape(-1)
    step = chunk or total
    worst = 0.0
    for i0 in range(0, total, step):
        logits = predictor._logits(windows[i0:i0 + step]).reshape(-1, 27)
        ref_lp, ref_rank = PF.token_logprob_reference(logits.cpu(), targets[i0:i0 + step])
        assert torch.equal(rank.view(-1)[i0:i0 + step].cpu().long(), ref_rank)
        err = (logprob.view(-1)[i0:i0 + step].cpu().double() - ref_lp).abs()
        assert bool((err <= C.tolerance(27, ref_lp)).all()), (i0, float(err.max()))
        worst = max(worst, float((err / C.tolerance(27, ref_lp)).max()))
    print(f"{dtype} {rows}x{scored}: worst error / bound = {worst:.3f}")


def _reference_logprob(model, seq) -> torch.Tensor:
    """fp64 torch forward from the master parameters, layers in eval mode: log-softmax at the scored ids."""
    scored = seq.shape[1] - 3
    h = seq.unfold(1, 3, 1)[:, :scored].reshape(-1, 3)
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
            h = h.log_softmax(-1)
        else:
            h = getattr(h, a)()
    return h.gather(1, seq[:, 3:].reshape(-1, 1)).reshape(seq.shape[0], scored)


def test_score_is_as_accurate_as_the_layer_loop(models):
    model = models["float32"]
    seq = _sequences(4, 33, 5)
    ref = _reference_logprob(model, seq)
    full = model.score(seq.tolist())  # (left-padded: the first three ids of a row are scored too, and dropped here)
    got = torch.tensor([row[3:] for row in full["logprobs"]], dtype=torch.float64)
    old = model._score_layers(seq)[0].cpu()
    err_new, err_old = float((got - ref).abs().max()), float((old - ref).abs().max())
    bound = float(C.tolerance(27, ref).max())
    print(f"score err {err_new:.3e}, layer-loop scorer err {err_old:.3e}, kernel bound {bound:.3e}")
    assert got.shape == ref.shape == old.shape == (4, 30)
    assert err_new <= 2.0 * err_old + 1e-6 + bound, (err_new, err_old, bound)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_score_result_shape(models, dtype, monkeypatch):
    model = models[dtype]
    rows = [[5], [1, 2, 3], [9, 9, 4, 5, 6, 0, 26]]
    out = model.score(rows)
    assert sorted(out) == ["logprobs", "nll", "perplexity", "ranks", "tokens", "top1"]
    assert out["tokens"] == 11 and [len(r) for r in out["logprobs"]] == [1, 3, 7] == [len(r) for r in out["ranks"]]
    flat = [v for row in out["logprobs"] for v in row]
    ranks = [v for row in out["ranks"] for v in row]
    assert all(v <= 0 for v in flat) and all(0 <= r < 27 for r in ranks)
    assert out["nll"] == pytest.approx(-math.fsum(flat) / 11, rel=1e-6)
    assert out["perplexity"] == pytest.approx(math.exp(-math.fsum(flat) / 11), rel=1e-6)
    assert out["top1"] == ranks.count(0) / 11
    # a row's scores do not depend on the rows it is padded against (fewer than 64 windows: the skinny GEMMs)
    alone = model.score(rows[1])
    assert alone["logprobs"] == [out["logprobs"][1]] and alone["ranks"] == [out["ranks"][1]]
    downloads = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: downloads.append(self.numel()) or real(self))
    brief = model.score(rows, details=False)
    assert brief == {k: out[k] for k in ("tokens", "nll", "perplexity", "top1")}
    assert max(downloads) <= 4  # the range check's four numbers and the two sums: nothing the size of the request


@pytest.mark.parametrize("dtype,kw", [("float32", {}), ("float32", {"loop": "resident"}), ("bfloat16", {}),
                                      ("bfloat16", {"loop": "resident"}), ("bfloat16", {"weights": "fp8"})],
                         ids=["f32", "f32-resident", "bf16", "bf16-resident", "bf16-fp8"])
def test_generate_logprobs(models, dtype, kw):
    model = models[dtype]
    weights = {k: v for k, v in kw.items() if k == "weights"}
    plain = model.generate(CONTEXTS, 8, seed=SEED, **kw)
    out = model.generate(CONTEXTS, 8, seed=SEED, logprobs=True, **kw)
    assert sorted(out) == ["logprobs", "seed", "tokens"] and out["tokens"] == plain["tokens"] and "logprobs" not in plain
    assert [len(r) for r in out["logprobs"]] == [8, 8, 8]
    # the same call path (fewer than 64 windows either way): bit for bit
    scored = model.score([c + row for c, row in zip(CONTEXTS, out["tokens"])], **weights)
    assert out["logprobs"] == [lps[len(c):] for c, lps in zip(CONTEXTS, scored["logprobs"])]
    windows = torch.tensor([([0] * 3 + c)[-3:] + row for c, row in zip(CONTEXTS, out["tokens"])])
    assert out["logprobs"] == model._predictor.score(windows, **weights)[0].tolist()
    assert all(v <= 0 and math.isfinite(v) for row in out["logprobs"] for v in row)
    stop = plain["tokens"][0][3]
    cut = model.generate(CONTEXTS, 8, seed=SEED, stop_token=stop, logprobs=True, **kw)
    assert [len(r) for r in cut["logprobs"]] == [len(r) for r in cut["tokens"]] and len(cut["tokens"][0]) <= 4
    assert cut["logprobs"][0] == out["logprobs"][0][:len(cut["tokens"][0])]
    greedy = model.generate(CONTEXTS, 8, temperature=0, seed=1, logprobs=True, **kw)
    if "loop" not in kw:  # (the resident loop's logits differ from the forward kernels' by summation order)
        ranks = model.score([c + row for c, row in zip(CONTEXTS, greedy["tokens"])], **weights)["ranks"]
        assert [r[len(c):] for c, r in zip(CONTEXTS, ranks)] == [[0] * 8] * 3


def test_generate_without_logprobs_launches_no_scorer(models, monkeypatch):
    model = models["float32"]
    calls = []
    real = PF.token_logprob
    monkeypatch.setattr(PF, "token_logprob", lambda *a: calls.append(a[0].shape[0]) or real(*a))
    model.generate(CONTEXTS, 8, seed=SEED)
    assert calls == []
    model.generate(CONTEXTS, 8, seed=SEED, logprobs=True)
    assert calls == [24]  # one launch for the request, not one per token


def test_errors(models):
    with pytest.raises(ValueError, match="fp8"):
        models["float32"].score([[1, 2, 3]], weights="fp8")
    with pytest.raises(ValueError, match="fp8"):
        models["float32"]._fused_predictor().score(torch.tensor([[1, 2, 3, 4]]), weights="fp8")
    dense = NeuralNetworkModel("dense", [9, 18, 9], activation_algos=["relu", "sigmoid"], dtype="float32", device="cuda:0")
    with pytest.raises(ValueError, match="embedding"):
        dense.score([[1, 2, 3]])
    with pytest.raises(ValueError, match="embedding"):
        FusedPredictor(dense).score(torch.tensor([[1, 2, 3, 4]]))
    headless = NeuralNetworkModel("headless", [27, 10, 30, 27], activation_algos=["embedding", "linear", "tanh"],
                                  dtype="float32", device="cuda:0")
    with pytest.raises(ValueError, match="softmax"):
        FusedPredictor(headless).score(torch.tensor([[1, 2, 3, 4]]))
    with pytest.raises(IndexError):
        models["float32"].score([[1, 2, 27]])
    predictor = models["float32"]._fused_predictor()
    with pytest.raises(IndexError):
        predictor.score(torch.tensor([[1, 2, 3, 27]]))   # a scored id that is no class
    with pytest.raises(IndexError):
        predictor.score(torch.tensor([[1, 27, 3, 4]]))   # a context id outside the table
    for bad in (torch.tensor([[1, 2, 3]]), torch.tensor([1, 2, 3, 4]), torch.tensor([[1.0, 2.0, 3.0, 4.0]])):
        with pytest.raises(ValueError):
            predictor.score(bad)  # no id to score; not a matrix; not ids
    with pytest.raises(ValueError):
        predictor.score(torch.tensor([[1, 2, 3, 4]]), chunk_rows=0)
    empty_lp, empty_rank = predictor.score(torch.zeros(0, 5, dtype=torch.int64))
    assert empty_lp.shape == empty_rank.shape == (0, 2)
