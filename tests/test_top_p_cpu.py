"""Nucleus (top-p) and min-p sampling without a GPU: the fp64 rule of ``PF.sample_rows_reference``,
``NeuralNetworkModel.generate`` through the layer loop, ``POST /generate/``, and the proof that the
fixed-seed inputs of ``test_top_p_gpu.py`` leave the fp64 reference unambiguous within that file's caps
(``tests/top_p_cases.py`` holds the inputs, the tolerances and their derivation)."""
import math

import pytest
import torch
from fastapi.testclient import TestClient

import main
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import top_p_cases as C

SEED = C.SEED
CHAR_SIZES = [27, 10, 30, 64, 27]
CHAR_ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]
N = 4096  # (row, step) draws of a hand-checkable row: the lightest kept column (1/16 of 5/8 at least) has
#           probability 0.1, so it is missed with probability 0.9^4096 < 1e-180


def _drawn(row, n=N, steps=2, **kw):
    """The set of tokens over ``n / steps`` rows times ``steps`` steps of one row of logits."""
    lg = row.repeat(n // steps, 1)
    out = set()
    for s in range(steps):
        out |= set(PF.sample_rows_reference(lg, SEED, s, **kw).tolist())
    return out


# --------------------------------------------------------------------------------------------
# the rule
# --------------------------------------------------------------------------------------------
def test_top_p_keeps_the_smallest_set_that_reaches_the_mass():
    row, order = C.hand_row(), C.HAND_ORDER  # probabilities 1/2, 1/4, 1/8, 1/16, 1/16 in a permuted column order
    assert _drawn(row, top_p=0.6) == set(order[:2])    # 1/2 < 0.6 <= 3/4
    assert _drawn(row, top_p=0.5) == set(order[:1])    # the mass above the second column is 1/2, not < 1/2
    assert _drawn(row, top_p=0.76) == set(order[:3])   # 3/4 < 0.76 <= 7/8
    assert _drawn(row, top_p=0.9) == set(order)        # 7/8 < 0.9: the two tied at 1/16 come together
    assert _drawn(row, top_p=1e-9) == set(order[:1])   # the most likely column always stays


def test_ties_with_the_last_admitted_column_all_stay():
    row = torch.tensor([0.0, 2.0, -1.0, 2.0, 2.0, 0.5, 2.0])
    assert _drawn(row, top_p=0.1) == {1, 3, 4, 6}
    assert _drawn(row, top_p=0.1, temperature=3.0) == {1, 3, 4, 6}


def test_min_p_drops_what_is_too_unlikely_next_to_the_maximum():
    row, order = C.hand_row(), C.HAND_ORDER  # weights relative to the maximum: 1, 1/2, 1/4, 1/8, 1/8
    assert _drawn(row, min_p=0.2) == set(order[:3])
    assert _drawn(row, min_p=0.126) == set(order[:3])
    assert _drawn(row, min_p=0.124) == set(order)
    assert _drawn(row, min_p=0.999) == set(order[:1])


def test_top_p_takes_the_nucleus_of_the_renormalised_top_k():
    row, order = C.hand_row(), C.HAND_ORDER  # top-3 renormalised: 4/7, 2/7, 1/7
    assert _drawn(row, top_k=3, top_p=0.9) == set(order[:3])    # 6/7 < 0.9
    assert _drawn(row, top_k=3, top_p=0.85) == set(order[:2])   # 4/7 < 0.85 <= 6/7
    assert _drawn(row, top_p=0.85) == set(order[:3])            # without top-k: 3/4 < 0.85 <= 7/8
    # min-p first, then the nucleus of what is left: {1/2, 1/4, 1/8} again
    assert _drawn(row, min_p=0.2, top_p=0.85) == set(order[:2])


@pytest.mark.parametrize("kw", [{}, {"top_k": 7}, {"temperature": 0.6}])
def test_off_values_give_todays_tokens(kw):
    lg = C.make_logits("gauss", 64, 101, 7)
    for step in range(3):
        want = PF.sample_rows_reference(lg, SEED, step, **kw)
        for top_p in (None, 1.0):
            for min_p in (None, 0.0):
                assert torch.equal(PF.sample_rows_reference(lg, SEED, step, top_p=top_p, min_p=min_p, **kw), want)


def test_draw_frequencies_inside_the_nucleus():
    n = 16384
    one = C.make_logits("gauss", 1, 27, 3) / 3.0
    lg = one.repeat(n, 1)
    got = PF.sample_rows_reference(lg, SEED, 0, top_p=0.8, min_p=0.02)
    nucleus, _, _ = C.analyse(one, 1.0, None, 0.8, 0.02)
    p = torch.where(nucleus[0], one[0].double().softmax(0), torch.zeros(27, dtype=torch.float64))
    p = p / p.sum()
    assert 3 <= int(nucleus.sum()) < 27
    counts = torch.bincount(got, minlength=27).double()
    for c in range(27):
        assert abs(counts[c] / n - p[c]) <= 5.0 / math.sqrt(n), (c, counts[c] / n, float(p[c]))


def test_rows_are_independent_and_greedy_ignores_the_options():
    lg = C.make_logits("heavy", 64, 65, 9)
    kw = dict(temperature=0.9, top_k=40, top_p=0.7, min_p=0.01)
    whole = PF.sample_rows_reference(lg, SEED, 2, **kw)
    for r in (0, 1, 17, 63):
        assert PF.sample_rows_reference(lg[r], SEED, 2, row0=r, **kw).tolist() == [int(whole[r])]
    assert torch.equal(PF.sample_rows_reference(lg[10:20], SEED, 2, row0=10, **kw), whole[10:20])
    greedy = PF.sample_rows_reference(lg, SEED, 0, temperature=0.0)
    assert torch.equal(PF.sample_rows_reference(lg, SEED, 0, temperature=0.0, top_p=0.3, min_p=0.5), greedy)


@pytest.mark.parametrize("kw", [{"top_p": 0.0}, {"top_p": -0.1}, {"top_p": 1.01}, {"top_p": float("nan")},
                                {"min_p": -0.1}, {"min_p": 1.0}, {"min_p": float("nan")}])
def test_bad_values_raise(kw, char_model):
    with pytest.raises(ValueError):
        PF.sample_rows_reference(C.make_logits("gauss", 2, 5, 0), SEED, 0, **kw)
    with pytest.raises(ValueError, match=r"top_p must be in \(0, 1\]" if "top_p" in kw else r"min_p must be in \[0, 1\)"):
        char_model.generate([[1, 2, 3]], 4, **kw)


# --------------------------------------------------------------------------------------------
# NeuralNetworkModel.generate
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def char_model():
    torch.manual_seed(3)
    model = NeuralNetworkModel("chars", CHAR_SIZES, activation_algos=CHAR_ALGOS, bias_algo="random")
    ids = torch.randint(0, 27, (64, 3), generator=torch.Generator().manual_seed(4))
    model.compute_output(ids.tolist(), [[int(i)] for i in ids[:, 0]])
    return model


@pytest.mark.parametrize("kw", [{"top_p": 0.8}, {"min_p": 0.05}, {"top_p": 0.8, "top_k": 5, "min_p": 0.05, "temperature": 1.5}])
def test_cpu_generate_follows_the_reference(char_model, kw):
    ctx = [[0, 0, 1], [1, 2, 3], [4, 5, 6]]
    out = char_model.generate(ctx, 12, seed=5, **kw)
    assert out == char_model.generate(ctx, 12, seed=5, **kw)
    assert out["tokens"] != char_model.generate(ctx, 12, seed=5)["tokens"]
    for r, (c, row) in enumerate(zip(ctx, out["tokens"])):
        seq = c + row
        for s, token in enumerate(row):  # teacher-forced
            probs = torch.tensor(char_model.predict([seq[s:s + 3]])[0], dtype=torch.float64)
            assert token == int(PF.sample_rows_reference(probs.log().unsqueeze(0), (5, 0), s, row0=r, **kw)), (r, s)
    assert char_model.generate(ctx, 6, temperature=0, seed=1, **{k: v for k, v in kw.items() if k != "temperature"}) == \
        char_model.generate(ctx, 6, temperature=0, seed=1)


def test_cpu_generate_passes_the_options_down_only_when_set(char_model, monkeypatch):
    calls = []
    real = PF.sample_rows_reference

    def spy(*args, **kwargs):
        calls.append(kwargs)
        return real(*args, **kwargs)

    monkeypatch.setattr(PF, "sample_rows_reference", spy)
    char_model.generate([[1, 2, 3]], 2, seed=1)
    char_model.generate([[1, 2, 3]], 2, seed=1, top_p=0.5)
    char_model.generate([[1, 2, 3]], 2, seed=1, min_p=0.1, top_p=1)
    assert calls == [{}, {}, {"top_p": 0.5}, {"top_p": 0.5}, {"top_p": 1.0, "min_p": 0.1}, {"top_p": 1.0, "min_p": 0.1}]


# --------------------------------------------------------------------------------------------
# POST /generate/
# --------------------------------------------------------------------------------------------
@pytest.fixture
def client(models_tmpdir):
    main._predict_cache.clear()
    with TestClient(main.app) as c:
        yield c
    main._predict_cache.clear()


def test_rest_generate_takes_top_p_and_min_p(client, monkeypatch):
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
    nucleus = client.post("/generate/", json={**ok, "top_p": 0.3, "min_p": 0.1})
    assert plain.status_code == 200 and nucleus.status_code == 200, nucleus.text
    assert "top_p" not in seen[0] and "min_p" not in seen[0]  # they reach generate only when sent
    assert seen[1]["top_p"] == 0.3 and seen[1]["min_p"] == 0.1
    assert nucleus.json() == real(NeuralNetworkModel.deserialize("chars"), [[1, 2, 3]], 6, seed=3, top_p=0.3, min_p=0.1)
    for bad in ({"top_p": 0}, {"top_p": 1.5}, {"min_p": 1.0}, {"min_p": -0.5}):
        r = client.post("/generate/", json={**ok, **bad})
        assert r.status_code == 400, (bad, r.text)
        assert "Value error occurred" in r.json()["detail"]
    props = client.get("/openapi.json").json()["components"]["schemas"]["GenerateRequest"]["properties"]
    assert "description" in props["top_p"] and "description" in props["min_p"]


# --------------------------------------------------------------------------------------------
# the inputs of test_top_p_gpu.py: the reference alone is unambiguous within the caps
# --------------------------------------------------------------------------------------------
def test_gpu_inputs_are_unambiguous_within_the_caps():
    cases = C.cases()
    used = 0
    for name, kind, rows, cols, seed, kw in cases:
        n = C.ambiguous_draws(C.make_logits(kind, rows, cols, seed), C.STEPS, kw)
        if n:
            print(f"{name}: {n} of {rows * C.STEPS} draws are ambiguous in fp64")
        assert n <= C.CAP_DRAWS * rows * C.STEPS, name
        used += n > 0
    assert used <= C.CAP_CASES * len(cases), (used, len(cases))
    # every value the GPU file must cover is there
    assert {kw["top_p"] for *_, kw in cases} >= {0.05, 0.5, 0.9, 0.999}
    assert {kw["min_p"] for *_, kw in cases} >= {0.01, 0.3}
    assert {kw["top_k"] for *_, kw in cases} >= {1, 5, 50}
    assert {kw["temperature"] for *_, kw in cases} == {0.5, 1.0, 3.0}
    assert {c[3] for c in cases} == {1, 2, 27, 63, 64, 65, 4097, 8192, 8193, 65613}
    assert all({c[1] for c in cases if c[3] == cols} >= set(C.KINDS) for cols in C.SMALL + C.LARGE)
    for name, kind, rows, cols, seed, kw in cases:  # the flat rows: the select runs over many comparable columns
        if kind == "flat":
            sizes = C.analyse(C.make_logits(kind, rows, cols, seed), **kw)[0].sum(-1)
            assert float(sizes.double().mean()) >= 80, (name, sizes.tolist())  # (about 93 at 4097, 190 at 8193)
