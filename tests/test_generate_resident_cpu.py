"""The one-launch generation feature without a GPU: the LDS planner (``engine/resident.py``) on the
stage descriptions of the test models, the ``loop`` argument of ``NeuralNetworkModel.generate`` on a
CPU model, and the ``loop`` field of ``POST /generate/``."""
import pytest
from fastapi.testclient import TestClient

import main
from penr_oz_neural_network_torch_amd.engine.resident import (HEAD, H_TABLE_LDS, H_TOTAL, PARAM, RESIDENT_LDS_BYTES,
                                                              SAMPLER_LDS_BYTES, StageDesc, resident_plan)
from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel

CHAR_SIZES = [27, 10, 30, 64, 27]
CHAR_ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]
TANH, RELU = 3, 1


def _model_a(bias=True):
    return [StageDesc("embed", 0, 10, vocab=27), StageDesc("flatten", 10, 30, ratio=3),
            StageDesc("gemm", 30, 64, bias=bias), StageDesc("bn", 64, 64, act=TANH), StageDesc("gemm", 64, 27, bias=bias)], 3


def _model_b():
    return [StageDesc("embed", 0, 4, vocab=27), StageDesc("flatten", 4, 8, ratio=2), StageDesc("gemm", 8, 16, act=TANH),
            StageDesc("flatten", 16, 32, ratio=2), StageDesc("gemm", 32, 27)], 4


def _model_c():
    return [StageDesc("embed", 0, 6, vocab=300), StageDesc("flatten", 6, 18, ratio=3), StageDesc("gemm", 18, 40, act=RELU),
            StageDesc("gemm", 40, 300)], 3


@pytest.mark.parametrize("make", [_model_a, _model_b, _model_c])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_plan_regions_are_aligned_apart_and_inside_the_total(make, dtype):
    stages, length = make()
    plan = resident_plan(stages, dtype, length)
    assert not isinstance(plan, str), plan
    assert plan.table_in_lds and plan.total <= RESIDENT_LDS_BYTES and plan.total % 16 == 0
    assert plan.ints[H_TOTAL] == plan.total and plan.ints[H_TABLE_LDS] == 1
    spans = sorted(plan.regions.values())
    assert all(off % 16 == 0 and nbytes > 0 for off, nbytes in spans)
    assert all(a_off + a_len <= b_off for (a_off, a_len), (b_off, _) in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] <= plan.total
    assert plan.regions["sampler"][1] == SAMPLER_LDS_BYTES
    # the parameter table of the int list names the same offsets, in the order of plan.params
    assert plan.params[0] == (0, "table") and len(plan.ints) == HEAD + PARAM * len(plan.params) + 12 * (len(stages) - 1)
    for i, (stage, role) in enumerate(plan.params):
        off, numel, esize = plan.ints[HEAD + PARAM * i: HEAD + PARAM * (i + 1)]
        assert (off, numel * esize) == plan.regions["table" if role == "table" else f"{role}{stage}"]
        assert esize == (2 if role == "weights" and dtype == "bfloat16" else 4)


def test_plan_shapes_of_the_hierarchical_model():
    stages, length = _model_b()
    plan = resident_plan(stages, "float32", length)
    body = plan.ints[HEAD + PARAM * len(plan.params):]
    rows = [body[i:i + 4] for i in range(0, len(body), 12)]     # kind, P, K, N
    assert rows == [[0, 2, 2, 8], [1, 2, 8, 16], [0, 1, 2, 32], [1, 1, 32, 27]]
    assert plan.regions["buf0"][1] == 2 * 16 * 4               # the widest hidden output: 2 positions of 16


def test_plan_totals_grow_with_the_element_size_and_drop_absent_biases():
    for make in (_model_a, _model_b, _model_c):
        stages, length = make()
        assert resident_plan(stages, "float32", length).total > resident_plan(stages, "bfloat16", length).total
    with_bias, without = resident_plan(_model_a()[0], "float32", 3), resident_plan(_model_a(False)[0], "float32", 3)
    assert [r for _, r in without.params].count("bias") == 1 and [r for _, r in with_bias.params].count("bias") == 3
    assert without.total < with_bias.total


def test_table_placement_flips_at_the_budget_that_just_holds_it():
    stages, length = _model_a()
    full = resident_plan(stages, "float32", length)
    assert full.table_in_lds and full.regions["table"] == (full.total - 1088, 27 * 10 * 4)
    assert resident_plan(stages, "float32", length, budget=full.total).table_in_lds
    lean = resident_plan(stages, "float32", length, budget=full.total - 1)
    assert not isinstance(lean, str) and not lean.table_in_lds and "table" not in lean.regions
    assert lean.total == full.total - 1088 and lean.ints[HEAD] == -1 and lean.ints[H_TABLE_LDS] == 0
    # everything but the table keeps its place
    assert all(lean.regions[k] == v for k, v in full.regions.items() if k != "table")
    # one byte under what the rest needs: refused, with both numbers
    reason = resident_plan(stages, "float32", length, budget=lean.total - 1)
    assert isinstance(reason, str) and str(full.total) in reason and str(lean.total - 1) in reason


def test_reasons():
    stages, length = _model_a()
    wide = stages[:-1] + [StageDesc("gemm", 64, 8193)]
    wide[0] = StageDesc("embed", 0, 10, vocab=8193)
    assert "8192" in resident_plan(wide, "float32", length)
    big = [StageDesc("embed", 0, 64, vocab=27), StageDesc("flatten", 64, 192, ratio=3), StageDesc("gemm", 192, 1024, act=TANH),
           StageDesc("gemm", 1024, 27)]
    reason = resident_plan(big, "float32", 3)
    assert isinstance(reason, str) and str(RESIDENT_LDS_BYTES) in reason and "bytes of LDS" in reason
    assert int(reason.split("needs ")[1].split(" ")[0]) > 192 * 1024 * 4
    assert "embedding first" in resident_plan(stages[2:], "float32", 1)
    assert "embedding first" in resident_plan([], "float32", 1)
    assert "softmax head" in resident_plan(stages, "float32", length, head="mse")
    assert "float64" in resident_plan(stages, "float64", length)
    assert "27 classes but embeds 20" in resident_plan([StageDesc("embed", 0, 10, vocab=20)] + stages[1:], "float32", length)
    assert "product of the flatten ratios" in resident_plan(stages, "float32", 6)


# --------------------------------------------------------------------------------------------
# NeuralNetworkModel.generate(loop=...)
# --------------------------------------------------------------------------------------------
def test_model_generate_loop_argument_on_a_cpu_model():
    model = NeuralNetworkModel("chars", CHAR_SIZES, activation_algos=CHAR_ALGOS)
    plain = model.generate([[1, 2, 3]], 5, seed=3)
    assert model.generate([[1, 2, 3]], 5, seed=3, loop=None) == plain
    with pytest.raises(ValueError, match="needs a model on a GPU"):
        model.generate([[1, 2, 3]], 5, seed=3, loop="resident")
    with pytest.raises(ValueError, match="unknown loop 'nonsense'"):
        model.generate([[1, 2, 3]], 5, seed=3, loop="nonsense")


# --------------------------------------------------------------------------------------------
# POST /generate/
# --------------------------------------------------------------------------------------------
@pytest.fixture
def client(models_tmpdir):
    main._predict_cache.clear()
    with TestClient(main.app) as c:
        yield c
    main._predict_cache.clear()


def test_rest_generate_loop_field(client):
    body = {"model_id": "chars", "layer_sizes": CHAR_SIZES, "activation_algos": CHAR_ALGOS}
    assert client.post("/model/", json=body).status_code == 200
    ok = {"model_id": "chars", "context": [[1, 2, 3]], "max_new_tokens": 4, "seed": 5}
    plain = client.post("/generate/", json=ok)
    assert plain.status_code == 200 and [len(t) for t in plain.json()["tokens"]] == [4]
    assert client.post("/generate/", json={**ok, "loop": None}).json() == plain.json()
    for loop, word in (("resident", "GPU"), ("nonsense", "unknown loop")):
        r = client.post("/generate/", json={**ok, "loop": loop})
        assert r.status_code == 400, r.text
        assert "Value error occurred" in r.json()["detail"] and word in r.json()["detail"]
    spec = client.get("/openapi.json").json()
    field = spec["components"]["schemas"]["GenerateRequest"]["properties"]["loop"]
    assert "resident" in field["description"]
