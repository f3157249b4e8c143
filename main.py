"""REST microservice (reference L6/L8, ``main.py:1-370``): create / train / serve / inspect MLPs.

Routes, request schemas, defaults, status codes and error mapping are those of the reference so
existing clients, its test-suite and the dashboard work unchanged:

    GET  /              -> 307 /dashboard            GET /dashboard      -> HTML page
    POST /model/        create + serialize            POST /output/       inference (+ cost)
    POST /predict/      batch inference, outputs only (models stay loaded between requests)
    POST /generate/     token sampling from a next-token model (same loaded models as /predict/)
    POST /score/        log-probabilities, ranks and perplexity of given id sequences (same loaded models)
    PUT  /train/        202, training in background   (409 while that model is training)
    GET  /progress/     progress / avg cost / status  GET /stats/         training diagnostics
    DELETE /model/      204

Additions (optional, defaults reproduce the reference): ``dtype`` and ``device`` on model
creation (``"bfloat16"`` + ``"cuda"`` trains on the MI355X fused engine), ``GET /health``, and
multi-GPU data-parallel training of GPU models (``PZ_SERVICE_GPUS=N|auto``: this process is rank 0
of an N-rank RCCL group whose workers it starts at startup — ``parallel/service.py``).
Fixes of reference races: the 409 check happens before the model is loaded,
checkpoint files are replaced atomically (no torn reads from ``/progress/``), and exceptions in a
background training task are logged instead of vanishing.
"""
from __future__ import annotations

import logging
import os
import threading
from asyncio import Lock, create_task
from collections import OrderedDict
from contextlib import asynccontextmanager
from typing import Dict

from fastapi import Body, FastAPI, HTTPException, Request
from fastapi.concurrency import run_in_threadpool
from fastapi.params import Query
from fastapi.responses import HTMLResponse, JSONResponse, RedirectResponse, Response
from fastapi.staticfiles import StaticFiles
from fastapi.templating import Jinja2Templates
from pydantic import BaseModel, Field

from neural_net_model import NeuralNetworkModel
from penr_oz_neural_network_torch_amd.ops.functional import nucleus_args
from penr_oz_neural_network_torch_amd.parallel import service
from penr_oz_neural_network_torch_amd.utils import checkpoint as ckpt

_HERE = os.path.dirname(os.path.abspath(__file__))


@asynccontextmanager
async def lifespan(_: FastAPI):
    # PZ_SERVICE_GPUS=N|auto: GPU models train data-parallel on N GPUs (rank 0 = this process);
    # the worker ranks are started here, before anything in this process touches the GPU
    service.start_from_env()
    try:
        yield
    finally:
        service.stop()


app = FastAPI(
    title="Neural Network Model API",
    description="API to create, serialize, compute output and diagnose of neural network models.",
    version="0.0.1",
    lifespan=lifespan,
)
app.mount("/static", StaticFiles(directory=os.path.join(_HERE, "static")), name="static")
templates = Jinja2Templates(directory=os.path.join(_HERE, "templates"))

LOG_FORMAT = "%(asctime)s - %(name)s - %(levelname)s - %(message)s"
DATE_FORMAT = "%Y-%m-%dT%H:%M:%S"
logging.basicConfig(datefmt=DATE_FORMAT, format=LOG_FORMAT)
log = logging.getLogger(__name__)

# tic-tac-toe style examples for the OpenAPI docs: 9-cell board in {-1,0,1} -> one-hot next move
_BOARDS = [
    ([0, 0, 0, 0, 0, 0, 0, 0, 0], 4), ([0, 0, 0, 0, -1, 0, 0, 0, 0], 0), ([1, 0, 0, 0, -1, 0, 0, 0, 0], 1),
    ([1, -1, 0, 0, -1, 0, 0, 0, 0], 7), ([1, -1, 0, 0, -1, 0, 0, 1, 0], 2), ([1, -1, -1, 0, -1, 0, 0, 1, 0], 6),
    ([1, -1, -1, 0, -1, 0, 1, 1, 0], 8), ([1, -1, -1, 0, -1, 0, 1, 1, -1], 3), ([1, -1, -1, 1, -1, 0, 1, 1, -1], 5),
]
EXAMPLES = [{"activation_vector": board, "target_vector": [1 if i == move else 0 for i in range(9)]}
            for board, move in _BOARDS]


class InputItem(BaseModel):
    activation_vector: list = Field(..., description="The input activation data. 1D or 2D supported.")
    target_vector: list | None = Field(None, description="The optional expected target data same size as input data.")


class TrainingItem(InputItem):
    target_vector: list[float] = Field(..., description="The expected output vector, required for training items.")


class ModelRequest(BaseModel):
    model_id: str = Field(..., examples=["test"], description="The unique identifier for the model.")


class CreateModelRequest(ModelRequest):
    layer_sizes: list[int] = Field(..., examples=[[9, 1, 9, 9]],
                                   description="A list of integers representing the sizes of each layer in the neural network.")
    weight_algo: str = Field("xavier", examples=["xavier", "he", "gaussian"], description="An initialization algorithm")
    bias_algo: str = Field("random", examples=["random", "zeros"], description="An initialization algorithm")
    activation_algos: list[str] = Field(..., examples=[["sigmoid"] * 3, ["relu"] * 2 + ["sigmoid"],
                                                       ["relu"] * 2 + ["softmax"], ["embedding", "tanh"]],
                                        description="The activation algorithms to apply")
    optimizer: str = Field("adam", examples=["adam", "stochastic"],
                           description="The optimizer to use for updating for gradient descent")
    batchnorm_eps: float = Field(1e-5, examples=[1e-5], description="Batch Normalization Epsilon")
    batchnorm_momentum: float = Field(0.1, examples=[0.1], description="Batch Normalization Momentum")
    confidence: float = Field(1.0, examples=[1.0], description="Confidence factor for the last layer with weights")
    dtype: str | None = Field(None, examples=["float64", "bfloat16"],
                              description="Compute precision (default float64 = reference behaviour)")
    device: str | None = Field(None, examples=["cpu", "cuda"], description="Device to keep the model on (default cpu)")


class ActivationRequest(ModelRequest):
    input: InputItem = Field(..., description="The input data, an InputItem.")


class PredictRequest(ModelRequest):
    inputs: list = Field(..., description="One input vector (1D) or a batch of them (2D); id sequences for "
                                          "embedding models.")
    # (the OpenAPI example of this option is the field's own: the request-body examples stay the two above)
    weights: str | None = Field(None, examples=["fp8"],
                                description="Weight format to predict from. Omitted: the model's own precision. 'fp8': "
                                            "weight-only e4m3 copies, one power-of-two scale per output column (GPU "
                                            "models with dtype bfloat16 or fp8; anything else answers 400)")


class GenerateRequest(ModelRequest):
    context: list = Field(..., description="One id list or a batch of id lists. A row shorter than the model's context "
                                           "length is left-padded with pad_token; of a longer one the last ids count.")
    max_new_tokens: int = Field(..., description="Tokens to sample per row (1 to 4096).")
    temperature: float = Field(1.0, description="Softmax temperature; 0 is greedy (the most likely token).")
    top_k: int | None = Field(None, description="Sample among the k most likely tokens only (ties at the k-th stay).")
    top_p: float | None = Field(None, description="Nucleus sampling: sample among the smallest set of most likely tokens "
                                                  "that holds this share of the probability mass, in (0, 1]; ties with "
                                                  "the last one admitted stay. Omitted or 1: off.")
    min_p: float | None = Field(None, description="Drop tokens less than min_p times as likely as the most likely one, "
                                                  "in [0, 1). Omitted or 0: off.")
    seed: int | None = Field(None, description="64-bit seed naming the random draws; omitted: drawn by the server "
                                               "and returned, so the call can be repeated.")
    stop_token: int | None = Field(None, description="A row ends with its first occurrence of this id (inclusive).")
    pad_token: int = Field(0, description="Id that left-pads short context rows.")
    weights: str | None = Field(None, description="'fp8': weight-only e4m3 copies, as on /predict/.")
    loop: str | None = Field(None, description="'resident': the whole request as one GPU launch with the model held in "
                                               "on-chip memory (GPU models whose parameters fit in 160 KiB, at most "
                                               "8192 classes; anything else answers 400 with the reason). Omitted: "
                                               "one sampling launch per token.")
    logprobs: bool | None = Field(None, description="true: the response gains 'logprobs', the log-probability of every "
                                                    "returned token under the model's own distribution (temperature 1, "
                                                    "no top-k / top-p / min-p truncation), from one scoring pass after "
                                                    "the loop. Omitted: nothing extra is computed.")
    top_logprobs: int | None = Field(None, description="k in [1, min(classes, 64)]: the response gains 'top_tokens' and "
                                                       "'top_logprobs', for every returned token the k classes the model "
                                                       "found most likely at its position, most likely first, and their "
                                                       "log-probabilities, from the same scoring pass as logprobs. "
                                                       "Omitted: nothing extra is computed.")


class ClassifyRequest(ModelRequest):
    inputs: list = Field(..., description="One input vector (1D) or a batch of them (2D); id sequences for "
                                          "embedding models. The model must end in a softmax layer.")
    top_k: int = Field(1, description="How many of the most likely classes to return per row, in [1, min(classes, 64)], "
                                      "most likely first; equally likely classes in ascending order.")
    weights: str | None = Field(None, description="'fp8': weight-only e4m3 copies, as on /predict/.")


class ScoreRequest(ModelRequest):
    sequences: list = Field(..., description="One non-empty id list or a batch of non-empty id lists. Every id is scored "
                                             "given the ids before it (as many as the model's context length; a row is "
                                             "left-padded with pad_token). At most 1,048,576 ids per request.")
    pad_token: int = Field(0, description="Id that left-pads every row, as on /generate/.")
    weights: str | None = Field(None, description="'fp8': weight-only e4m3 copies, as on /predict/.")
    details: bool = Field(True, description="false: only tokens, nll, perplexity and top1 come back, no per-id lists.")
    top_logprobs: int | None = Field(None, description="k in [1, min(classes, 64)]: the response gains 'top_tokens' and "
                                                       "'top_logprobs', for every scored id the k classes the model found "
                                                       "most likely there, most likely first, and their log-probabilities "
                                                       "(needs details; rows x longest row x k at most 16,777,216). "
                                                       "Omitted: nothing extra is computed.")


class TrainingRequest(ModelRequest):
    training_data: list[TrainingItem] = Field(..., examples=[EXAMPLES], description="A list of training data pairs.")
    epochs: int = Field(10, examples=[10], description="The number of training epochs.")
    learning_rate: float = Field(0.01, examples=[0.01], description="The learning rate for training.")
    batch_size: int | None = Field(None, examples=[32], description="The batch size for training sample each epoch. (Optional)")
    decay_rate: float = Field(0.9, examples=[0.9], description="The decay rate of learning rate during training.")
    dropout_rate: float = Field(0.2, examples=[0.2],
                                description="The drop out rate of activated neurons to improve generalization")
    l2_lambda: float = Field(0.001, examples=[0.001],
                             description="The L2 Lambda penalty reducing weight magnitude during backpropagation")
    adam_beta1: float = Field(0.9, examples=[0.9],
                              description="The Adam optimizer parameter for gradient mean optimization after backpropagation")
    adam_beta2: float = Field(0.999, examples=[0.999],
                              description="The Adam optimizer parameter for gradient variance optimization after backpropagation")
    adam_epsilon: float = Field(1e-8, examples=[1e-8],
                                description="The Adam optimizer parameter for smallest step for gradient optimization after backpropagation")


class ModelIdQuery(Query):
    description = "The unique identifier for the model."


@app.exception_handler(Exception)
async def generic_exception_handler(_: Request, e: Exception):
    log.error(f"An error occurred: {str(e)}")
    return JSONResponse(status_code=500, content={"detail": "Please refer to server logs"})


@app.exception_handler(KeyError)
async def key_error_handler(_: Request, e: KeyError):
    raise HTTPException(status_code=404, detail=f"Not found error occurred: {str(e)}")


@app.exception_handler(ValueError)
async def value_error_handler(_: Request, e: ValueError):
    raise HTTPException(status_code=400, detail=f"Value error occurred: {str(e)}")


@app.get("/", include_in_schema=False)
def redirect_to_dashboard():
    return RedirectResponse(url="/dashboard")


@app.get("/dashboard", response_class=HTMLResponse)
async def dashboard(request: Request):
    return templates.TemplateResponse(request, "dashboard.html")


@app.get("/health")
def health():
    import torch
    gpus = torch.cuda.device_count() if torch.cuda.is_available() else 0
    from penr_oz_neural_network_torch_amd.ops import native
    group = service.get_group()
    return {"status": "ok", "gpus": gpus, "native": native.has_host_ops(), "training": sorted(
        k for k, v in model_locks.items() if v.locked()), "train_group": group.status() if group else None}


@app.post("/model/")
def create_model(body: CreateModelRequest = Body(...)):
    model_id = body.model_id
    log.info(f"Requesting creation of model {model_id}")
    kwargs = {}
    if body.dtype is not None:
        kwargs["dtype"] = body.dtype
    if body.device is not None:
        kwargs["device"] = body.device
    model = NeuralNetworkModel(model_id, body.layer_sizes, body.weight_algo, body.bias_algo, body.activation_algos,
                               body.optimizer, (body.batchnorm_eps, body.batchnorm_momentum), body.confidence,
                               **kwargs)
    model.serialize()
    return {"message": f"Model {model_id} created and saved successfully"}


@app.post("/output/")
def compute_model_output(body: ActivationRequest = Body(..., openapi_examples={
        f"example_{i}": {"summary": f"Example {i + 1}", "description": f"Example input and training data for case {i + 1}",
                         "value": {"model_id": "test", "input": ex}} for i, ex in enumerate(EXAMPLES)})):
    model_id = body.model_id
    log.info(f"Requesting output for model {model_id}")
    model = NeuralNetworkModel.deserialize(model_id)
    output, cost = model.compute_output(body.input.activation_vector, body.input.target_vector)
    return {"output_vector": output, "cost": cost}


# POST /predict/ keeps the models it served loaded: a small LRU by model id. Every request checks
# the entry against the checkpoint file's (mtime, size), so a checkpoint rewritten by a training
# (or a re-created model) is loaded again; DELETE /model/ evicts.
PREDICT_CACHE_SIZE = 4
_predict_cache: "OrderedDict[str, tuple]" = OrderedDict()
_predict_cache_lock = threading.Lock()


def _evict_cached_model(model_id: str) -> None:
    with _predict_cache_lock:
        _predict_cache.pop(model_id, None)


def _cached_model(model_id: str) -> NeuralNetworkModel:
    try:
        st = os.stat(ckpt.model_path(model_id))
    except FileNotFoundError:
        _evict_cached_model(model_id)
        raise KeyError(f"Model {model_id} not created yet.")
    stamp = (st.st_mtime_ns, st.st_size)
    with _predict_cache_lock:
        entry = _predict_cache.get(model_id)
        if entry is not None and entry[0] == stamp:
            _predict_cache.move_to_end(model_id)
            return entry[1]
    model = NeuralNetworkModel.deserialize(model_id)  # (stamp taken first: a later rewrite reloads again)
    with _predict_cache_lock:
        _predict_cache[model_id] = (stamp, model)
        _predict_cache.move_to_end(model_id)
        while len(_predict_cache) > PREDICT_CACHE_SIZE:
            _predict_cache.popitem(last=False)
    return model


def _check_predict_inputs(model: NeuralNetworkModel, inputs: list) -> None:
    """1-D or 2-D, rectangular, and as wide as the model's first linear layer (ValueError -> 400)."""
    if not inputs:
        raise ValueError("inputs must not be empty")
    batch = isinstance(inputs[0], list)
    rows = inputs if batch else [inputs]
    if any(not isinstance(r, list) for r in rows) or any(isinstance(v, list) for v in rows[0]):
        raise ValueError("inputs must be one vector (1D) or a batch of vectors (2D)")
    width = len(rows[0])
    if width == 0 or any(len(r) != width for r in rows):
        raise ValueError("every input row must have the same, non-zero length")
    first = next((layer for layer in model.layers if layer.weights is not None), None)
    if first is not None and first.algo == "linear" and width != first.weights.shape[0]:
        raise ValueError(f"model {model.model_id} takes {first.weights.shape[0]} inputs per row, got {width}")


PREDICT_EXAMPLES = {
    "single": {"summary": "One vector", "description": "One 9-cell board; the response holds one output vector.",
               "value": {"model_id": "test", "inputs": EXAMPLES[2]["activation_vector"]}},
    "batch": {"summary": "A batch", "description": "Three boards in one request; one output vector per row.",
              "value": {"model_id": "test", "inputs": [ex["activation_vector"] for ex in EXAMPLES[:3]]}},
}


@app.post("/predict/")
def predict_model_output(body: PredictRequest = Body(..., openapi_examples=PREDICT_EXAMPLES)):
    model_id = body.model_id
    log.info(f"Requesting prediction for model {model_id}")
    model = _cached_model(model_id)
    _check_predict_inputs(model, body.inputs)
    try:
        if body.weights is None:
            return {"output_vectors": model.predict(body.inputs)}
        return {"output_vectors": model.predict(body.inputs, weights=body.weights)}
    except IndexError as e:  # an embedding id outside the vocabulary is a bad request
        raise ValueError(str(e))


CLASSIFY_EXAMPLES = {
    "single": {"summary": "One vector", "description": "One 9-cell board of a softmax-head model; the three most likely "
                                                       "moves and their probabilities.",
               "value": {"model_id": "test", "inputs": EXAMPLES[2]["activation_vector"], "top_k": 3}},
    "batch": {"summary": "A batch", "description": "Three boards in one request; the most likely move of each.",
              "value": {"model_id": "test", "inputs": [ex["activation_vector"] for ex in EXAMPLES[:3]]}},
}


@app.post("/classify/")
def classify_inputs(body: ClassifyRequest = Body(..., openapi_examples=CLASSIFY_EXAMPLES)):
    model_id = body.model_id
    log.info(f"Requesting classification for model {model_id}")
    model = _cached_model(model_id)
    _check_predict_inputs(model, body.inputs)
    try:
        if body.weights is None:
            return model.classify(body.inputs, top_k=body.top_k)
        return model.classify(body.inputs, top_k=body.top_k, weights=body.weights)
    except IndexError as e:  # an embedding id outside the vocabulary is a bad request
        raise ValueError(str(e))


GENERATE_EXAMPLES = {
    "single": {"summary": "One context", "description": "Ten tokens after one context of a character model "
                                                        "(vocabulary 27, id 0 ends a word).",
               "value": {"model_id": "names", "context": [0, 0, 5], "max_new_tokens": 10, "stop_token": 0}},
    "batch": {"summary": "A batch, reproducible", "description": "Two rows of different lengths (the short one is "
                                                                  "left-padded), top-k sampling with a fixed seed.",
              "value": {"model_id": "names", "context": [[13], [1, 14, 14, 1]], "max_new_tokens": 8, "temperature": 0.8,
                        "top_k": 5, "seed": 1234, "stop_token": 0}},
}


@app.post("/generate/")
def generate_tokens(body: GenerateRequest = Body(..., openapi_examples=GENERATE_EXAMPLES)):
    model_id = body.model_id
    log.info(f"Requesting generation for model {model_id}")
    model = _cached_model(model_id)
    # (only when asked for, as weights on /predict/)
    extra = {**({} if body.loop is None else {"loop": body.loop}), **nucleus_args(body.top_p, body.min_p),
             **({} if body.logprobs is None else {"logprobs": body.logprobs}),
             **({} if body.top_logprobs is None else {"top_logprobs": body.top_logprobs})}
    try:
        return model.generate(body.context, body.max_new_tokens, temperature=body.temperature, top_k=body.top_k,
                              seed=body.seed, stop_token=body.stop_token, pad_token=body.pad_token, weights=body.weights,
                              **extra)
    except IndexError as e:  # a context id outside the vocabulary is a bad request
        raise ValueError(str(e))


SCORE_MAX_IDS = 1 << 20  # scored ids per POST /score/ request
SCORE_EXAMPLES = {
    "single": {"summary": "One sequence", "description": "A word of a character model (vocabulary 27, id 0 ends a word): "
                                                         "the log-probability and the rank of each of its ids, and the "
                                                         "word's perplexity.",
               "value": {"model_id": "names", "sequences": [5, 13, 13, 1, 0]}},
    "batch": {"summary": "Held-out text, scalars only", "description": "Rows of different lengths in one request; only the "
                                                                       "id count, mean negative log-probability, perplexity "
                                                                       "and top-1 share come back.",
              "value": {"model_id": "names", "sequences": [[5, 13, 13, 1, 0], [1, 22, 1, 0]], "details": False}},
}


@app.post("/score/")
def score_sequences(body: ScoreRequest = Body(..., openapi_examples=SCORE_EXAMPLES)):
    model_id = body.model_id
    log.info(f"Requesting scores for model {model_id}")
    rows = body.sequences if body.sequences and isinstance(body.sequences[0], list) else [body.sequences]
    if sum(len(row) for row in rows if isinstance(row, list)) > SCORE_MAX_IDS:
        raise ValueError(f"a request scores at most {SCORE_MAX_IDS} ids")
    model = _cached_model(model_id)
    try:
        extra = {} if body.top_logprobs is None else {"top_logprobs": body.top_logprobs}  # (only when asked for)
        return model.score(body.sequences, pad_token=body.pad_token, weights=body.weights, details=body.details, **extra)
    except IndexError as e:  # an id that is no class of the model is a bad request
        raise ValueError(str(e))


# active training sessions by model id (one event loop, so a plain dict is safe), and the ids
# whose PUT /train/ is still loading the checkpoint (between the 409 check and the task start)
model_locks: Dict[str, Lock] = {}
_starting: set = set()


def _log_task_failure(task) -> None:
    if not task.cancelled() and task.exception() is not None:
        log.error(f"Background training failed: {task.exception()!r}")


@app.put("/train/")
async def train_model(body: TrainingRequest = Body(...)):
    model_id = body.model_id
    log.info(f"Requesting training for model {model_id}")
    lock = model_locks.setdefault(model_id, Lock())
    if lock.locked() or model_id in _starting:
        raise HTTPException(status_code=409, detail=f"Training already in progress for model {model_id}.")
    # the checkpoint loads OFF the event loop (seconds for a 25 M-1 B parameter model; the
    # reference parses it on the loop, main.py:270, and every /progress/ poll stalls meanwhile)
    _starting.add(model_id)
    try:
        model = await run_in_threadpool(NeuralNetworkModel.deserialize, model_id)
        data = [(item.activation_vector, item.target_vector) for item in body.training_data]
        hp = dict(epochs=body.epochs, learning_rate=body.learning_rate, batch_size=body.batch_size,
                  decay_rate=body.decay_rate, dropout_rate=body.dropout_rate, l2_lambda=body.l2_lambda,
                  beta1=body.adam_beta1, beta2=body.adam_beta2, epsilon=body.adam_epsilon)

        async def train():
            try:
                async with lock:
                    _starting.discard(model_id)  # the lock now says "in progress"
                    # one thread trains; with a multi-GPU train group up, a GPU model trains on every rank
                    await run_in_threadpool(service.train, model, data, hp)
            finally:
                _starting.discard(model_id)

        def _done(task) -> None:
            if task.cancelled():  # cancelled before its first step: its body (and finally) never ran
                _starting.discard(model_id)
            _log_task_failure(task)

        create_task(train()).add_done_callback(_done)
    except BaseException:
        # anything before the task exists (load, request unpacking, task creation) must not leave
        # the id marked as starting: every later PUT /train/ would answer 409
        _starting.discard(model_id)
        raise
    return JSONResponse(content={"message": f"Training for model {model_id} started asynchronously."},
                        status_code=202)


@app.get("/progress/")
def model_progress(model_id: str = ModelIdQuery(...)):
    log.info(f"Requesting progress for model {model_id}")
    model = NeuralNetworkModel.deserialize(model_id, meta_only=True)  # no parameters, no GPU
    return {"progress": model.progress, "average_cost": model.avg_cost,
            "average_cost_history": model.avg_cost_history, "status": model.status}


@app.get("/stats/")
def model_stats(model_id: str = ModelIdQuery(...)):
    log.info(f"Requesting stats for model {model_id}")
    return NeuralNetworkModel.deserialize(model_id, meta_only=True).stats


@app.delete("/model/")
def delete_model(model_id: str = ModelIdQuery(...)):
    log.info(f"Requesting deletion of model {model_id}")
    NeuralNetworkModel.delete(model_id)
    _evict_cached_model(model_id)
    return Response(status_code=204)


def _uvicorn_log_config() -> dict:
    handler = {"level": "INFO", "class": "logging.StreamHandler", "formatter": "default"}
    quiet = {"level": "INFO", "handlers": ["default"], "propagate": False}
    return {
        "version": 1,
        "disable_existing_loggers": False,
        "formatters": {"default": {"format": LOG_FORMAT, "datefmt": DATE_FORMAT}},
        "handlers": {"default": handler},
        "loggers": {"uvicorn": quiet, "uvicorn.error": dict(quiet), "uvicorn.access": dict(quiet)},
        "root": {"level": "INFO", "handlers": ["default"]},
    }


if __name__ == "__main__":  # pragma: no cover
    import uvicorn

    uvicorn.run(app, host=os.environ.get("PZ_HOST", "127.0.0.1"), port=int(os.environ.get("PZ_PORT", "8000")),
                log_config=_uvicorn_log_config())
