"""``NeuralNetworkModel`` — model lifecycle, training, persistence, diagnostics (reference L4/L5,
``neural_net_model.py:269-585``).

Public API, attributes, checkpoint format and training semantics are the reference's. What a
model runs on is chosen at construction (new optional ``dtype`` / ``device`` arguments):

* default (``float64`` on the CPU): the reference algorithm on ATen, op for op. Seeded runs are
  bit-identical to the reference (tested), which keeps its 65-case test suite green.
* ``device="cuda"`` (any precision): parameters move into one flat device buffer
  (:class:`..engine.params.ParamStore`; layers hold views). ``train`` runs the device-resident
  fused engine (:class:`..engine.trainer.FusedTrainer`: MFMA GEMMs with fused epilogues, fused
  optimizer, on-device sampling, no host syncs between epochs, data parallel over RCCL when a
  process group is up). ``compute_output`` / ``_forward`` run the HIP kernels under autograd.
  Architectures the fused engine cannot schedule train through the same HIP kernels under
  autograd instead.

Fixes of reference defects: a zero sample size is clamped to 1; a training that
raises persists ``status == "Failed"`` instead of staying ``"Training"`` forever; checkpoints are
replaced atomically; periodic checkpoints of long trainings are written by a background thread.
"""
from __future__ import annotations

import logging
import math
import random
import time
from datetime import datetime
from typing import Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from ..config import Precision, resolve_device, resolve_precision
from ..utils import checkpoint as ckpt
from ..utils.stats import build_stats
from .mlp import MultiLayerPerceptron

log = logging.getLogger("neural_net_model")

CHECKPOINT_INTERVAL_S = 10.0   # reference neural_net_model.py:488
MAX_PROGRESS_POINTS = 100      # reference :504


class _SaveAgreement:
    """Data parallel fused training: every rank must take the SAME record / checkpoint steps — a
    record step issues its collectives in another order (no paired dW launch, all-reduced instead
    of reduce-scattered buckets, the sharded optimizer's state gathers), so ranks whose 10 s
    wall clocks disagree would pair mismatched collectives. Each rank's "10 s since the last save"
    flag is summed over the ranks asynchronously; the step ``LAG`` epochs later acts on that
    agreed value. The sum is read through pinned memory behind an event on a side stream: the
    host waits for a two-step-old collective, never for the compute stream."""
    LAG = 2

    def __init__(self, ctx, device: torch.device):
        self.ctx, self.device = ctx, device
        self.side = torch.cuda.Stream(device=device) if device.type == "cuda" else None
        self.queue: list = []
        self.skip = 0

    def decide(self, flag: bool) -> bool:
        t = torch.tensor([1.0 if flag else 0.0], dtype=torch.float64, device=self.device)
        h = self.ctx.all_reduce_async(t, exact=True)
        if self.side is not None:
            host = torch.empty(1, dtype=torch.float64, pin_memory=True)
            self.side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self.side):
                self.ctx.wait_one(h)
                host.copy_(t, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.side)
            t.record_stream(self.side)
            self.queue.append((ev, host))
        else:
            self.ctx.wait_one(h)
            self.queue.append((None, t))
        if len(self.queue) <= self.LAG:
            return False
        ev, host = self.queue.pop(0)
        if ev is not None:
            ev.synchronize()
        agreed = host.item() > 0.0
        if self.skip:  # (flags raised before the last agreed save)
            self.skip -= 1
            return False
        if agreed:
            self.skip = self.LAG
        return agreed
MAX_COST_HISTORY = 100         # reference :539


def _effective_device(device) -> torch.device:
    dev = resolve_device(device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        log.warning(f"device {dev} requested but no GPU is available; keeping the model on the CPU")
        return torch.device("cpu")
    return dev


class ModelMeta:
    """Checkpoint metadata under the attribute names of :class:`NeuralNetworkModel`."""

    def __init__(self, model_id: str, meta: dict):
        self.model_id = model_id
        self.algos = meta.get("algos")
        self.progress = meta.get("progress", [])
        self.avg_cost = meta.get("average_cost")
        self.avg_cost_history = meta.get("average_cost_history", [])
        self.stats = meta.get("stats")
        self.status = meta.get("status")
        self.runtime = meta.get("runtime")


class NeuralNetworkModel(MultiLayerPerceptron):
    def __init__(self, model_id, layer_sizes: list[int] = None, weight_algo="xavier", bias_algo="zeros",
                 activation_algos=None, optimizer_algo="adam", batchnorm=(1e-5, 0.1), confidence=1.0,
                 dtype=None, device=None):
        super().__init__(layer_sizes or [], weight_algo, bias_algo, activation_algos, batchnorm)
        self.model_id = model_id
        self.precision: Precision = resolve_precision(dtype)
        self.device = _effective_device(device)
        self._param_store = None
        self._predictor = None  # lazily built FusedPredictor (False: this model has none); see predict
        self.optimizer: torch.optim.Optimizer | None = None
        if self.params:
            if self.weights:
                self.weights[-1] *= confidence
            self._place()
            if optimizer_algo == "adam":
                self.optimizer = torch.optim.Adam(self.params)
        self.progress = []
        self.training_data_buffer: list = []
        self.training_buffer_size: int = self.num_params
        self.avg_cost = None
        self.avg_cost_history = []
        self.stats = None
        self.status = "Created"
        # data-parallel group this model trains in (None: the process-wide context); set by the
        # REST service's multi-GPU train group (parallel/service.py) around ``train``
        self._context = None

    # ------------------------------------------------------------------------------------
    # placement
    # ------------------------------------------------------------------------------------
    @property
    def is_reference_runtime(self) -> bool:
        """fp64 on the CPU: the reference's own runtime (and checkpoint without a runtime key)."""
        return self.device.type == "cpu" and self.precision.name == "float64"

    @property
    def on_gpu(self) -> bool:
        return self.device.type == "cuda"

    def _place(self) -> None:
        """Move the (fp64, CPU) parameters into one flat buffer on the model's device/precision."""
        self._predictor = None  # its weight copies belong to the previous placement
        if self.is_reference_runtime or not self.params:
            self._param_store = None
            return
        from ..engine.params import ParamStore
        self._param_store = ParamStore.adopt(self.layers, self.device, self.precision.master)

    @property
    def weights(self) -> list[Tensor]:
        return [layer.weights for layer in self.layers if layer.weights is not None]

    @property
    def num_params(self) -> int:
        return sum(p.numel() for p in self.params)

    # ------------------------------------------------------------------------------------
    # persistence (reference :306-369)
    # ------------------------------------------------------------------------------------
    def _runtime_entry(self) -> dict | None:
        if self.is_reference_runtime:
            return None
        return {"dtype": self.precision.name, "device": self.device.type}

    def _model_data(self, layer_states: list) -> dict:
        data = {
            "algos": self.algos,
            "layers": layer_states,
            "progress": self.progress,
            "training_data_buffer": self.training_data_buffer,
            "average_cost": self.avg_cost,
            "average_cost_history": self.avg_cost_history,
            "stats": self.stats,
            "status": self.status,
        }
        runtime = self._runtime_entry()
        if runtime is not None:  # optional key; the reference ignores unknown keys on load
            data["runtime"] = runtime
        return data

    def get_model_data(self) -> dict:
        return self._model_data([layer.state_dict for layer in self.layers])

    def _checkpoint_skeleton(self) -> dict:
        """``get_model_data`` with parameter tensors left as tensors (rendered natively)."""
        return self._model_data([layer.checkpoint_state(ckpt.TensorRef) for layer in self.layers])

    def set_model_data(self, model_data: dict):
        for layer, state in zip(self.layers, model_data["layers"]):
            layer.state_dict = state
        self._place()
        self.progress = model_data["progress"]
        self.training_data_buffer = model_data["training_data_buffer"]
        self.training_buffer_size = self.num_params
        self.avg_cost = model_data["average_cost"]
        self.avg_cost_history = model_data["average_cost_history"]
        self.stats = model_data["stats"]
        self.status = model_data["status"]

    def _optimizer_state(self) -> dict | None:
        return self.optimizer.state_dict() if self.optimizer is not None else None

    def _dp_context(self):
        from ..parallel.dist import get_context
        return self._context if self._context is not None else get_context()

    def _is_writer(self) -> bool:
        """Under data parallelism every rank holds the same model; rank 0 owns the files."""
        return self._dp_context().rank == 0

    def serialize(self):
        if not self._is_writer():
            return
        ckpt.wait_pending(self.model_id)  # a background snapshot must not land after this write
        ckpt.save(self.model_id, self._checkpoint_skeleton(), self._optimizer_state())

    def serialize_background(self) -> bool:
        """Snapshot now, write on a background thread; False if the previous write is still running."""
        if not self._is_writer() or ckpt.pending(self.model_id):
            return False
        skeleton, opt_state = ckpt.snapshot(self._checkpoint_skeleton(), self._optimizer_state())
        ckpt.save_async(self.model_id, skeleton, opt_state)
        return True

    @classmethod
    def deserialize(cls, model_id: str, meta_only: bool = False):
        """Load a model. ``meta_only=True`` (the REST ``/progress/`` / ``/stats/`` polls; the
        reference deserialises the whole model for each, ``main.py:303-318``): a :class:`ModelMeta`
        with the progress / cost / status / stats attributes only — no parameter is parsed and
        nothing is placed on a GPU."""
        if meta_only:
            try:
                return ModelMeta(model_id, ckpt.load_meta(model_id))
            except FileNotFoundError as e:
                log.error(f"File not found error occurred: {str(e)}")
                raise KeyError(f"Model {model_id} not created yet.")
        try:
            model_data, opt_state = ckpt.load(model_id)
        except FileNotFoundError as e:
            log.error(f"File not found error occurred: {str(e)}")
            raise KeyError(f"Model {model_id} not created yet.")
        runtime = model_data.get("runtime") or {}
        model = cls(model_id, activation_algos=model_data["algos"], dtype=runtime.get("dtype"),
                    device=runtime.get("device"))
        model.set_model_data(model_data)
        if opt_state is not None:
            model.optimizer = torch.optim.Adam(model.params)
            model.optimizer.load_state_dict(opt_state)
        return model

    @classmethod
    def delete(cls, model_id: str):
        try:
            ckpt.delete(model_id)
        except FileNotFoundError as e:
            log.warning(f"Failed to delete: {str(e)}")

    # ------------------------------------------------------------------------------------
    # inference / forward (reference :371-408)
    # ------------------------------------------------------------------------------------
    @property
    def _activation_dtype(self) -> torch.dtype:
        """dtype of activations on the GPU autograd path (GEMM operand precision)."""
        if self.precision.name in ("bfloat16", "fp8"):
            return torch.bfloat16
        return self.precision.master

    def _input_tensor(self, data) -> Tensor:
        if self.is_reference_runtime or not self.on_gpu:
            return torch.tensor(data, dtype=self.precision.master if not self.is_reference_runtime else torch.float64)
        return torch.tensor(data, dtype=self.precision.master).to(self.device)

    def compute_output(self, input_data: list, target: list = None) -> Tuple[list, float]:
        activations, cost = self._forward(self._input_tensor(input_data), target)
        out = activations[-1].detach()
        if out.dtype == torch.bfloat16:
            out = out.float()
        return out.tolist(), cost.item() if cost.numel() > 0 else None

    def predict(self, input_data: list, weights: str | None = None) -> list:
        """Outputs only, forward-only: what ``compute_output(input_data)[0]`` returns, without a
        cost or a target, layers in eval mode, nothing recorded for autograd.

        GPU models run the fused forward schedule of :class:`..engine.predictor.FusedPredictor`
        (GEMM-dtype weight copies made once, the skinny-batch GEMM below 64 rows, fused bias /
        activation epilogues); it is built on first use and dropped whenever the parameters may
        have changed (``train``, ``set_model_data``, re-placement), so it never serves stale
        weights. Models it cannot schedule (``float64``, unusual layer orders), CPU models and the
        reference runtime run the layer loop under ``no_grad`` — there the result is bit-identical
        to ``compute_output``'s.

        ``weights="fp8"`` opts into weight-only quantised inference: the linear layers read OCP
        e4m3 copies of the weights with one power-of-two scale per output column (activations stay
        bf16, accumulation fp32; see :mod:`..engine.predictor`). Only GPU models whose compute
        dtype is bf16 (``bfloat16`` / ``fp8``) and which the fused predictor can schedule take it;
        anything else raises ``ValueError`` — there is no silent fall-back to unquantised weights.
        ``None`` is the model's own precision."""
        if weights is not None:
            if weights != "fp8":
                raise ValueError(f"unknown weights {weights!r}: None (the model's own precision) or 'fp8'")
            if not self.on_gpu:
                raise ValueError("weights='fp8' needs a model on a GPU (the e4m3 kernels are HIP kernels)")
        x = self._input_tensor(input_data)
        with torch.no_grad():
            predictor = self._fused_predictor() if self.on_gpu else None
            if weights is not None and predictor is None:
                raise ValueError(f"weights='fp8' is not available for model {self.model_id}: "
                                 f"{getattr(self, '_predictor_reason', 'no fused predictor')}")
            if predictor is not None:
                for layer in self.layers:
                    layer.training = False
                out = predictor.forward(x, weights=weights) if weights is not None else predictor.forward(x)
            else:
                out = self._forward(x, None)[0][-1].detach()
                if out.dtype == torch.bfloat16:
                    out = out.float()
        return out.tolist()

    def classify(self, input_data: list, top_k: int = 1, weights: str | None = None) -> dict:
        """The ``top_k`` most likely classes of a softmax-head model and how sure it is of them:
        ``{"classes": [...], "probabilities": [...]}`` in rank order (descending probability, equal logits in
        ascending class order: the rule of :func:`..ops.functional.topk_rows_reference`). ``input_data`` as in
        :meth:`predict`: a vector gives one flat list each, a batch one list per row.

        GPU models with a fused predictor run :meth:`..engine.predictor.FusedPredictor.classify`: the
        forward kernels and one selection launch on the logits; the softmax row is never formed, and only
        ``[rows, top_k]`` numbers are downloaded. CPU models, the reference runtime and models without a
        predictor run the layers in eval mode under ``no_grad`` and the pure-torch rule on the softmax
        layer's input. ``weights="fp8"`` as in :meth:`predict`. ``ValueError`` for another head and for a
        ``top_k`` that is no integer in ``[1, min(classes, 64)]``."""
        from ..ops import functional as PF
        if weights is not None:
            if weights != "fp8":
                raise ValueError(f"unknown weights {weights!r}: None (the model's own precision) or 'fp8'")
            if not self.on_gpu:
                raise ValueError("weights='fp8' needs a model on a GPU (the e4m3 kernels are HIP kernels)")
        if not self.algos or self.algos[-1] != "softmax":
            raise ValueError(f"model {self.model_id} cannot classify: top-k classes need a softmax head")
        if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1:
            raise ValueError(f"top_k must be an integer >= 1, got {top_k!r}")
        x = self._input_tensor(input_data)
        with torch.no_grad():
            predictor = self._fused_predictor() if self.on_gpu else None
            if weights is not None and predictor is None:
                raise ValueError(f"weights='fp8' is not available for model {self.model_id}: "
                                 f"{getattr(self, '_predictor_reason', 'no fused predictor')}")
            for layer in self.layers:
                layer.training = False
            single = self._output_is_vector(x)
            if predictor is not None:
                idx, logprob = (predictor.classify(x, top_k, weights=weights) if weights is not None
                                else predictor.classify(x, top_k))
            else:
                logits = self._forward(x, None)[0][-2].detach()  # the softmax layer's input
                idx, logprob = PF.topk_rows_reference(logits, PF.check_topk(top_k, logits.shape[-1], "top_k"))
            # one download: the classes (exact in fp64) next to their probabilities, exp of the fp64 image
            both = torch.empty(2, *idx.shape, device=idx.device, dtype=torch.float64)
            both[0].copy_(idx)
            both[1].copy_(logprob)
            both[1].exp_()
            both = both.tolist()
        classes = [[int(c) for c in row] for row in both[0]]
        return {"classes": classes[0] if single else classes, "probabilities": both[1][0] if single else both[1]}

    def _output_is_vector(self, x: Tensor) -> bool:
        """Whether this input is one row without a batch dimension (a vector, or one id row whose positions
        the flatten layers merge into one), by the dimensions the layers give it. (Not by the output's: the
        CPU batchnorm's running statistics keep a leading 1 after a training step.)"""
        shape = list(x.shape)
        for layer in self.layers:
            if layer.algo == "embedding":
                shape.append(1)
            elif layer.algo == "flatten" and len(shape) > 1:
                shape[-2] //= int(layer.ratio)
                if shape[-2] == 1:
                    del shape[-2]
        return len(shape) == 1

    def _fused_predictor(self):
        if self._predictor is None:
            from ..engine.predictor import FusedPredictor, UnsupportedModel
            try:
                self._predictor = FusedPredictor(self)
            except UnsupportedModel as e:
                log.info(f"Model {self.model_id}: fused predictor unavailable ({e}); predicting through the layers")
                self._predictor = False
                self._predictor_reason = str(e)
        return self._predictor or None

    # ------------------------------------------------------------------------------------
    # token generation
    # ------------------------------------------------------------------------------------
    @property
    def context_length(self) -> int:
        """Ids per row of a next-token model (embedding -> flatten ... -> softmax): the product of
        the flatten ratios."""
        length = 1
        for layer in self.layers:
            if layer.algo == "flatten":
                length *= int(layer.ratio)
        return length

    def _generation_shape(self) -> tuple[int, int]:
        """(embedding rows, output classes) of a model that can generate; ValueError with the reason."""
        if not self.algos or self.algos[0] != "embedding" or self.layers[0].weights is None:
            raise ValueError(f"model {self.model_id} cannot generate: token generation needs an embedding first layer")
        if self.algos[-1] != "softmax":
            raise ValueError(f"model {self.model_id} cannot generate: token generation needs a softmax head")
        widths = [layer.weights.shape[1] for layer in self.layers[1:] if layer.algo == "linear" and layer.weights is not None]
        if not widths:
            raise ValueError(f"model {self.model_id} cannot generate: no linear layer produces the logits")
        vocab, classes = int(self.layers[0].weights.shape[0]), int(widths[-1])
        if classes > vocab:
            raise ValueError(f"model {self.model_id} cannot generate: it predicts {classes} classes but embeds {vocab} "
                             "ids, so a sampled id could not be fed back")
        return vocab, classes

    def generate(self, context: list, max_new_tokens: int, temperature: float = 1.0, top_k: int | None = None,
                 seed: int | None = None, stop_token: int | None = None, pad_token: int = 0,
                 weights: str | None = None, loop: str | None = None, top_p: float | None = None,
                 min_p: float | None = None, logprobs: bool = False, top_logprobs: int | None = None) -> dict:
        """Sample ``max_new_tokens`` ids after ``context`` from a next-token model (embedding first,
        softmax head): ``{"tokens": [[...], ...], "seed": int}``, one row per context row.

        ``context`` is one id list or a batch of lists; a row shorter than :attr:`context_length`
        is left-padded with ``pad_token``, a longer one contributes its last ``context_length`` ids.
        Each step feeds the last ``context_length`` ids, takes the logits and draws by the rule of
        :func:`..ops.functional.sample_rows_reference`: ``temperature == 0`` is greedy, ``top_k``
        keeps the k largest logits (ties included), ``min_p`` drops what is less than ``min_p`` times as
        likely as the most likely token, ``top_p`` keeps the smallest set of most likely tokens that holds
        ``top_p`` of the remaining mass (nucleus sampling; ties with the last one stay), and row ``r`` draws
        ``PF.sample_uniform((seed & 0xFFFFFFFF, seed >> 32), r, step)`` at step ``step`` — so a seed
        names its output; ``seed=None`` takes 64 bits from ``os.urandom`` and returns them. A row is
        cut after its first ``stop_token`` (inclusive).

        GPU models with a fused predictor keep the whole loop on the device
        (:meth:`..engine.predictor.FusedPredictor.generate`: the forward kernels plus one sampling
        launch per token, one download at the end). CPU models, the reference runtime and models
        without a predictor run the layer loop under ``no_grad`` with the same rule and the same
        random numbers. ``weights="fp8"`` as in :meth:`predict`.

        ``loop="resident"`` opts into the one-launch form
        (:meth:`..engine.predictor.FusedPredictor.generate_resident`): the model's parameters are
        copied into every row's workgroup LDS and the token loop runs inside one kernel. It needs a GPU
        model with a fused predictor whose parameters fit (160 KiB of LDS, at most 8192 classes);
        anything else raises ``ValueError`` with the reason — there is no silent fall-back to the
        per-token loop. ``None`` is the per-token loop.

        ``logprobs=True`` adds ``"logprobs"``: for every returned token its log-probability under the
        model's own distribution — temperature 1 and no truncation, whatever ``temperature``, ``top_k``,
        ``top_p`` and ``min_p`` drew it with (a token that top-k sampling drew has the probability the
        whole vocabulary leaves it). It is computed after the loop by one :meth:`score` pass over
        ``[context | tokens]`` (one batched forward, with the loop's ``weights``), and cut after
        ``stop_token`` as the tokens are. Unset, nothing is computed and the key is absent.

        ``top_logprobs=k`` (an integer in ``[1, min(classes, 64)]``, with or without ``logprobs``) adds
        ``"top_tokens"`` and ``"top_logprobs"`` from the same pass: for every returned token the ``k`` classes
        the model found most likely at that position, in rank order, and their log-probabilities
        (:func:`..ops.functional.topk_rows_reference`), cut as the tokens are."""
        from ..ops import functional as PF
        if not isinstance(logprobs, bool):
            raise ValueError(f"logprobs must be a boolean, got {logprobs!r}")
        if loop is not None:
            if loop != "resident":
                raise ValueError(f"unknown loop {loop!r}: None (one sampling launch per token) or 'resident'")
            if not self.on_gpu:
                raise ValueError("loop='resident' needs a model on a GPU (the resident loop is a HIP kernel)")
        if weights is not None:
            if weights != "fp8":
                raise ValueError(f"unknown weights {weights!r}: None (the model's own precision) or 'fp8'")
            if not self.on_gpu:
                raise ValueError("weights='fp8' needs a model on a GPU (the e4m3 kernels are HIP kernels)")
        vocab, classes = self._generation_shape()
        if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or not 1 <= max_new_tokens <= 4096:
            raise ValueError(f"max_new_tokens must be an integer in [1, 4096], got {max_new_tokens!r}")
        if not isinstance(temperature, (int, float)) or temperature != temperature or temperature < 0:
            raise ValueError(f"temperature must be >= 0, got {temperature!r}")
        if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1):
            raise ValueError(f"top_k must be an integer >= 1, got {top_k!r}")
        if top_p is not None and (isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0 < top_p <= 1):
            raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
        if min_p is not None and (isinstance(min_p, bool) or not isinstance(min_p, (int, float)) or not 0 <= min_p < 1):
            raise ValueError(f"min_p must be in [0, 1), got {min_p!r}")
        extra = PF.nucleus_args(top_p, min_p)  # (only when set, as loop)
        if top_logprobs is not None:
            PF.check_topk(top_logprobs, classes, "top_logprobs")
        if stop_token is not None and (not isinstance(stop_token, int) or not 0 <= stop_token < classes):
            raise ValueError(f"stop_token {stop_token!r} is outside the vocabulary of {classes}")
        if not isinstance(pad_token, int) or not 0 <= pad_token < vocab:
            raise ValueError(f"pad_token {pad_token!r} is outside the vocabulary of {vocab}")
        if seed is None:
            import os
            seed = int.from_bytes(os.urandom(8), "little")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        key = (seed & 0xFFFFFFFF, seed >> 32)
        if not isinstance(context, list) or not context:
            raise ValueError("context must be a non-empty id list or a non-empty batch of id lists")
        batch = context if isinstance(context[0], list) else [context]
        length = self.context_length
        window = []
        for row in batch:
            if not isinstance(row, list) or any(isinstance(v, bool) or not isinstance(v, int) for v in row):
                raise ValueError("context rows must be lists of integer ids")
            row = row[-length:]
            window.append([pad_token] * (length - len(row)) + row)
        ids = torch.tensor(window, dtype=torch.int64)
        PF.check_index_range(ids.reshape(-1), -vocab, vocab, "index", vocab)  # IndexError, as predict
        with torch.no_grad():
            predictor = self._fused_predictor() if self.on_gpu else None
            if weights is not None and predictor is None:
                raise ValueError(f"weights='fp8' is not available for model {self.model_id}: "
                                 f"{getattr(self, '_predictor_reason', 'no fused predictor')}")
            if loop is not None:
                reason = (getattr(self, "_predictor_reason", "no fused predictor") if predictor is None
                          else predictor.resident_plan())
                if isinstance(reason, str):
                    raise ValueError(f"loop='resident' is not available for model {self.model_id}: {reason}")
            for layer in self.layers:
                layer.training = False
            if loop is not None:
                drawn = predictor.generate_resident(ids, max_new_tokens, temperature=float(temperature), top_k=top_k,
                                                    seed=key, stop_token=stop_token, weights=weights, **extra)
            elif predictor is not None:
                drawn = predictor.generate(ids, max_new_tokens, temperature=float(temperature), top_k=top_k, seed=key,
                                           stop_token=stop_token, weights=weights, **extra)
            else:
                drawn = self._generate_layers(ids, max_new_tokens, float(temperature), top_k, key, stop_token, **extra)
            tokens = drawn.tolist() if isinstance(drawn, Tensor) else drawn
            scores = tops = None
            if logprobs or top_logprobs is not None:  # one batched forward on [context | tokens], after the loop
                full = torch.cat([ids.to(self.device), torch.as_tensor(drawn).to(self.device)], dim=1)
                more = {} if top_logprobs is None else {"top_logprobs": top_logprobs}
                if predictor is not None:
                    scored = predictor.score(full, weights=weights, **more)
                else:
                    scored = self._score_layers(full, **more)
                if logprobs:
                    scores = scored[0].tolist()
                if top_logprobs is not None:
                    tops = (scored[2].tolist(), scored[3].tolist())
        result = {"tokens": tokens, "seed": seed}
        if stop_token is not None:
            result["tokens"] = [row[:row.index(stop_token) + 1] if stop_token in row else row for row in tokens]
        if scores is not None:
            result["logprobs"] = [lp[:len(row)] for lp, row in zip(scores, result["tokens"])]
        if tops is not None:
            result["top_tokens"] = [t[:len(row)] for t, row in zip(tops[0], result["tokens"])]
            result["top_logprobs"] = [t[:len(row)] for t, row in zip(tops[1], result["tokens"])]
        return result

    def _generate_layers(self, ids: Tensor, steps: int, temperature: float, top_k, key, stop_token, **nucleus) -> list:
        """The generation loop through the layers (``_forward`` in eval mode) with the pure-torch sampler."""
        from ..ops import functional as PF
        rows, length = ids.shape
        seq = torch.cat([ids, torch.zeros(rows, steps, dtype=torch.int64)], dim=1).to(self.device)
        done = torch.zeros(rows, dtype=torch.bool, device=self.device)
        for s in range(steps):
            logits = self._forward(seq[:, s:s + length], None)[0][-2].detach()  # the softmax layer's input
            token = PF.sample_rows_reference(logits.reshape(rows, -1), key, s, temperature, top_k, **nucleus)
            if stop_token is not None:
                token = torch.where(done, torch.full_like(token, stop_token), token)
                done |= token == stop_token
            seq[:, length + s] = token
        return seq[:, length:].tolist()

    # ------------------------------------------------------------------------------------
    # sequence scoring
    # ------------------------------------------------------------------------------------
    SCORE_MAX_IDS = 1 << 24  # scored ids per call (the padded batch is one tensor on the device)
    SCORE_LAYERS_BYTES = 64 << 20  # _score_layers: the fp64 log-softmax of one chunk of windows stays within this

    def score(self, sequences: list, pad_token: int = 0, weights: str | None = None, details: bool = True,
              top_logprobs: int | None = None) -> dict:
        """How likely a next-token model (embedding first, softmax head) finds ``sequences``: one non-empty
        id list or a non-empty batch of non-empty lists. Every id of a row is scored given the
        :attr:`context_length` ids before it; a row is left-padded with ``pad_token``, the convention of
        :meth:`generate` for short contexts, so its first id is scored after a window of padding. Rows of
        different lengths are padded on the right and the padding is masked out.

        Returns ``{"tokens": n, "nll": ..., "perplexity": ..., "top1": ...}``: the number of scored ids, their
        mean negative log-probability (natural log; summed in fp64 where the model lives), its exponential,
        and the share of ids that were the model's most likely class (rank 0, ties to the lowest index: what
        greedy sampling picks). ``details=True`` adds ``"logprobs"`` and ``"ranks"``, one list per row, by the
        rule of :func:`..ops.functional.token_logprob_reference`; without it only the four scalars leave the
        device.

        GPU models with a fused predictor run :meth:`..engine.predictor.FusedPredictor.score` (batched
        forward kernels and one ``PF.token_logprob`` launch per chunk of windows). CPU models, the reference
        runtime and models without a predictor run the layer loop in eval mode under ``no_grad`` with the
        pure-torch rule. ``weights="fp8"`` as in :meth:`predict`. ``IndexError`` for an id that is not a
        class of the model.

        ``top_logprobs=k`` (an integer in ``[1, min(classes, 64)]``; needs ``details=True``) adds
        ``"top_tokens"`` and ``"top_logprobs"``: per row, for every scored id, the ``k`` classes the model found
        most likely there, in rank order, and their log-probabilities
        (:func:`..ops.functional.topk_rows_reference`; on the device one more ``PF.topk_rows`` launch per
        chunk). ``rows x longest x k`` stays within ``SCORE_MAX_IDS``."""
        from ..ops import functional as PF
        if weights is not None:
            if weights != "fp8":
                raise ValueError(f"unknown weights {weights!r}: None (the model's own precision) or 'fp8'")
            if not self.on_gpu:
                raise ValueError("weights='fp8' needs a model on a GPU (the e4m3 kernels are HIP kernels)")
        if not isinstance(details, bool):
            raise ValueError(f"details must be a boolean, got {details!r}")
        vocab, classes = self._generation_shape()
        if top_logprobs is not None:
            PF.check_topk(top_logprobs, classes, "top_logprobs")
            if not details:
                raise ValueError("top_logprobs needs details=True: the per-id lists are where it is reported")
        if isinstance(pad_token, bool) or not isinstance(pad_token, int) or not 0 <= pad_token < vocab:
            raise ValueError(f"pad_token {pad_token!r} is outside the vocabulary of {vocab}")
        if not isinstance(sequences, list) or not sequences:
            raise ValueError("sequences must be a non-empty id list or a non-empty batch of non-empty id lists")
        batch = sequences if isinstance(sequences[0], list) else [sequences]
        for row in batch:
            if not isinstance(row, list) or not row or any(isinstance(v, bool) or not isinstance(v, int) for v in row):
                raise ValueError("sequences rows must be non-empty lists of integer ids")
        lengths = [len(row) for row in batch]
        count, longest, length = sum(lengths), max(lengths), self.context_length
        if len(batch) * longest > self.SCORE_MAX_IDS:
            raise ValueError(f"too many ids to score in one call: {len(batch)} rows of up to {longest} "
                             f"(at most {self.SCORE_MAX_IDS} with the padding)")
        if top_logprobs is not None and len(batch) * longest * top_logprobs > self.SCORE_MAX_IDS:
            raise ValueError(f"too many top_logprobs in one call: {len(batch)} rows of up to {longest} ids, {top_logprobs} "
                             f"each (at most {self.SCORE_MAX_IDS} with the padding)")
        # [pad] * L, the row, then zeros (masked: any class would do) up to the longest row
        ids = torch.tensor([[pad_token] * length + row + [0] * (longest - len(row)) for row in batch], dtype=torch.int64)
        valid = torch.arange(longest).unsqueeze(0) < torch.tensor(lengths).unsqueeze(1)
        PF.check_index_range(ids[:, length:].reshape(-1), 0, classes, "Target")  # IndexError, as generate
        with torch.no_grad():
            predictor = self._fused_predictor() if self.on_gpu else None
            if weights is not None and predictor is None:
                raise ValueError(f"weights='fp8' is not available for model {self.model_id}: "
                                 f"{getattr(self, '_predictor_reason', 'no fused predictor')}")
            for layer in self.layers:
                layer.training = False
            more = {} if top_logprobs is None else {"top_logprobs": top_logprobs}
            if predictor is not None:
                logprob, rank, *tops = predictor.score(ids, weights=weights, **more)
            else:
                logprob, rank, *tops = self._score_layers(ids, **more)
            valid = valid.to(logprob.device)
            total = torch.where(valid, logprob.double(), torch.zeros((), dtype=torch.float64, device=logprob.device)).sum()
            first = ((rank == 0) & valid).sum().double()
            total, first = torch.stack([total, first]).tolist()  # the one download without details
            nll = -total / count
            result = {"tokens": count, "nll": nll, "perplexity": math.inf if nll >= 709 else math.exp(nll),  # (no OverflowError)
                      "top1": first / count}
            if details:
                result["logprobs"] = [row[:n] for row, n in zip(logprob.tolist(), lengths)]
                result["ranks"] = [row[:n] for row, n in zip(rank.tolist(), lengths)]
                if tops:
                    result["top_tokens"] = [row[:n] for row, n in zip(tops[0].tolist(), lengths)]
                    result["top_logprobs"] = [row[:n] for row, n in zip(tops[1].tolist(), lengths)]
        return result

    def _score_layers(self, ids: Tensor, top_logprobs: int | None = None) -> tuple:
        """The scorer through the layers (``_forward`` in eval mode) with the pure-torch rule: ``ids [R, L + n]``
        -> ``(fp64 logprob [R, n], int64 rank [R, n])`` of the columns from ``L`` on, in chunks of windows;
        with ``top_logprobs=k`` also ``(int64 top_idx [R, n, k], fp64 top_logprob [R, n, k])``."""
        from ..ops import functional as PF
        rows, length = ids.shape[0], self.context_length
        scored = ids.shape[1] - length
        ids = ids.to(self.device)
        windows = ids.unfold(1, length, 1)[:, :scored].reshape(rows * scored, length)
        targets = ids[:, length:].reshape(-1)
        classes = self._generation_shape()[1]
        chunk = max(1, self.SCORE_LAYERS_BYTES // (8 * classes))
        logprob, rank, top_idx, top_lp = [], [], [], []
        for i0 in range(0, rows * scored, chunk):
            logits = self._forward(windows[i0:i0 + chunk], None)[0][-2].detach()  # the softmax layer's input
            lp, rk = PF.token_logprob_reference(logits.reshape(-1, classes), targets[i0:i0 + chunk])
            logprob.append(lp)
            rank.append(rk)
            if top_logprobs is not None:
                ti, tl = PF.topk_rows_reference(logits.reshape(-1, classes), top_logprobs)
                top_idx.append(ti)
                top_lp.append(tl)
        out = (torch.cat(logprob).view(rows, scored), torch.cat(rank).view(rows, scored))
        if top_logprobs is not None:
            out += (torch.cat(top_idx).view(rows, scored, -1), torch.cat(top_lp).view(rows, scored, -1))
        return out

    def _forward(self, input_tensor: Tensor, target: list, dropout_rate=0.0) -> Tuple[list[Tensor], Tensor]:
        target_specified = target is not None and (isinstance(target, Tensor) or all(t is not None for t in target))
        gpu = self.on_gpu
        if gpu:
            from ..ops import functional as PF
            input_tensor = input_tensor.to(self.device)
            if self.algos[0] != "embedding":
                input_tensor = input_tensor.to(self._activation_dtype)
        outputs: list[Tensor] = []
        x = logits = input_tensor
        for layer in self.layers:
            layer.training = target_specified
            logits = x
            x = layer.forward(logits)
            if layer.hidden and layer.training:  # dropout on every hidden output (reference :393-395)
                x = PF.dropout(x, dropout_rate) if gpu else F.dropout(x, p=dropout_rate)
            outputs.append(x)

        if not target_specified:
            cost = torch.empty(0)
        elif self.algos[-1] == "softmax":  # CE on the softmax layer's input (reference :400-403)
            if isinstance(target, Tensor):  # programmatic use: class ids already as a tensor
                label_tensor = target.reshape(-1).to(torch.int64)
            else:
                labels = target[0] if logits.ndim == 1 else [t[0] for t in target]
                label_tensor = torch.tensor(labels, dtype=torch.int64)
            if gpu:
                cost = PF.cross_entropy(logits.to(self._loss_dtype), label_tensor.to(self.device))
            else:
                cost = F.cross_entropy(logits, label_tensor)
        else:
            target_tensor = torch.tensor(target, dtype=torch.float64)
            if gpu:
                cost = PF.mse_loss(x.to(self._loss_dtype), target_tensor.to(self.device, self._loss_dtype))
            else:
                cost = F.mse_loss(x, target_tensor.to(x.dtype) if x.dtype != torch.float64 else target_tensor)
        return outputs, cost

    @property
    def _loss_dtype(self) -> torch.dtype:
        return torch.float64 if self.precision.master == torch.float64 else torch.float32

    # ------------------------------------------------------------------------------------
    # training (reference :410-530)
    # ------------------------------------------------------------------------------------
    def train(self, training_data: list, epochs=100, learning_rate=0.01, batch_size=None, decay_rate=0.9,
              dropout_rate=0.2, l2_lambda=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.training_data_buffer.extend(training_data)
        if len(self.training_data_buffer) < self.training_buffer_size:
            log.info(f"Model {self.model_id}: Insufficient training data. "
                     f"Current buffer size: {len(self.training_data_buffer)}, "
                     f"required: {self.training_buffer_size}")
            self.serialize()  # keep the partial buffer for next time
            return

        data = self.training_data_buffer
        self.training_data_buffer = []
        epochs = max(0, int(epochs))
        # explicit, or an equal share per epoch; clamped (the reference crashes on 0 in mm)
        sample_size = max(1, batch_size or (int(len(data) / epochs) if epochs else len(data)))
        log.info(f"Training sample size: {sample_size}")

        if self.optimizer is not None:
            for group in self.optimizer.param_groups:
                group["betas"] = (beta1, beta2)
                group["eps"] = epsilon

        self.progress = []
        self.stats = None
        self.status = "Training"
        self.serialize()

        hp = dict(epochs=epochs, learning_rate=learning_rate, sample_size=sample_size, decay_rate=decay_rate,
                  dropout_rate=dropout_rate, l2_lambda=l2_lambda)
        self._predictor = None  # the masters change from here on: predict rebuilds its weight copies
        try:
            trainer = self._fused_trainer() if self.on_gpu else None
            if trainer is not None:
                try:
                    self._train_fused(trainer, data, **hp)
                except BaseException:
                    trainer.close(ok=False)  # no device sync on the failure path (engine/events.py)
                    raise
                trainer.close()
            else:
                self._train_autograd(data, **hp)
        except Exception:
            log.exception(f"Model {self.model_id}: training failed")
            self.status = "Failed"
            try:
                self.serialize()
            except Exception:  # pragma: no cover - keep the original error
                log.exception(f"Model {self.model_id}: could not persist the failed status")
            raise
        finally:
            self._predictor = None  # (a predict during the training built one on half-trained weights)

        self.status = "Trained"
        log.info(f"Model {self.model_id}: Done training for {epochs} epochs.")
        self.serialize()

    def _progress_point(self, when: str, epoch: int, cost: float, ratios: list[float] | None,
                        extra: dict | None = None) -> None:
        pending = list(ratios or [])
        point = {
            "dt": when,
            "epoch": epoch + 1,
            "cost": cost,
            "weight_upd_ratio": [pending.pop(0) if layer.weights is not None and pending else None
                                 for layer in self.layers],
        }
        if extra:  # optional telemetry of GPU runs; the dashboard ignores unknown keys
            point.update(extra)
        self.progress.append(point)

    def _train_autograd(self, data, epochs, learning_rate, sample_size, decay_rate, dropout_rate, l2_lambda,
                        context=None, sampler: torch.Generator | None = None):
        """The reference epoch loop (``neural_net_model.py:457-522``). On the CPU it is the
        reference's exact op / RNG sequence; GPU models run it on the HIP kernels.

        Data parallel (a process group is up, e.g. gloo for CPU models): replicas start from rank
        0's parameters, every rank draws the same global sample from a shared ``sampler`` seed and
        trains on its contiguous shard, and gradients are averaged with one all-reduce before the
        (identical) optimizer step — equivalent to one process training on the whole sample."""
        ctx = context or self._dp_context()
        world, rank = ctx.world_size, ctx.rank
        self._predictor = None
        from . import layers as _layers
        _layers.set_bn_sync(self.layers, ctx if world > 1 else None)  # synchronised batchnorm statistics
        try:
            self._autograd_epochs(data, epochs, learning_rate, sample_size, decay_rate, dropout_rate, l2_lambda,
                                  ctx, sampler)
        finally:
            _layers.set_bn_sync(self.layers, None)

    def _autograd_epochs(self, data, epochs, learning_rate, sample_size, decay_rate, dropout_rate, l2_lambda, ctx,
                         sampler):
        world, rank = ctx.world_size, ctx.rank
        if world > 1:
            dev = self.params[0].device if self.params else torch.device("cpu")
            with torch.no_grad():
                for p in self.params:
                    ctx.broadcast_(p.data)
            if sampler is None:
                seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).to(dev)
                ctx.broadcast_(seed)
                sampler = torch.Generator().manual_seed(int(seed.item()))
        if sample_size < world:
            raise ValueError(f"sample size {sample_size} is smaller than the {world} data-parallel ranks")
        # contiguous shards of the global sample; the sample_size % world extra rows are spread by the
        # floor division (S=10, W=4: shards 2, 3, 2, 3)
        lo, hi = rank * sample_size // world, (rank + 1) * sample_size // world
        weight = (hi - lo) / sample_size  # this rank's share of the global mean loss
        activations = None
        every = max(1, epochs // MAX_PROGRESS_POINTS)
        last_saved = time.time()
        # GPU models: the parameters live in one flat device buffer (ParamStore); autograd
        # accumulates every gradient into views of one flat gradient buffer and the update is the
        # fused optimizer kernel (csrc/optim.hip, the trainer's), not torch.optim's per-tensor ops —
        # same math, and the torch.optim.Adam state stays the checkpointed object (its moments
        # become views of the kernel's flat buffers)
        fused, flat_grad, grad_views = None, None, None
        if self._param_store is not None and self._param_store.device.type == "cuda":
            from ..engine.optim import FusedOptimizer
            store = self._param_store
            fused = FusedOptimizer(store, self.params, self.optimizer, {})
            flat_grad = torch.zeros_like(store.flat)
            by_param = {seg.param_index: seg for seg in store.segments}
            grad_views = [store.view(by_param[i], flat_grad) for i in range(len(self.params))]
        for epoch in range(epochs):
            if sampler is None:  # the reference's draw from the global RNG
                picks = torch.randint(0, len(data), (sample_size,))
            else:
                picks = torch.randint(0, len(data), (sample_size,), generator=sampler)
            if world > 1:
                picks = picks[lo:hi]
            sample = [data[i] for i in picks]
            lr = learning_rate * (decay_rate ** epoch)
            if self.optimizer is not None:
                for group in self.optimizer.param_groups:
                    group["lr"] = lr
            inputs = self._input_tensor([inp for inp, _ in sample])
            target = [tgt for _, tgt in sample]
            prev_weights = [w.clone().detach() for w in self.weights]
            for p in self.params:
                p.requires_grad_()
            activations, cost = self._forward(inputs, target, dropout_rate)
            if l2_lambda > 0.0:
                cost = cost + l2_lambda * sum((w ** 2).sum() for w in self.weights)
            if fused is not None:  # backward accumulates into the zeroed flat buffer's views
                flat_grad.zero_()
                for p, gv in zip(self.params, grad_views):
                    p.grad = gv
            else:
                for p in self.params:
                    p.grad = None
            long_training = time.time() - last_saved >= CHECKPOINT_INTERVAL_S
            if epoch + 1 == epochs or long_training:
                for a in activations:
                    a.retain_grad()
            if world > 1:
                # the rank's share of the global objective: gradients then simply SUM over the ranks
                # (and a synchronised batchnorm's all-reduce backward combines the shares correctly)
                (cost * weight).backward()
                self._average_gradients(ctx, 1.0)
            else:
                cost.backward()
            if fused is not None:  # (the L2 term is already in the autograd gradient)
                fused.step(flat_grad, lr, 0.0, 1.0)
                fused.sync_torch_state()
            elif self.optimizer is not None:
                self.optimizer.step()
            else:
                for p in self.params:
                    p.data -= lr * p.grad
            when, value = datetime.now().isoformat(), cost.item()
            if world > 1:
                value = ctx.all_reduce_scalar(value * weight)
            if epoch % every == 0:
                with torch.no_grad():
                    ratios = [((w - pw).data.std() / (w.data.std() + 1e-8)).item()
                              for pw, w in zip(prev_weights, self.weights)]
                self._progress_point(when, epoch, value, ratios, {"world_size": world} if world > 1 else None)
            log.info(f"Model {self.model_id}: Epoch {epoch + 1}, Cost: {value:.4f}")
            if long_training:  # pragma: no cover - timing dependent
                self._record_training_overall_progress(activations)
                self.serialize_background()
                last_saved = time.time()
        if activations is not None:
            self._record_training_overall_progress(activations)

    def _average_gradients(self, ctx, weight: float) -> None:
        """Global-batch mean of every parameter gradient: each rank's shard-mean gradient weighted
        by its share of the sample, summed over the ranks in one flat all-reduce."""
        grads = [p.grad for p in self.params]
        flat = torch.cat([g.reshape(-1) for g in grads]) * weight
        ctx.wait_all([ctx.all_reduce_async(flat, exact=True)])
        off = 0
        for g in grads:
            g.copy_(flat[off:off + g.numel()].view_as(g))
            off += g.numel()

    def _fused_trainer(self):
        from ..engine.trainer import FusedTrainer, UnsupportedModel
        try:
            return FusedTrainer(self, self._dp_context())
        except UnsupportedModel as e:
            log.info(f"Model {self.model_id}: fused engine unavailable ({e}); training under autograd")
            return None

    def _drain_progress(self, trainer, sample_size: int) -> None:
        drained = trainer.drain()
        world = trainer.ctx.world_size
        for epoch, cost, ratios, when in drained:
            if ratios is not None:
                ms = trainer.step_ms.get(epoch)
                extra = {"device": str(self.device), "dtype": self.precision.name, "world_size": world}
                if ms:
                    extra["step_ms"] = round(ms, 4)
                    extra["samples_per_s"] = round(sample_size / (ms * 1e-3), 1)
                self._progress_point(when, epoch, cost, ratios, extra)
            log.info(f"Model {self.model_id}: Epoch {epoch + 1}, Cost: {cost:.4f}")

    def _record_fused(self, trainer) -> None:
        rec = trainer.record()
        self._record_training_overall_progress(rec["activations"], rec["act_grads"], rec["weight_grads"])

    def _train_fused(self, trainer, data, epochs, learning_rate, sample_size, decay_rate, dropout_rate, l2_lambda):
        """Same schedule as :meth:`_train_autograd`, enqueued on the GPU without host syncs;
        costs / ratios / timestamps come back in :meth:`FusedTrainer.drain`."""
        self._predictor = None
        trainer.load_data(data)
        trainer.begin(epochs, lr_schedule=lambda e: learning_rate * decay_rate ** e)
        every = max(1, epochs // MAX_PROGRESS_POINTS)
        last_saved = time.time()
        agree = _SaveAgreement(trainer.ctx, trainer.dev) if trainer.ctx.enabled else None
        for epoch in range(epochs):
            long_training = time.time() - last_saved >= CHECKPOINT_INTERVAL_S
            if agree is not None:
                long_training = agree.decide(long_training)
            trainer.step(epoch, learning_rate * decay_rate ** epoch, sample_size, dropout_rate, l2_lambda,
                         want_ratios=epoch % every == 0, record=epoch + 1 == epochs or long_training)
            if long_training:
                self._drain_progress(trainer, sample_size)
                self._record_fused(trainer)
                self.serialize_background()
                last_saved = time.time()
        self._drain_progress(trainer, sample_size)
        if epochs:
            self._record_fused(trainer)

    # ------------------------------------------------------------------------------------
    # diagnostics (reference :532-585)
    # ------------------------------------------------------------------------------------
    def _record_training_overall_progress(self, activations, act_grads=None, weight_grads=None):
        costs = [p["cost"] for p in self.progress]
        if not costs:
            return
        avg = sum(costs) / len(costs)
        self.avg_cost = ((self.avg_cost or avg) + avg) / 2.0
        self.avg_cost_history.append(self.avg_cost)
        if len(self.avg_cost_history) > MAX_COST_HISTORY:
            self.avg_cost_history.pop(random.randint(1, 98))
        if act_grads is None:
            act_grads = [a.grad for a in activations]
        if weight_grads is None:
            weight_grads = [layer.weights.grad if layer.weights is not None else None for layer in self.layers]
        self.stats = build_stats(self.layers, activations, act_grads, weight_grads)
        log.info(f"Model {self.model_id} - Cost: {avg:.4f} Overall Cost: {self.avg_cost:.4f}")


__all__ = ["NeuralNetworkModel"]
