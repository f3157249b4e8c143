"""Forward-only GPU inference — the serving counterpart of :mod:`.trainer`.

``compute_output`` runs a GPU model through the autograd layer loop: every linear layer
re-converts its fp32 master weights to the GEMM dtype, activation and softmax are launches of their
own, each op saves an autograd context nobody reads, and a batch under 64 rows never reaches a
kernel made for it. :class:`FusedPredictor` is the explicit forward schedule instead, under
``torch.no_grad()`` and with no autograd functions:

    [embedding_fwd]  ->  per stage:  linear | batchnorm (eval, running statistics) | flatten (view)
                     ->  softmax_rows on the fp32 logits (softmax heads)

* the model structure is :func:`.trainer.compile_stages`' (a model it cannot group raises
  :class:`.trainer.UnsupportedModel`; so do ``float64`` models, which stay on the layer loop);
* the GEMM-dtype copies of the weights are made ONCE, at construction: bf16 for the ``bfloat16``
  and ``fp8`` policies; ``float32`` models use the fp32 masters themselves (no copy). Biases,
  batchnorm parameters and embedding tables are the live fp32 master views. The owner
  (:meth:`NeuralNetworkModel.predict`) drops the predictor whenever the parameters may have changed;
* a linear stage with fewer than 64 rows runs in chunks of at most 16 rows through
  ``PF.gemm_skinny`` (csrc/gemm_skinny.hip: weight streaming, bias and activation fused); a layer
  that kernel does not take (e.g. 2 output columns) runs ``PF.gemm`` for that layer only;
* with 64 rows or more it is one ``PF.gemm`` with the fused forward epilogue (bias + activation,
  no dropout) — the training step's tiled kernels. The last linear stage stores fp32, which those
  kernels do as a plain store with bias; an activation behind it (an MSE head's sigmoid) is then
  one elementwise launch on the fp32 values;
* hidden activations are in the GEMM dtype (bf16 for bf16 models — the fused trainer's numerics,
  also behind an embedding, whose lookups the layer loop keeps in fp32), the last linear stage's
  output and the softmax are fp32.

Weight-only quantised inference, ``forward(x, weights="fp8")`` (bf16-compute models only): the same
schedule on OCP e4m3 weight copies with one power-of-two scale per output column
(``PF.quantize_cols`` of the fp32 masters; csrc/quant_cols.hip). Activations stay bf16, accumulation
fp32, biases / batchnorm / embedding / softmax are untouched. The copies are built lazily, per layer,
on the first fp8 request that needs them, so a predictor never asked for fp8 holds none:

* below 64 rows a linear stage runs ``PF.gemm_skinny_w8`` (csrc/gemm_skinny_w8.hip) in chunks of at
  most 16 rows; a layer that kernel does not take (an output width that is no multiple of 16, e.g.
  72) runs the bf16 path above on a **dequantised bf16 copy** of that layer;
* from 64 rows on, the tiled ``PF.gemm`` calls run on the dequantised bf16 copies.

The scales being powers of two, ``w8 * scale`` is exactly representable in bf16 and every product
of the e4m3 kernel is exact in fp32: whichever kernel runs computes the same function of the same
weight values, so the row a caller gets back does not change its meaning with the batch size. A
process that serves both regimes in fp8 holds 1 + 2 bytes per weight (e4m3 + dequantised bf16) on
top of the default path's copies; one that only sends batches under 64 rows holds 1 byte per weight
of the eligible layers. Measured (profiles/predict_w8_latency.txt): the e4m3 kernel beats the bf16
one at 1 row on every layer shape tried and at every row count on an 8192 x 8192 layer, and is
1.2-1.4x slower at 16 rows on layers of 16 Mi weights or fewer; the chunks still go through it, so
that the memory held does not depend on the batch sizes a process happens to see.

Token generation, :meth:`FusedPredictor.generate` (embedding first, softmax head, at least as many
embedding rows as classes): the context ``[rows, L]`` (``L`` = :attr:`FusedPredictor.context_length`,
the product of the flatten ratios) is uploaded once into an int64 buffer ``seq [rows, L + steps]``
and range-checked once; step ``s`` runs the stage loop above without the head (``_logits``) on the
window ``seq[:, s : s + L]`` — nothing is shifted in place, ``embedding_fwd`` reads a contiguous copy
of the view, its id check is skipped because the ids come from the sampling kernel — and one
``PF.sample_rows`` launch (csrc/sample.hip) draws ``seq[:, L + s]`` from the fp32 logits. No host
read happens inside the loop; the caller downloads ``seq[:, L:]`` once.

One-launch generation, :meth:`FusedPredictor.generate_resident` (``generate(loop="resident")`` of the
model): for models whose parameters fit in one workgroup's LDS (:mod:`.resident` plans the layout
within 160 KiB, once per predictor; at most 8192 classes), ``PF.generate_resident``
(csrc/generate_resident.hip) is the whole request. One workgroup per row copies the parameters into
LDS, keeps the window on chip and per token runs embedding, the stages and the sampler
(csrc/sample_core.h, the code of ``sample_rows``) between barriers; only the token store leaves the
CU. The weights are the predictor's compute-dtype copies (``weights="fp8"``: the dequantised bf16
copies, which are the e4m3 path's function exactly), the batchnorm running statistics are converted
per call. The tokens are those ``PF.sample_rows`` draws from the kernel's own logits, which differ
from the per-token loop's by fp32 summation order only. It is opt-in: a model that does not fit
raises ``ValueError`` with the planner's reason, never a fall-back to the loop.

Sequence scoring, :meth:`FusedPredictor.score` (the models that can generate): how likely the model
finds ids it is given. ``seq [R, W]`` is uploaded and range-checked once; every window
``seq[r, j : j + L]`` becomes a row of one ``[R * (W - L), L]`` matrix (torch views), which runs through
``_logits`` in chunks of rows whose fp32 logits stay within ``SCORE_LOGITS_BYTES``; one
``PF.token_logprob`` launch per chunk (csrc/token_logprob.hip) writes the log-probability and the rank
of ``seq[r, L + j]`` straight into the ``[R, W - L]`` results, which stay on the device. It is also what
``generate(..., logprobs=True)`` runs once, after its loop, on ``[context | tokens]``.

Top-k answers (csrc/topk_rows.hip): :meth:`FusedPredictor.classify` is ``_logits`` and one ``PF.topk_rows``
launch — the k most likely classes of every row in rank order with their log-probabilities, no softmax
row; ``score(..., top_logprobs=k)`` makes the same launch once more per chunk on the chunk's logits.
"""
from __future__ import annotations

import torch
from torch import Tensor

from ..ops import functional as PF
from ..ops import native
from .resident import RESIDENT_LDS_BYTES, describe_stages, resident_plan
from .trainer import UnsupportedModel, compile_stages

SKINNY_BELOW = 64  # rows from which the tiled GEMMs (M >= 64 on the matrix cores) take over
SCORE_LOGITS_BYTES = 64 << 20  # score(): the fp32 logits of one chunk of windows stay within this


class FusedPredictor:
    """Owns the GEMM-dtype weight copies of one GPU model and runs its forward pass."""

    def __init__(self, model):
        native.require()
        store = model._param_store
        if store is None or store.device.type != "cuda":
            raise UnsupportedModel("CPU models predict through the layer loop (the reference's own runtime)")
        if model.precision.master != torch.float32:
            raise UnsupportedModel("float64 models predict through the layer loop")
        self.model = model
        self.store = store
        self.dev = store.device
        self.compute = torch.bfloat16 if model.precision.name in ("bfloat16", "fp8") else torch.float32
        self.stages, self.head = compile_stages(model)
        for i, st in enumerate(self.stages):
            st.index = i
        self.weights: dict[int, Tensor] = {}
        self.biases: dict[int, Tensor | None] = {}
        self._skinny_ok: dict[int, bool] = {}
        # weights="fp8": e4m3 copies + column scales, their dequantised bf16 copies; built on demand
        self.weights8: dict[int, tuple[Tensor, Tensor]] = {}
        self.weights_deq: dict[int, Tensor] = {}
        self._w8_ok: dict[int, bool] = {}
        self._resident = None  # the one-launch generation plan (or the reason there is none), made on first need
        gemms = [st for st in self.stages if st.kind == "gemm"]
        self.last_gemm = gemms[-1].index if gemms else -1
        with torch.no_grad():
            for st in gemms:
                w = store.view(st.seg_w)
                self.weights[st.index] = w if w.dtype == self.compute else w.to(self.compute).contiguous()
                self.biases[st.index] = store.view(st.seg_b) if st.seg_b is not None else None

    # ------------------------------------------------------------------------------------
    def _quantised(self, index: int) -> tuple[Tensor, Tensor]:
        """(e4m3 copy, column scales) of one linear stage's fp32 master, built on first need."""
        if index not in self.weights8:
            self.weights8[index] = PF.quantize_cols(self.store.view(self.stages[index].seg_w))
        return self.weights8[index]

    def _dequantised(self, index: int) -> Tensor:
        """bf16 copy of the quantised weights (exact: the scales are powers of two), built on first need."""
        if index not in self.weights_deq:
            self.weights_deq[index] = PF.dequantize_cols(*self._quantised(index), dtype=self.compute).contiguous()
        return self.weights_deq[index]

    def _linear(self, st, x: Tensor, fp8: bool = False) -> Tensor:
        bias = self.biases[st.index]
        k, n = self.weights[st.index].shape
        if x.shape[-1] != k:
            raise ValueError(f"layer {st.first} expects {k} inputs per row, got {x.shape[-1]}")
        lead = x.shape[:-1]
        x2 = x.reshape(-1, k)
        if x2.dtype != self.compute:
            x2 = x2.to(self.compute)
        x2 = x2.contiguous()
        rows = x2.shape[0]
        last = st.index == self.last_gemm
        out = torch.empty(rows, n, device=self.dev, dtype=torch.float32 if last else self.compute)
        if rows == 0:
            return out.view(*lead, n)
        if fp8 and rows < SKINNY_BELOW:
            w8, scale = self._quantised(st.index)
            ok8 = self._w8_ok.get(st.index)
            if ok8 is None:  # a property of the layer, as _skinny_ok
                ok8 = self._w8_ok[st.index] = PF.gemm_skinny_w8_eligible(x2[:PF.SKINNY_MAX_ROWS], w8, scale,
                                                                          out[:PF.SKINNY_MAX_ROWS])
            if ok8:
                for r0 in range(0, rows, PF.SKINNY_MAX_ROWS):
                    PF.gemm_skinny_w8(x2[r0:r0 + PF.SKINNY_MAX_ROWS], w8, scale, out[r0:r0 + PF.SKINNY_MAX_ROWS],
                                      bias=bias, act=st.act)
                return out.view(*lead, n)
        # the bf16 / fp32 kernels: on the default copies, or on the dequantised ones of an fp8 request
        w = self._dequantised(st.index) if fp8 else self.weights[st.index]
        if rows < SKINNY_BELOW:
            ok = self._skinny_ok.get(st.index)
            for r0 in range(0, rows, PF.SKINNY_MAX_ROWS):
                xs, os_ = x2[r0:r0 + PF.SKINNY_MAX_ROWS], out[r0:r0 + PF.SKINNY_MAX_ROWS]
                if ok is None:  # a property of the layer (W's shape and alignment): asked once
                    ok = self._skinny_ok[st.index] = PF.gemm_skinny_eligible(xs, w, os_)
                if ok:
                    PF.gemm_skinny(xs, w, os_, bias=bias, act=st.act)
                else:
                    PF.gemm(xs, True, w, False, os_, bias=bias, mode=PF.EPI_FWD, epi=PF.epi_spec(act=st.act))
        elif last:
            # fp32 output: the tiled kernels store it plainly (with the bias); an activation follows
            PF.gemm(x2, True, w, False, out, bias=bias)
            if st.act != PF.ACT_NONE:
                pre, out = out, torch.empty_like(out)
                ei, ef = PF.epi_spec(act=st.act)
                torch.ops.pz.stage_fwd(pre, out, ei, ef)
        else:
            PF.gemm(x2, True, w, False, out, bias=bias, mode=PF.EPI_FWD, epi=PF.epi_spec(act=st.act))
        return out.view(*lead, n)

    def _batchnorm(self, st, x: Tensor) -> Tensor:
        layer = st.layer
        gain, bias = self.store.view(st.seg_w), self.store.view(st.seg_b)
        cols = gain.shape[0]
        if x.shape[-1] != cols:
            raise ValueError(f"layer {st.first} expects {cols} inputs per row, got {x.shape[-1]}")
        xc = x.contiguous()
        y = torch.empty_like(xc)
        rows = xc.numel() // max(cols, 1)
        # the layer's running statistics as they are NOW (a training-mode forward replaces them)
        rmean = layer.mean.detach().reshape(-1).to(device=self.dev, dtype=gain.dtype).contiguous()
        rvar = layer.variance.detach().reshape(-1).to(device=self.dev, dtype=gain.dtype).contiguous()
        ws = torch.empty(4 * cols, device=self.dev, dtype=torch.float64)
        ei, ef = PF.epi_spec(act=st.act)
        torch.ops.pz.batchnorm_fwd(xc, y, gain, bias, rmean, rvar, float(layer.eps), float(layer.momentum), False, rows,
                                   ws[:cols], ws[cols:2 * cols], ws[2 * cols:], ei, ef, 0)
        return y

    def _embed(self, st, ids: Tensor, check: bool = True) -> Tensor:
        table = self.store.view(st.seg_w)
        vocab = table.shape[0]
        if check:  # (one device sync; the generation loop's ids come from the sampling kernel and are < V)
            PF.check_index_range(ids.reshape(-1), -vocab, vocab, "index", vocab)  # as PF.embedding
        idc = ids.contiguous()
        out = torch.empty(*idc.shape, table.shape[1], device=self.dev, dtype=self.compute)
        torch.ops.pz.embedding_fwd(table, idc, out)
        return out

    def _want_fp8(self, weights: str | None) -> bool:
        if weights not in (None, "fp8"):
            raise ValueError(f"unknown weights {weights!r}: None (the model's own precision) or 'fp8'")
        fp8 = weights == "fp8"
        if fp8 and self.compute != torch.bfloat16:
            raise ValueError(f"weights='fp8' is for bfloat16 / fp8 models; a {self.model.precision.name} model "
                             "asked for exact weights")
        return fp8

    def _logits(self, x: Tensor, fp8: bool = False, check_ids: bool = True) -> Tensor:
        """The stage loop without the head: the fp32 output of the last stage (a softmax head's logits)."""
        x = x.to(self.dev)
        if self.stages[0].kind != "embed" and x.dtype != self.compute:
            x = x.to(self.compute)
        for st in self.stages:
            if st.kind == "embed":
                x = self._embed(st, x, check_ids)
            elif st.kind == "flatten":
                x = st.layer.forward(x)  # a view
            elif st.kind == "gemm":
                vector = x.dim() == 1
                x = self._linear(st, x.unsqueeze(0) if vector else x, fp8)
                x = x.squeeze(0) if vector else x
            else:
                x = self._batchnorm(st, x)
        if x.dtype != torch.float32:
            x = x.float()
        return x

    @torch.no_grad()
    def forward(self, x: Tensor, weights: str | None = None) -> Tensor:
        """``x``: what ``_forward`` takes — a vector, a batch, or id sequences for embedding models
        (any float / int dtype; moved to the model's device). Returns the fp32 output tensor.
        ``weights="fp8"``: the linear stages read the e4m3 weight copies (module docstring)."""
        x = self._logits(x, self._want_fp8(weights))
        if self.head == "softmax":
            xc = x.contiguous()
            y = torch.empty_like(xc)
            if xc.numel():
                torch.ops.pz.softmax_rows(xc, y)
            x = y
        return x

    @torch.no_grad()
    def classify(self, x: Tensor, k: int, weights: str | None = None) -> tuple[Tensor, Tensor]:
        """The ``k`` most likely classes of every row of ``x`` (what :meth:`forward` takes; a 1-D input is
        one row): ``(idx int32 [rows, k], logprob fp32 [rows, k])`` on the device, in rank order, by the
        rule of :func:`..ops.functional.topk_rows_reference`. The forward kernels, then one
        ``PF.topk_rows`` launch on the logits (csrc/topk_rows.hip); the softmax is never materialised.
        ValueError for another head (its outputs are no distribution) and for ``k`` outside
        ``[1, min(classes, 64)]``."""
        fp8 = self._want_fp8(weights)
        if self.head != "softmax":
            raise ValueError(f"classify needs a softmax head, this model ends in {self.head!r}")
        width = self.stages[-1].out_width
        k = PF.check_topk(k, width)
        logits = self._logits(x, fp8).reshape(-1, width)
        return PF.topk_rows(logits, k)

    # ------------------------------------------------------------------------------------
    # token generation
    # ------------------------------------------------------------------------------------
    @property
    def context_length(self) -> int:
        """Ids per row for which the model's output is one distribution per row: the product of the
        flatten ratios (each flatten merges that many adjacent positions)."""
        length = 1
        for st in self.stages:
            if st.kind == "flatten":
                length *= int(st.layer.ratio)
        return length

    def generation_unsupported(self) -> str | None:
        """Why this model cannot generate tokens (None: it can)."""
        if self.stages[0].kind != "embed":
            return "token generation needs an embedding first layer"
        if self.head != "softmax":
            return "token generation needs a softmax head"
        vocab, width = self.store.view(self.stages[0].seg_w).shape[0], self.stages[-1].out_width
        if width > vocab:
            return f"the model predicts {width} classes but embeds {vocab} ids: a sampled id could not be fed back"
        return None

    @torch.no_grad()
    def generate(self, context: Tensor, max_new_tokens: int, temperature: float = 1.0, top_k: int | None = None,
                 seed: tuple[int, int] = (0, 0), stop_token: int | None = None, weights: str | None = None,
                 top_p: float | None = None, min_p: float | None = None) -> Tensor:
        """``context``: int ids ``[rows, context_length]``. Returns the int64 ``[rows, max_new_tokens]``
        continuation, on the device. One upload, then per token the forward kernels on the window
        ``seq[:, s : s + L]`` and one ``PF.sample_rows`` launch that writes ``seq[:, L + s]``; nothing is
        read back inside the loop. Step ``s`` of row ``r`` draws ``PF.sample_uniform(seed, r, s)``; a row
        that drew ``stop_token`` repeats it from then on. ``top_p`` / ``min_p`` as in
        :func:`..ops.functional.sample_rows_reference`; they reach the sampler only when set."""
        fp8 = self._want_fp8(weights)
        extra = PF.nucleus_args(top_p, min_p)
        reason = self.generation_unsupported()
        if reason is not None:
            raise ValueError(reason)
        length, steps = self.context_length, int(max_new_tokens)
        context = torch.as_tensor(context)
        if context.dim() != 2 or context.shape[1] != length or context.is_floating_point():
            raise ValueError(f"context must be an int tensor [rows, {length}], got {tuple(context.shape)} {context.dtype}")
        if steps < 1:
            raise ValueError(f"max_new_tokens must be >= 1, got {max_new_tokens}")
        rows = context.shape[0]
        seq = torch.empty(rows, length + steps, device=self.dev, dtype=torch.int64)
        seq[:, :length] = context.to(device=self.dev, dtype=torch.int64)
        if rows == 0:
            return seq[:, length:]
        vocab = self.store.view(self.stages[0].seg_w).shape[0]
        PF.check_index_range(seq[:, :length].reshape(-1), -vocab, vocab, "index", vocab)  # once; the loop skips it
        done = torch.zeros(rows, device=self.dev, dtype=torch.int32)
        width = self.stages[-1].out_width
        for s in range(steps):
            logits = self._logits(seq[:, s:s + length], fp8, check_ids=False).reshape(rows, width)
            PF.sample_rows(logits, seq, done, length + s, seed=seed, step=s, temperature=temperature, top_k=top_k,
                           stop_token=stop_token, **extra)
        return seq[:, length:]

    # ------------------------------------------------------------------------------------
    # sequence scoring (csrc/token_logprob.hip)
    # ------------------------------------------------------------------------------------
    @torch.no_grad()
    def score(self, seq: Tensor, weights: str | None = None, chunk_rows: int | None = None,
              top_logprobs: int | None = None) -> tuple:
        """``seq``: int ids ``[R, W]`` with ``W > L`` = :attr:`context_length`. Returns ``(logprob fp32
        [R, W - L], rank int32 [R, W - L])`` on the device: entry ``[r, j]`` is the log-probability and the
        rank (0 = the most likely class) of ``seq[r, L + j]`` under the distribution the model gives the
        window ``seq[r, j : j + L]`` (:func:`..ops.functional.token_logprob_reference`).

        One upload, one range check (window ids as ``PF.embedding`` takes them, scored ids in
        ``[0, classes)``), then per chunk of ``chunk_rows`` windows (default: as many as keep a chunk's
        fp32 logits within ``SCORE_LOGITS_BYTES``) the forward kernels and one ``PF.token_logprob`` launch
        that writes its slice of the results; nothing is read back inside the loop.

        ``top_logprobs=k`` (``1 <= k <= min(classes, 64)``) adds one ``PF.topk_rows`` launch per chunk on the
        same logits and returns ``(logprob, rank, top_idx int32 [R, W - L, k], top_logprob fp32 [R, W - L, k])``:
        what the model would have preferred at every scored position, in rank order. Unset, the call makes
        the launches and returns the two tensors it always did."""
        fp8 = self._want_fp8(weights)
        reason = self.generation_unsupported()
        if reason is not None:
            raise ValueError(reason)
        length = self.context_length
        seq = torch.as_tensor(seq)
        if seq.dim() != 2 or seq.shape[1] <= length or seq.is_floating_point() or seq.dtype == torch.bool:
            raise ValueError(f"seq must be an int tensor [rows, more than {length}], got {tuple(seq.shape)} {seq.dtype}")
        width = self.stages[-1].out_width
        if chunk_rows is None:
            chunk_rows = max(1, SCORE_LOGITS_BYTES // (4 * width))
        if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1:
            raise ValueError(f"chunk_rows must be an integer >= 1, got {chunk_rows!r}")
        k = None if top_logprobs is None else PF.check_topk(top_logprobs, width, "top_logprobs")
        seq = seq.to(device=self.dev, dtype=torch.int64)
        rows, scored = seq.shape[0], seq.shape[1] - length
        logprob = torch.empty(rows, scored, device=self.dev, dtype=torch.float32)
        rank = torch.empty(rows, scored, device=self.dev, dtype=torch.int32)
        tops = ()
        if k is not None:
            tops = (torch.empty(rows, scored, k, device=self.dev, dtype=torch.int32),
                    torch.empty(rows, scored, k, device=self.dev, dtype=torch.float32))
        if rows == 0:
            return (logprob, rank) + tops
        vocab = self.store.view(self.stages[0].seg_w).shape[0]
        # once, one read (the loop skips the id check): PF.check_index_range's rule for the context columns as
        # PF.embedding takes them, and for the scored columns as classes (width <= vocab: they are valid inputs too)
        lo_c, hi_c, lo_t, hi_t = torch.stack(torch.aminmax(seq[:, :length]) + torch.aminmax(seq[:, length:])).tolist()
        if lo_c < -vocab or hi_c >= vocab:
            raise IndexError(f"index {lo_c if lo_c < -vocab else hi_c} is out of bounds for size {vocab}")
        if lo_t < 0 or hi_t >= width:
            raise IndexError(f"Target {lo_t if lo_t < 0 else hi_t} is out of bounds for size {width}")
        # window i = r * scored + j holds seq[r, j : j + L] and is scored on seq[r, L + j]
        windows = seq.unfold(1, length, 1)[:, :scored].reshape(rows * scored, length)
        targets = seq[:, length:].reshape(-1)
        lp, rk = logprob.view(-1), rank.view(-1)
        for i0 in range(0, rows * scored, chunk_rows):
            i1 = min(i0 + chunk_rows, rows * scored)
            logits = self._logits(windows[i0:i1], fp8, check_ids=False).reshape(i1 - i0, width)
            PF.token_logprob(logits, targets[i0:i1], lp[i0:i1], rk[i0:i1])
            if k is not None:
                PF.topk_rows(logits, k, tops[0].view(-1, k)[i0:i1], tops[1].view(-1, k)[i0:i1])
        return (logprob, rank) + tops

    # ------------------------------------------------------------------------------------
    # one-launch generation (csrc/generate_resident.hip)
    # ------------------------------------------------------------------------------------
    def resident_plan(self, budget: int = RESIDENT_LDS_BYTES):
        """The LDS plan of this model (:func:`.resident.resident_plan`) or the reason it has none; the
        default-budget answer is made once and kept."""
        if budget != RESIDENT_LDS_BYTES:
            return resident_plan(describe_stages(self.stages), self.compute, self.context_length, budget, head=self.head)
        if self._resident is None:
            self._resident = resident_plan(describe_stages(self.stages), self.compute, self.context_length, head=self.head)
        return self._resident

    def resident_params(self, plan, fp8: bool = False) -> list[Tensor]:
        """The tensors ``plan.params`` names, in its order: the table, per linear stage the compute-dtype
        weights (the dequantised e4m3 copies for ``fp8``) and the bias, per batchnorm stage gain, bias and
        the layer's running statistics as they are now, in fp32."""
        out = []
        for index, role in plan.params:
            st = self.stages[index]
            if role == "weights" and st.kind == "gemm":
                out.append((self._dequantised(index) if fp8 else self.weights[index]).contiguous())
            elif role in ("table", "weights", "gain"):
                out.append(self.store.view(st.seg_w).contiguous())
            elif role == "bias":
                out.append(self.store.view(st.seg_b).contiguous())
            else:  # not in the store: converted per call, as _batchnorm does
                stat = st.layer.mean if role == "mean" else st.layer.variance
                out.append(stat.detach().reshape(-1).to(device=self.dev, dtype=torch.float32).contiguous())
        return out

    @torch.no_grad()
    def generate_resident(self, context: Tensor, max_new_tokens: int, temperature: float = 1.0, top_k: int | None = None,
                          seed: tuple[int, int] = (0, 0), stop_token: int | None = None, weights: str | None = None,
                          logits_out: Tensor | None = None, top_p: float | None = None,
                          min_p: float | None = None) -> Tensor:
        """:meth:`generate` as ONE launch: every row's workgroup keeps the model in LDS and loops over the
        tokens itself. Same arguments, same rule, same random numbers; the logits differ from the
        per-token loop's by fp32 summation order only. ``logits_out`` (fp32 ``[rows, steps, V]``, zeroed
        by the caller) receives each step's logits. ValueError with the planner's reason for a model
        that does not fit."""
        fp8 = self._want_fp8(weights)
        plan = self.resident_plan()
        if isinstance(plan, str):
            raise ValueError(plan)
        length, steps = self.context_length, int(max_new_tokens)
        context = torch.as_tensor(context)
        if context.dim() != 2 or context.shape[1] != length or context.is_floating_point():
            raise ValueError(f"context must be an int tensor [rows, {length}], got {tuple(context.shape)} {context.dtype}")
        if steps < 1:
            raise ValueError(f"max_new_tokens must be >= 1, got {max_new_tokens}")
        rows = context.shape[0]
        seq = torch.empty(rows, length + steps, device=self.dev, dtype=torch.int64)
        seq[:, :length] = context.to(device=self.dev, dtype=torch.int64)
        if rows == 0:
            return seq[:, length:]
        vocab = self.store.view(self.stages[0].seg_w).shape[0]
        PF.check_index_range(seq[:, :length].reshape(-1), -vocab, vocab, "index", vocab)
        done = torch.zeros(rows, device=self.dev, dtype=torch.int32)
        PF.generate_resident(seq, done, self.resident_params(plan, fp8), plan.ints, steps, seed=seed,
                             temperature=temperature, top_k=top_k, stop_token=stop_token, logits_out=logits_out,
                             **PF.nucleus_args(top_p, min_p))
        return seq[:, length:]


__all__ = ["FusedPredictor", "UnsupportedModel", "SKINNY_BELOW", "SCORE_LOGITS_BYTES", "resident_plan", "RESIDENT_LDS_BYTES"]
