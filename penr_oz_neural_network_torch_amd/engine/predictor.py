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
"""
from __future__ import annotations

import torch
from torch import Tensor

from ..ops import functional as PF
from ..ops import native
from .trainer import UnsupportedModel, compile_stages

SKINNY_BELOW = 64  # rows from which the tiled GEMMs (M >= 64 on the matrix cores) take over


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
        gemms = [st for st in self.stages if st.kind == "gemm"]
        self.last_gemm = gemms[-1].index if gemms else -1
        with torch.no_grad():
            for st in gemms:
                w = store.view(st.seg_w)
                self.weights[st.index] = w if w.dtype == self.compute else w.to(self.compute).contiguous()
                self.biases[st.index] = store.view(st.seg_b) if st.seg_b is not None else None

    # ------------------------------------------------------------------------------------
    def _linear(self, st, x: Tensor) -> Tensor:
        w, bias = self.weights[st.index], self.biases[st.index]
        k, n = w.shape
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

    def _embed(self, st, ids: Tensor) -> Tensor:
        table = self.store.view(st.seg_w)
        vocab = table.shape[0]
        PF.check_index_range(ids.reshape(-1), -vocab, vocab, "index", vocab)  # as PF.embedding
        idc = ids.contiguous()
        out = torch.empty(*idc.shape, table.shape[1], device=self.dev, dtype=self.compute)
        torch.ops.pz.embedding_fwd(table, idc, out)
        return out

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        """``x``: what ``_forward`` takes — a vector, a batch, or id sequences for embedding models
        (any float / int dtype; moved to the model's device). Returns the fp32 output tensor."""
        x = x.to(self.dev)
        if self.stages[0].kind != "embed" and x.dtype != self.compute:
            x = x.to(self.compute)
        for st in self.stages:
            if st.kind == "embed":
                x = self._embed(st, x)
            elif st.kind == "flatten":
                x = st.layer.forward(x)  # a view
            elif st.kind == "gemm":
                vector = x.dim() == 1
                x = self._linear(st, x.unsqueeze(0) if vector else x)
                x = x.squeeze(0) if vector else x
            else:
                x = self._batchnorm(st, x)
        if x.dtype != torch.float32:
            x = x.float()
        if self.head == "softmax":
            xc = x.contiguous()
            y = torch.empty_like(xc)
            if xc.numel():
                torch.ops.pz.softmax_rows(xc, y)
            x = y
        return x


__all__ = ["FusedPredictor", "UnsupportedModel", "SKINNY_BELOW"]
