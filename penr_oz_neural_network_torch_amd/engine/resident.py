"""LDS layout of the one-launch generation kernel (csrc/generate_resident.hip).

:func:`resident_plan` turns a stage list into the int list the kernel reads, or into the reason why
the model cannot run resident. It is pure Python and takes no tensors, so it runs (and is tested)
without a GPU. The int list (slot names: csrc/pz_kernels.h, ``ResHead`` / ``ResParam`` / ``ResStage``):

* ``HEAD`` ints: magic, context length ``L``, embedding width ``E``, table rows, classes ``V``, stage
  and parameter counts, table-in-LDS flag, compute element size, bytes of one activation buffer, the
  byte offsets of the id window, the two activation buffers, the logits row, the sampler's scratch
  and the K-split partial sums, and the total;
* per parameter ``(offset, numel, element size)`` in the order the kernel receives the tensors —
  the table first, then per linear stage the weights and (if any) the bias, per batchnorm stage gain,
  bias, running mean, running variance. Offset ``-1``: the parameter stays in global memory (only the
  table may);
* per stage ``(kind, P, K, N, act, parameter indices, batchnorm scratch offset, eps bits)``.

Everything is 16-byte aligned. The order is: window, buffers, logits, partial sums, sampler scratch,
batchnorm scratch, parameters, and the table last — it goes to LDS when it still fits in the budget
and is read from global memory (``L`` rows per token) otherwise.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

RESIDENT_LDS_BYTES = 160 * 1024   # an MI355X CU's LDS: one workgroup may hold all of it
RESIDENT_MAX_VOCAB = 8192         # the 256-thread form of the sampler (csrc/sample_core.h)
SAMPLER_LDS_BYTES = 16912         # sizeof(SampleScratch)
PARTIAL_LDS_BYTES = 1024          # 256 floats of K-split partial sums
MAX_STAGES, MAX_PARAMS = 16, 64
MAGIC = 0x5A52
HEAD, PARAM, STAGE = 20, 3, 12
KIND_FLATTEN, KIND_GEMM, KIND_BN = 0, 1, 2
# header slots
(H_MAGIC, H_L, H_E, H_VOCAB, H_V, H_STAGES, H_PARAMS, H_TABLE_LDS, H_ESIZE, H_BUF_BYTES, H_OFF_WIN, H_OFF_BUF0,
 H_OFF_BUF1, H_OFF_LOGITS, H_OFF_SAMPLER, H_OFF_PARTIAL, H_TOTAL) = range(17)

_ESIZE = {"float32": 4, "bfloat16": 2}


@dataclass
class StageDesc:
    """What the planner needs to know of one stage of :func:`..engine.trainer.compile_stages`."""
    kind: str                 # embed | flatten | gemm | bn
    in_width: int = 0
    out_width: int = 0
    act: int = 0              # PF.ACT_*
    ratio: int = 1            # flatten
    bias: bool = True         # gemm
    eps: float = 1e-5         # bn
    vocab: int = 0            # embed: table rows


def describe_stages(stages) -> list[StageDesc]:
    """:class:`StageDesc` of each compiled stage (reads shapes only, no tensor data)."""
    out = []
    for st in stages:
        d = StageDesc(st.kind, int(st.in_width or 0), int(st.out_width or 0), int(st.act))
        if st.kind == "embed":
            d.vocab = int(st.layer.weights.shape[0])
        elif st.kind == "flatten":
            d.ratio = int(st.layer.ratio)
        elif st.kind == "gemm":
            d.bias = st.seg_b is not None
        elif st.kind == "bn":
            d.eps = float(st.layer.eps)
        out.append(d)
    return out


@dataclass
class ResidentPlan:
    ints: list[int]                       # what the kernel reads
    total: int                            # LDS bytes of a workgroup
    table_in_lds: bool
    params: list[tuple[int, str]]         # (stage index, "table" | "weights" | "bias" | "gain" | "mean" | "var") per tensor
    regions: dict = field(default_factory=dict)  # name -> (offset, bytes), for inspection and tests


def _up16(n: int) -> int:
    return (n + 15) // 16 * 16


def resident_plan(stages, compute_dtype, context_length: int, budget: int = RESIDENT_LDS_BYTES,
                  head: str = "softmax") -> ResidentPlan | str:
    """The plan of a model (``stages``: :class:`StageDesc` list, embed stage first), or the reason it has none."""
    name = str(compute_dtype).replace("torch.", "")
    if name not in _ESIZE:
        return f"the resident kernel computes in bfloat16 or float32, not {name}"
    esize = _ESIZE[name]
    if not stages or stages[0].kind != "embed":
        return "token generation needs an embedding first layer"
    if head != "softmax":
        return "token generation needs a softmax head"
    body = list(stages[1:])
    if not body or body[-1].kind != "gemm":
        return "the resident kernel needs a linear stage before the softmax head"
    if len(body) > MAX_STAGES:
        return f"the resident kernel takes at most {MAX_STAGES} stages, the model has {len(body)}"
    length, width, vocab = int(context_length), int(stages[0].out_width), int(stages[0].vocab)
    classes = int(body[-1].out_width)
    if classes > RESIDENT_MAX_VOCAB:
        return f"the resident kernel samples at most {RESIDENT_MAX_VOCAB} classes, the model predicts {classes}"
    if classes > vocab:
        return f"the model predicts {classes} classes but embeds {vocab} ids: a sampled id could not be fed back"
    if length < 1 or width < 1:
        return "empty context or embedding"

    # shapes: [P, W] per row after each stage
    pos, shapes, widest = length, [], length * width
    for i, st in enumerate(body):
        if st.kind == "flatten":
            if st.ratio < 1 or pos % st.ratio:
                return f"stage {i}: {pos} positions cannot be flattened by {st.ratio}"
            pos, width = pos // st.ratio, width * st.ratio
            shapes.append((KIND_FLATTEN, pos, st.ratio, width))
        elif st.kind == "gemm":
            if st.in_width != width:
                return f"stage {i}: a linear stage of {st.in_width} inputs follows a width of {width}"
            width = int(st.out_width)
            shapes.append((KIND_GEMM, pos, st.in_width, width))
        elif st.kind == "bn":
            if st.out_width != width:
                return f"stage {i}: a batchnorm of {st.out_width} columns follows a width of {width}"
            shapes.append((KIND_BN, pos, width, width))
        else:
            return f"stage {i}: unknown kind {st.kind!r}"
        if i < len(body) - 1:
            widest = max(widest, pos * width)
    if pos != 1:
        return f"the last stage runs on {pos} positions, not 1: the context length must be the product of the flatten ratios"

    regions: dict = {}
    cursor = 0

    def carve(key: str, nbytes: int) -> int:
        nonlocal cursor
        off = cursor
        regions[key] = (off, nbytes)
        cursor = _up16(off + nbytes)
        return off

    buf_bytes = _up16(widest * esize)
    off_win = carve("window", 4 * (length + 1))
    off_buf0, off_buf1 = carve("buf0", buf_bytes), carve("buf1", buf_bytes)
    off_logits = carve("logits", 4 * classes)
    off_partial = carve("partial", PARTIAL_LDS_BYTES)
    off_sampler = carve("sampler", SAMPLER_LDS_BYTES)

    params: list[tuple[int, str]] = [(0, "table")]
    par_ints: list[list[int]] = [[-1, vocab * int(stages[0].out_width), 4]]
    stage_ints: list[int] = []

    def param(stage: int, role: str, numel: int, es: int) -> int:
        params.append((stage, role))
        par_ints.append([carve(f"{role}{stage}", numel * es), numel, es])
        return len(params) - 1

    for i, (st, (kind, p, k, n)) in enumerate(zip(body, shapes), start=1):
        pa = pb = pm = pv = -1
        off_inv = eps_lo = eps_hi = 0
        if kind == KIND_GEMM:
            pa = param(i, "weights", k * n, esize)
            pb = param(i, "bias", n, 4) if st.bias else -1
        elif kind == KIND_BN:
            pa, pb = param(i, "gain", n, 4), param(i, "bias", n, 4)
            pm, pv = param(i, "mean", n, 4), param(i, "var", n, 4)
            off_inv = carve(f"invstd{i}", 8 * n)
            bits = struct.unpack("<Q", struct.pack("<d", float(st.eps)))[0]
            eps_lo, eps_hi = bits & 0xFFFFFFFF, bits >> 32
        stage_ints += [kind, p, k, n, int(st.act), pa, pb, pm, pv, off_inv, eps_lo, eps_hi]
    if len(params) > MAX_PARAMS:
        return f"the resident kernel takes at most {MAX_PARAMS} parameter tensors, the model has {len(params)}"

    table_bytes = par_ints[0][1] * 4
    without_table = cursor
    if without_table > budget:
        return (f"the model needs {_up16(without_table + table_bytes)} bytes of LDS ({without_table} without its embedding "
                f"table) against a budget of {budget}")
    table_in_lds = _up16(without_table + table_bytes) <= budget
    if table_in_lds:
        par_ints[0][0] = carve("table", table_bytes)
    total = cursor

    head_ints = [0] * HEAD
    head_ints[H_MAGIC], head_ints[H_L], head_ints[H_E], head_ints[H_VOCAB], head_ints[H_V] = MAGIC, length, int(stages[0].out_width), vocab, classes
    head_ints[H_STAGES], head_ints[H_PARAMS], head_ints[H_TABLE_LDS] = len(body), len(params), int(table_in_lds)
    head_ints[H_ESIZE], head_ints[H_BUF_BYTES] = esize, buf_bytes
    head_ints[H_OFF_WIN], head_ints[H_OFF_BUF0], head_ints[H_OFF_BUF1] = off_win, off_buf0, off_buf1
    head_ints[H_OFF_LOGITS], head_ints[H_OFF_SAMPLER], head_ints[H_OFF_PARTIAL], head_ints[H_TOTAL] = off_logits, off_sampler, off_partial, total
    ints = head_ints + [v for p in par_ints for v in p] + stage_ints
    return ResidentPlan(ints, total, table_in_lds, params, regions)


__all__ = ["resident_plan", "describe_stages", "StageDesc", "ResidentPlan", "RESIDENT_LDS_BYTES", "RESIDENT_MAX_VOCAB"]
