"""Inputs shared by the scoring tests (``test_token_logprob_gpu.py``, ``test_score_cpu.py``): seeded logits
of six kinds, their targets, the case list and the kernel's tolerance.

Tolerance of ``pz::token_logprob`` against ``PF.token_logprob_reference`` (fp64 ``log_softmax`` of the same
fp32 logits): ``|got - ref| <= (ceil(V / 256) + 56) * 2^-23 + 2^-22 * |ref|``. The kernel's sum has at most
``D(V) = ceil(V / 256) + 24`` dependent fp32 additions, each half a unit of 2^-23 on a sum normalised to its
largest term; 32 more units cover the rounding of ``exp`` and ``log``, which includes the rounding of
``l - max`` carried through ``exp`` (about ``log V`` <= 12 units on a normalised sum); everything is doubled.
The relative term is the rounding of ``l_t - max`` itself and of the final subtraction (a target 160 below
the maximum has an fp32 spacing of 2^-16)."""
import math

import torch

KINDS = ("normal", "flat", "peaked", "wide", "ties", "neginf")
SMALL = (1, 2, 27, 63, 64, 65, 255, 256, 257, 1024, 1025)  # both sides of the kernel's thresholds at 64 and 1024
LARGE = (4097, 8193)                                         # ... and at 8192
HUGE = 65613                                                 # `normal` and `ties` only
SMALL_ROWS = (1, 3, 4, 5, 257)                               # 4 rows per workgroup in the wave form
LARGE_ROWS = (3,)
FLAT_VALUE = 1.5


def tolerance(cols: int, ref: torch.Tensor) -> torch.Tensor:
    return (math.ceil(cols / 256) + 56) * 2.0 ** -23 + 2.0 ** -22 * ref.abs()


def neginf_columns(cols: int) -> torch.Tensor:
    """The columns the ``neginf`` kind sets to ``-inf``: a third of them (none at V = 1)."""
    return torch.arange(cols) % 3 == 1


def make_logits(kind: str, rows: int, cols: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    if kind == "normal":
        return x * 4
    if kind == "flat":
        return torch.full((rows, cols), FLAT_VALUE)
    if kind == "peaked":
        peak = torch.randint(0, cols, (rows,), generator=g)
        x[torch.arange(rows), peak] = x.max(dim=-1).values + 30
        return x
    if kind == "wide":
        return x * 40
    if kind == "ties":
        return torch.round(x * 2) / 2
    if kind == "neginf":
        x = x * 4
        x[:, neginf_columns(cols)] = -math.inf
        return x
    raise ValueError(kind)


def make_targets(kind: str, rows: int, cols: int, seed: int) -> torch.Tensor:
    """int64 ``[rows]``. ``neginf``: finite columns, except the last row (of two or more), whose target is ``-inf``;
    ``peaked``: row 0 asks for the peak itself."""
    g = torch.Generator().manual_seed(seed + 1000)
    t = torch.randint(0, cols, (rows,), generator=g)
    if kind == "neginf" and cols >= 2:
        finite = torch.nonzero(~neginf_columns(cols)).reshape(-1)
        t = finite[torch.randint(0, finite.numel(), (rows,), generator=g)]
        if rows >= 2:
            t[-1] = 1
    if kind == "peaked":
        t[0] = make_logits(kind, rows, cols, seed)[0].argmax()
    return t


def cases() -> list:
    """``(name, kind, rows, cols, seed)``: every kind at every small and large width, at every row count of its
    class; ``normal`` and ``ties`` at 65,613 columns."""
    out = []
    for kind in KINDS:
        for cols in SMALL + LARGE:
            for rows in (SMALL_ROWS if cols in SMALL else LARGE_ROWS):
                out.append((f"{kind}-{rows}x{cols}", kind, rows, cols, 17 * cols + rows))
    for kind in ("normal", "ties"):
        out.append((f"{kind}-3x{HUGE}", kind, 3, HUGE, 5))
    return out
