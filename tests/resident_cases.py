"""Cases for the op-level tests of ``pz::generate_resident`` (csrc/generate_resident.hip): hand-written
stage lists, integer-valued parameters, an exact fp64 reference, and a restatement of the kernel's
rule for how a linear stage is spread over its 256 threads. Pure torch on the CPU: shared by
tests/test_resident_exact_cpu.py and tests/test_resident_exact_gpu.py.

Why the reference is exact. The table, the weights and the biases are small integers and the
batchnorm parameters are chosen so that ``1 / sqrt(var + eps)`` is exactly 2, 1 or 0.5 and the gain
+-0.5, +-1 or +-2: every value a stage reads is a multiple of 2^-2, and so is every product and every
partial sum. :func:`reference_logits` asserts that ``(|h| @ |w| + |bias|) * 4 < 2^24`` in every
linear stage: whatever the order, each fp32 partial sum is then a multiple of 2^-2 below 2^22 in
magnitude, which fp32 holds exactly. So the kernel's sums carry no rounding at all, the only
roundings are the ones to the compute dtype after each hidden stage, and an fp64 forward with those
roundings gives the kernel's bits.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import torch

from penr_oz_neural_network_torch_amd.engine.resident import StageDesc, resident_plan

NONE, RELU = 0, 1
BN_EPS = 2.0 ** -10
DTYPES = {"bfloat16": torch.bfloat16, "float32": torch.float32}
KNT, WAVE = 256, 64  # generate_resident.hip: kNT threads per row, kWave


def F(r):
    return StageDesc("flatten", ratio=r)


def G(k, n, act=NONE, bias=True):
    return StageDesc("gemm", k, n, act=act, bias=bias)


def B(n, act=NONE):
    return StageDesc("bn", n, n, act=act, eps=BN_EPS)


@dataclass(frozen=True)
class Case:
    name: str
    L: int
    vocab: int
    E: int
    body: tuple
    wmax: int = 2      # weights are integers in [-wmax, wmax]
    seed: int = 0

    @property
    def stages(self):
        return [StageDesc("embed", 0, self.E, vocab=self.vocab)] + list(self.body)

    @property
    def V(self):
        return self.body[-1].out_width

    @property
    def steps(self):
        return max(20, 2 * self.L + 3)


CASES = {c.name: c for c in [
    # K < S, three empty groups, V = 1
    Case("one", 1, 1, 1, (G(1, 1),), seed=1),
    # O = 64 exactly; K = 5 over S = 4: [0,2) [2,4) [4,5) [5,5)
    Case("ragged", 1, 11, 5, (G(5, 64, RELU), G(64, 9)), seed=2),
    # K = 1 under S = 4; K = 33 ragged; O = 70: S = 2, kc = 1
    Case("tinyK", 1, 70, 1, (G(1, 33), G(33, 2, RELU), G(2, 70)), seed=3),
    # K = 3 and 7 under S = 4
    Case("k3", 3, 13, 1, (F(3), G(3, 7, RELU), G(7, 13)), seed=4),
    # opad = 128 at O = 65 and 128; odd K = 65 over two groups; opad = 192 at O = 130
    Case("s2", 2, 130, 7, (F(2), G(14, 65, RELU), G(65, 128, NONE, False), G(128, 5, RELU), G(5, 130)), seed=5),
    # O = 192, 255 (opad = 256), 256 (loop, no tail), 257 (tail of 1); seven linear stages: both buffer parities
    Case("edges", 2, 257, 3, (F(2), G(6, 192, RELU), G(192, 8, RELU), G(8, 255, RELU), G(255, 8, RELU, False),
                              G(8, 256, RELU), G(256, 4), G(4, 257)), wmax=1, seed=6),
    # P = 8 and 4 in split stages; batchnorm over 4 positions; a ring of 8
    Case("positions", 8, 31, 3, (G(3, 5, RELU), F(2), G(10, 33, NONE, False), B(33, RELU), F(4), G(132, 31)), seed=7),
    # the strided loop with P = 6, O = 300 (tail 44, o / N crossing positions); batchnorm over 6 positions
    Case("wide_p", 6, 40, 4, (G(4, 50, RELU), B(50), F(3), G(150, 64, RELU), F(2), G(128, 40)), seed=8),
    # V = 8192 = kSampleNarrowCols; about 9 distinct logit values per row: massive ties
    Case("vmax", 2, 8192, 1, (F(2), G(2, 3, RELU), G(3, 8192, NONE, False)), seed=9),
]}
# cases whose fp32 table does not fit next to the rest: the planner leaves it in global memory
TABLE_GLOBAL = {("vmax", "float32")}


def case_shapes(case: Case):
    """``(kind, P, K, N, stage)`` per body stage, as the planner derives them: [P, N] is the stage's output."""
    pos, width, out = case.L, case.E, []
    for st in case.body:
        if st.kind == "flatten":
            assert pos % st.ratio == 0
            pos, width = pos // st.ratio, width * st.ratio
            out.append(("flatten", pos, st.ratio, width, st))
        elif st.kind == "gemm":
            assert st.in_width == width
            out.append(("gemm", pos, width, st.out_width, st))
            width = st.out_width
        else:
            assert st.kind == "bn" and st.out_width == width
            out.append(("bn", pos, width, width, st))
    assert pos == 1 and width == case.V
    return out


def regimes(P: int, K: int, N: int):
    """How generate_resident.hip spreads a linear stage of ``P`` positions, ``K`` inputs and ``N`` outputs
    over its 256 threads, restated: ``("loop", O, O % 256)`` where ``O = P N >= 256`` (thread ``t`` takes
    outputs ``t, t + 256, ...``, each over all of ``K``), else ``("split", opad, S, kc, ranges)``: ``S =
    256 // opad`` groups of ``opad = roundup(O, 64)`` threads, group ``g`` summing ``ranges[g] = [min(K, g kc),
    min(K, (g + 1) kc))`` with ``kc = ceil(K / S)``."""
    O = P * N
    if O >= KNT:
        return ("loop", O, O % KNT)
    opad = -(-O // WAVE) * WAVE
    S = KNT // opad
    kc = -(-K // S)
    return ("split", opad, S, kc, [(min(K, g * kc), min(K, (g + 1) * kc)) for g in range(S)])


def case_regimes(case: Case):
    """``(P, K, N, bias, regimes(P, K, N))`` of every linear stage of the case."""
    return [(p, k, n, st.bias, regimes(p, k, n)) for kind, p, k, n, st in case_shapes(case) if kind == "gemm"]


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _pick(g, values, n):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), (n,), generator=g)]


@functools.lru_cache(maxsize=None)
def make_params(name: str) -> dict:
    """fp64 parameters of a case from a seeded CPU generator, keyed as ``ResidentPlan.params`` names them:
    ``(0, "table")``, then ``(stage, role)`` with the body's stages counted from 1. Callers must not
    modify them."""
    case = CASES[name]
    g = torch.Generator(device="cpu").manual_seed(1000 + case.seed)
    out = {(0, "table"): _ints(g, -3, 3, case.vocab, case.E)}
    for i, (kind, p, k, n, st) in enumerate(case_shapes(case), start=1):
        if kind == "gemm":
            out[(i, "weights")] = _ints(g, -case.wmax, case.wmax, k, n)
            if st.bias:
                out[(i, "bias")] = _ints(g, -4, 4, n)
        elif kind == "bn":
            out[(i, "gain")] = _pick(g, [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], n)
            out[(i, "bias")] = _ints(g, -4, 4, n)
            out[(i, "mean")] = _ints(g, -3, 3, n)
            out[(i, "var")] = _pick(g, [0.25, 1.0, 4.0], n) - BN_EPS  # exact in fp32: var + eps is 0.25, 1 or 4
    return out


def plans(case: Case, dtype: str) -> dict:
    """``{"lds": plan, "lean": plan}``: the planner's own plan and the one with the table pushed to global
    memory (``budget = total - 1``). Where the planner already leaves the table outside there is no second
    plan, and the only one is under ``"lean"``."""
    full = resident_plan(case.stages, dtype, case.L)
    assert not isinstance(full, str), (case.name, dtype, full)
    if not full.table_in_lds:
        return {"lean": full}
    lean = resident_plan(case.stages, dtype, case.L, budget=full.total - 1)
    assert not isinstance(lean, str), (case.name, dtype, lean)
    return {"lds": full, "lean": lean}


def placements():
    """Every (case name, dtype name, placement) there is a plan for."""
    return [(n, d, p) for n in CASES for d in DTYPES for p in (("lean",) if (n, d) in TABLE_GLOBAL else ("lds", "lean"))]


def param_tensors(values: dict, plan, dtype: str, device) -> list:
    """The kernel's tensors in the order of ``plan.params``: weights in the compute dtype, the rest fp32."""
    out = []
    for key in plan.params:
        t = values[key].to(DTYPES[dtype] if key[1] == "weights" else torch.float32)
        assert torch.equal(t.double(), values[key].double()), key  # (the dtype holds the value)
        out.append(t.contiguous().to(device))
    return out


def wrap_ids(ids: torch.Tensor, vocab: int) -> torch.Tensor:
    """Ids as the kernel's prologue reads them: negative ones count from the end, and what is still
    outside ``[0, vocab)`` becomes -1, the row of zeros."""
    ids = torch.where(ids < 0, ids + vocab, ids)
    return torch.where((ids >= 0) & (ids < vocab), ids, torch.full_like(ids, -1))


def _quarter(t: torch.Tensor) -> bool:
    return bool(torch.equal(t * 4, (t * 4).round()))


def reference_logits(case: Case, params: dict, windows: torch.Tensor, dtype, rounded: bool = True) -> torch.Tensor:
    """fp64 logits ``[rows, V]`` of ``windows`` (int64 ``[rows, L]``, already wrapped: -1 reads a row of
    zeros) with one rounding to ``dtype`` after every hidden stage (and of the embedding, which the
    kernel stores in the compute dtype too); the last stage stays unrounded. ``rounded=False`` leaves
    the roundings out. Asserts the conditions under which the kernel must give these very bits
    (module docstring)."""
    dtype = DTYPES.get(dtype, dtype)

    def rnd(h):
        return h.to(dtype).double() if rounded else h

    windows = torch.as_tensor(windows, dtype=torch.int64)
    rows = windows.shape[0]
    assert windows.shape == (rows, case.L) and int(windows.min()) >= -1 and int(windows.max()) < case.vocab
    table = params[(0, "table")]
    assert _quarter(table)
    h = torch.where((windows >= 0).unsqueeze(-1), table[windows.clamp_min(0)], torch.zeros((), dtype=torch.float64))
    h = rnd(h)  # [rows, L, E]
    shapes = case_shapes(case)
    for i, (kind, p, k, n, st) in enumerate(shapes, start=1):
        assert _quarter(h), (case.name, i, "a stage input is no multiple of 2^-2")
        if kind == "flatten":
            h = h.reshape(rows, p, n)
            continue
        assert h.shape == (rows, p, k)
        if kind == "gemm":
            w = params[(i, "weights")]
            bias = params.get((i, "bias"))
            assert _quarter(w) and (bias is None or _quarter(bias)) and (bias is not None) == st.bias
            bound = h.abs() @ w.abs() + (bias.abs() if bias is not None else 0.0)
            assert float(bound.max()) * 4 < 2 ** 24, (case.name, i, float(bound.max()))
            h = h @ w
            if bias is not None:
                h = h + bias
        else:
            gain, bias, mean, var = (params[(i, r)] for r in ("gain", "bias", "mean", "var"))
            assert _quarter(gain) and _quarter(bias) and _quarter(mean)
            assert torch.equal(var.float().double(), var), "the running variance must be exact in fp32"
            inv = 1.0 / torch.sqrt(var + st.eps)
            assert bool(((inv == 2.0) | (inv == 1.0) | (inv == 0.5)).all())
            bound = gain.abs() * ((h.abs() + mean.abs()) * inv) + bias.abs()
            assert float(bound.max()) * 4 < 2 ** 24  # (the kernel goes through fp32 on its way to the compute dtype)
            h = gain * ((h - mean) * inv) + bias
        assert st.act in (NONE, RELU)
        if st.act == RELU:
            h = h.clamp_min(0)
        if i < len(shapes):
            h = rnd(h)
    return h.reshape(rows, case.V)


def plain_logits(case: Case, params: dict, windows: torch.Tensor) -> torch.Tensor:
    """A straightforward fp64 forward written apart from :func:`reference_logits`: no roundings, no checks."""
    windows = torch.as_tensor(windows, dtype=torch.int64)
    table = torch.cat([params[(0, "table")], torch.zeros(1, case.E, dtype=torch.float64)])  # (row -1: zeros)
    h = table[windows]
    for i, st in enumerate(case.body, start=1):
        if st.kind == "flatten":
            h = h.reshape(h.shape[0], h.shape[1] // st.ratio, h.shape[2] * st.ratio)
        elif st.kind == "gemm":
            h = torch.einsum("rpk,kn->rpn", h, params[(i, "weights")])
            if st.bias:
                h = h + params[(i, "bias")]
        else:
            h = (h - params[(i, "mean")]) / torch.sqrt(params[(i, "var")] + st.eps) * params[(i, "gain")] + params[(i, "bias")]
        if st.act == RELU:
            h = torch.relu(h)
    return h.reshape(h.shape[0], case.V)


# ways a kernel of this shape goes subtly wrong, for emulate_logits: the cases must tell each from the truth
MUTANTS = ("drop_k", "repeat_k", "bias_o", "bn_channel", "no_round", "loop_tail", "no_swap")


def emulate_logits(case: Case, params: dict, windows: torch.Tensor, dtype, mutant: str | None = None) -> torch.Tensor:
    """The kernel's own indexing restated on two flat ping-pong buffers: output ``o = p N + n``, the K groups
    of :func:`regimes` summed one by one, ``i % N`` in batchnorm, a swap after every hidden linear stage.
    Without a ``mutant`` it must give :func:`reference_logits`. With one it is wrong in one small way:

    * ``drop_k`` / ``repeat_k``: group 0 stops one ``k`` short / group 1 starts one ``k`` early;
    * ``bias_o``: ``bias[o]`` (clamped to the vector) instead of ``bias[n]``: the same wherever ``P = 1``;
    * ``bn_channel``: batchnorm column ``i / P`` instead of ``i % N``;
    * ``no_round``: hidden values are not rounded to the compute dtype;
    * ``loop_tail``: the strided loop leaves out the outputs past the last whole 256;
    * ``no_swap``: the buffers are not swapped after the second hidden linear stage.

    The tests use it to show that the cases' numbers expose each of these (a condition on the inputs)."""
    assert mutant is None or mutant in MUTANTS
    dtype = DTYPES.get(dtype, dtype)

    def rnd(h):
        return h if mutant == "no_round" else h.to(dtype).double()

    rows = windows.shape[0]
    shapes = case_shapes(case)
    widest = max([case.L * case.E] + [p * n for kind, p, k, n, st in shapes[:-1]])
    table = torch.cat([params[(0, "table")], torch.zeros(1, case.E, dtype=torch.float64)])
    cur, nxt = torch.zeros(rows, widest, dtype=torch.float64), torch.zeros(rows, widest, dtype=torch.float64)
    cur[:, :case.L * case.E] = table[windows].to(dtype).double().reshape(rows, -1)
    swaps, logits = 0, torch.zeros(rows, case.V, dtype=torch.float64)
    for i, (kind, p, k, n, st) in enumerate(shapes, start=1):
        if kind == "flatten":
            continue
        O = p * n
        o = torch.arange(O)
        if kind == "bn":
            c = o // p if mutant == "bn_channel" else o % n
            gain, bias, mean, var = (params[(i, r)] for r in ("gain", "bias", "mean", "var"))
            v = gain[c] * ((cur[:, :O] - mean[c]) * (1.0 / torch.sqrt(var[c] + st.eps))) + bias[c]
            cur[:, :O] = rnd(v.clamp_min(0) if st.act == RELU else v)
            continue
        x, w = cur[:, :p * k].reshape(rows, p, k), params[(i, "weights")]
        reg, live = regimes(p, k, n), O
        if reg[0] == "loop":
            ranges = [(0, k)]
            live = O - reg[2] if mutant == "loop_tail" else O
        else:
            ranges = list(reg[4])
            if mutant == "drop_k" and reg[2] > 1 and ranges[0][1] > ranges[0][0]:
                ranges[0] = (ranges[0][0], ranges[0][1] - 1)
            if mutant == "repeat_k" and reg[2] > 1 and ranges[1][1] > ranges[1][0]:
                ranges[1] = (ranges[1][0] - 1, ranges[1][1])
        acc = torch.zeros(rows, p, n, dtype=torch.float64)
        for k0, k1 in ranges:
            acc = acc + x[:, :, k0:k1] @ w[k0:k1]
        acc = acc.reshape(rows, O)
        if st.bias:
            acc = acc + params[(i, "bias")][o.clamp(max=n - 1) if mutant == "bias_o" else o % n]
        if st.act == RELU:
            acc = acc.clamp_min(0)
        if i == len(shapes):
            logits[:, :live] = acc[:, :live]
        else:
            nxt[:, :live] = rnd(acc)[:, :live]
            swaps += 1
            if not (mutant == "no_swap" and swaps == 2):
                cur, nxt = nxt, cur
    return logits


def lowest_argmax(logits: torch.Tensor) -> torch.Tensor:
    """The lowest index among the maxima of each row."""
    v = logits.shape[-1]
    idx = torch.arange(v).expand_as(logits)
    return torch.where(logits == logits.max(-1, keepdim=True).values, idx, v).min(-1).values


def contexts(case: Case, rows: int = 4, seed: int = 0) -> torch.Tensor:
    """int64 ``[rows, L]`` ids in ``[0, vocab)`` from a seeded CPU generator."""
    g = torch.Generator(device="cpu").manual_seed(77 + 13 * case.seed + seed)
    return torch.randint(0, case.vocab, (rows, case.L), generator=g)


def greedy_tokens(case: Case, dtype, ctx: torch.Tensor, steps: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Free-running greedy generation from the reference alone: ``(tokens [rows, steps], logits [rows, steps, V])``,
    each token the lowest index among the maxima of the reference logits of the window before it."""
    params = make_params(case.name)
    seq = torch.cat([ctx, torch.zeros(ctx.shape[0], steps, dtype=torch.int64)], dim=1)
    logits = []
    for s in range(steps):
        lg = reference_logits(case, params, wrap_ids(seq[:, s:s + case.L], case.vocab), dtype)
        seq[:, case.L + s] = lowest_argmax(lg)
        logits.append(lg)
    return seq[:, case.L:], torch.stack(logits, dim=1)


@functools.lru_cache(maxsize=None)
def stop_scenario(dtype: str, steps: int = 600):
    """Contexts for the stop test on ``k3``, found by running the reference's greedy generation on all
    13^3 contexts: ``(ctx [4, 3], stop_token, free tokens [4, steps], free logits [4, steps, V])`` with

    * row 0: the token of step 2 (the stop token) is not drawn at steps 0 and 1;
    * row 1: any context (the test launches it as done);
    * row 2: never draws the stop token in ``steps`` steps;
    * row 3: draws the stop token for the first time after step 2 (so a second row is cut, elsewhere).

    The first contexts in id order that qualify are taken; the search fails loudly if there are none."""
    case = CASES["k3"]
    ids = torch.arange(case.vocab)
    every = torch.cartesian_prod(ids, ids, ids)
    tokens, _ = greedy_tokens(case, dtype, every, steps)
    for r0 in range(every.shape[0]):
        stop = int(tokens[r0, 2])
        if stop in tokens[r0, :2].tolist():
            continue
        has = (tokens == stop).any(dim=1)
        first = torch.where(tokens == stop, torch.arange(steps).expand_as(tokens), steps).min(dim=1).values
        never = (~has).nonzero().flatten().tolist()
        late = ((first > 2) & has).nonzero().flatten().tolist()
        late = [r for r in late if r != r0]
        if never and late:
            rows = [r0, (r0 + 1) % every.shape[0], never[0], late[0]]
            assert len(set(rows)) == 4
            ctx = every[rows].clone()
            free, logits = greedy_tokens(case, dtype, ctx, steps)
            assert torch.equal(free, tokens[rows])
            return ctx, stop, free, logits
    raise AssertionError("no context of k3 gives the stop scenario: change the case's seed")


# the real-valued stage of the precision test: L = 2, E = 8, flatten by 2, one linear stage of 16 inputs
REAL_K, REAL_V = 16, 40
REAL_CASE = Case("real", 2, REAL_V, 8, (F(2), G(REAL_K, REAL_V)), seed=10)


def real_params(dtype) -> dict:
    """Normal-distributed fp32 table, weights (cast to ``dtype``) and bias of :data:`REAL_CASE`."""
    g = torch.Generator(device="cpu").manual_seed(4242)
    return {(0, "table"): torch.randn(REAL_V, 8, generator=g), (2, "weights"): torch.randn(REAL_K, REAL_V, generator=g).to(DTYPES[dtype]),
            (2, "bias"): torch.randn(REAL_V, generator=g)}


def real_reference(params: dict, windows: torch.Tensor, dtype) -> tuple[torch.Tensor, torch.Tensor]:
    """fp64 logits of :data:`REAL_CASE` on the operands as the kernel holds them (the embedding rounded to
    ``dtype``, the weights in ``dtype``, the bias in fp32) and the magnitude ``|x| |w| + |bias|`` of each."""
    x = params[(0, "table")][windows].to(DTYPES[dtype]).double().reshape(windows.shape[0], REAL_K)
    w, bias = params[(2, "weights")].double(), params[(2, "bias")].double()
    return x @ w + bias, x.abs() @ w.abs() + bias.abs()
