"""Fixed-seed inputs and the fp64 analysis shared by ``test_top_p_cpu.py`` and ``test_top_p_gpu.py``.

Tolerances of the comparison of ``pz::sample_rows`` with ``PF.sample_rows_reference``.

``EPS`` (the CDF clause) is the bound of ``test_sample_gpu.py`` for the same weights and the same
summation order: at most 80 dependent fp32 additions, ``80 * 2^-24 = 4.8e-6``, plus the error of
``exp``; rounded up, ``1e-5``.

``eps_p(V)`` (the nucleus clause) bounds, relative to the kept mass ``S0``, the error of the kernel's
integer masses ``m_c = floor(w_c * 2^32)`` against the fp64 weights:

* the kernel computes ``x = (l_c - max) / T`` in fp32 with two correctly rounded operations and
  ``__expf(x) = exp2(x * log2 e)`` with a rounded constant and a rounded product before a hardware
  ``exp2`` of 1 ulp: four roundings of the argument, ``4 * 2^-24`` relative. A relative error ``d`` of
  the argument is a relative error ``|x| d`` of the weight, so a weight is off by at most
  ``(4 |x| + 2) * 2^-24`` of itself;
* the columns at depth ``x`` weigh at most ``min(S0, V e^x)`` together (``S0 >= 1``: the maximum weighs 1),
  so relative to ``S0`` a sum of weights is off by at most ``(4 ln V + 2) * 2^-24``: ``2.8e-6`` at
  V = 65,613. The mass above a column and ``top_p * S0`` both carry it: ``5.6e-6``, rounded up to the
  ``1e-5`` the existing tests use for these weights;
* truncation to the fixed-point quantum loses less than ``2^-32`` per column, ``V * 2^-32`` in all;
  ``top_p`` as fp32 and the fp64 product add ``6e-8``, inside the rounding up above.

So ``eps_p(V) = 1e-5 + V * 2^-32``: ``1e-5`` up to a few thousand columns, ``2.5e-5`` at 65,613. The same
relative bound serves the min-p comparison ``w < min_p`` (one weight, no sum).

A draw is *ambiguous* when the fp64 reference alone cannot name the token within these bounds:
its row has a column whose strictly-above mass lies within ``eps_p * S0`` of ``top_p * S0`` or whose
weight lies within ``eps_p`` (relative) of ``min_p``, or its ``u`` lies within ``EPS`` of an edge of
the reference token's CDF interval. ``ambiguous_draws`` counts them; the GPU test may pass by a
boundary clause only where a draw is ambiguous, so the caps proven here on the CPU bound the GPU
test's use of the clauses."""
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF

SEED = (11, 22)
EPS = 1e-5
STEPS = 4
SMALL = (1, 2, 27, 63, 64, 65)
LARGE = (4097, 8192, 8193)  # 8192: the last column count on 4 waves, 8193: the first on 16
LARGEST = 65613
FLAT = (4097, 8193)                   # widths of the flat rows, on 4 and on 16 waves
FLAT_OPTION = (0.5, None, None, 1.0)  # (top_p, min_p, top_k, temperature) of the flat rows
KINDS = ("gauss", "heavy", "ties", "neginf")
OPTIONS = [  # (top_p, min_p, top_k, temperature)
    (0.9, None, None, 1.0), (0.5, None, None, 0.5), (0.05, None, None, 3.0), (0.999, None, None, 0.5),
    (None, 0.01, None, 1.0), (None, 0.3, None, 3.0), (0.9, 0.01, None, 0.5), (0.5, None, 5, 1.0),
    (0.9, None, 50, 3.0), (0.999, 0.3, 1, 1.0), (0.5, 0.01, 50, 0.5), (0.05, 0.3, 5, 1.0),
]
CAP_DRAWS = 0.02  # of a case's draws
CAP_CASES = 0.05  # of the cases

# the hand-checkable row: probabilities 1/2, 1/4, 1/8, 1/16, 1/16 at columns 3, 0, 4, 1, 2
HAND_PROBS = [1 / 4, 1 / 16, 1 / 16, 1 / 2, 1 / 8]
HAND_ORDER = [3, 0, 4, 1, 2]  # columns, most likely first


def eps_p(cols: int) -> float:
    return 1e-5 + cols * 2.0 ** -32


def hand_row() -> torch.Tensor:
    return torch.tensor(HAND_PROBS, dtype=torch.float64).log().float()


def make_logits(kind: str, rows: int, cols: int, seed: int) -> torch.Tensor:
    """fp32 logits [rows, cols]. Large rows are peaked (a wide Gaussian) so that the nucleus edge falls among
    heavy columns: the share of rows with a column within eps_p of the edge grows with eps_p / (weight at
    the edge), and the caps leave room for about one such row per case. ``flat`` is the exception: a Gaussian
    of scale 2 whose nucleus at top_p = 0.5 spans about 90 columns of 4097 and 190 of 8193, so that the mass
    select runs over many comparable columns; its seeds are chosen (SEEDS) so that no row is ambiguous."""
    g = torch.Generator().manual_seed(seed)
    scale = 2.0 if kind == "flat" else 3.0 if cols <= 65 else 8.0
    lg = scale * torch.randn(rows, cols, generator=g)
    if kind == "heavy":
        lg = torch.randn(rows, cols, generator=g)
        for j in range(min(3, cols)):
            at = torch.randint(0, cols, (rows,), generator=g)
            lg[torch.arange(rows), at] += 6.0 + 4.0 * torch.rand(rows, generator=g) + j
    elif kind == "ties":  # a coarse grid: runs of exactly equal logits everywhere, also across the nucleus edge
        lg = (lg * (2.0 if cols <= 65 else 0.5)).round() / (2.0 if cols <= 65 else 0.5)
    elif kind == "neginf":
        gone = torch.rand(rows, cols, generator=g) < 0.3
        gone[torch.arange(rows), torch.arange(rows) % cols] = False  # every row keeps a finite column
        lg = lg.masked_fill(gone, float("-inf"))
    return lg.float()


def cases():
    """[(name, kind, rows, cols, seed, dict(temperature, top_k, top_p, min_p))]: every small width with every
    option set, every large width with every kind of logits, the largest width once, and the flat rows."""
    out = []

    def add(kind, rows, cols, opt, seed):
        top_p, min_p, top_k, temperature = opt
        kw = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p)
        out.append((f"V{cols}-{kind}-p{top_p}-m{min_p}-k{top_k}-T{temperature}", kind, rows, cols, seed, kw))

    for vi, cols in enumerate(SMALL):
        for oi, opt in enumerate(OPTIONS):
            add(KINDS[(oi + vi) % 4], 64, cols, opt, SEEDS.get((cols, oi), 100 * vi + oi))
    for vi, cols in enumerate(LARGE):
        for ki, kind in enumerate(KINDS):
            oi = (5 * vi + 3 * ki) % len(OPTIONS)
            add(kind, 64, cols, OPTIONS[oi], SEEDS.get((cols, oi), 1000 + 10 * vi + ki))
    add("gauss", 4, LARGEST, OPTIONS[8], SEEDS.get((LARGEST, 8), 2000))
    for cols in FLAT:
        add("flat", 64, cols, FLAT_OPTION, SEEDS[(cols, "flat")])
    return out


# (columns, option index) -> generator seed, changed from the default where the fp64 reference alone found
# more ambiguous draws than the caps allow (top_p = 0.999 puts the edge among light columns)
SEEDS = {(63, 3): 5305, (64, 3): 5416, (65, 3): 5521, (4097, 3): 6003,
         # the flat rows: about two of 64 rows would be ambiguous at an arbitrary seed (2 eps_p / the edge column's share)
         (4097, "flat"): 7098, (8193, "flat"): 11201}


def analyse(lg: torch.Tensor, temperature, top_k=None, top_p=None, min_p=None, slack=0.0):
    """The fp64 rule on fp32 logits: ``(nucleus, wide, ambiguous_rows)``. ``nucleus [rows, V]`` is the
    reference's kept set; ``wide`` is it widened by the ambiguous columns (by every column that
    passed top-k and min-p where an ambiguous min-p column moves ``S0`` under top-p, since then the edge
    may fall anywhere); ``ambiguous_rows [rows]``. ``slack`` widens eps_p where the logits themselves
    carry an error."""
    l64 = lg.double()
    rows, v = l64.shape
    e = eps_p(v) + slack
    kept = torch.ones_like(l64, dtype=torch.bool)
    if top_k and top_k < v:
        kept = l64 >= torch.topk(l64, top_k, dim=-1).values[:, -1:]
    t32 = float(torch.tensor(temperature, dtype=torch.float32))
    w = torch.exp((l64 - l64.max(-1, keepdim=True).values) / t32)
    amb = torch.zeros_like(kept)
    if min_p:
        amb = kept & ((w - min_p).abs() <= e * min_p)
        kept = kept & ~(w < min_p)
    floating = amb.any(-1, keepdim=True) & bool(top_p is not None and top_p < 1)
    nucleus = kept
    if top_p is not None and top_p < 1:
        ls, order = l64.sort(dim=-1, descending=True, stable=True)
        ws = torch.where(kept, w, torch.zeros_like(w)).gather(1, order)
        excl = ws.cumsum(-1) - ws
        first = torch.ones_like(kept)
        first[:, 1:] = ls[:, 1:] != ls[:, :-1]
        above_sorted = torch.where(first, excl, torch.zeros_like(excl)).cummax(-1).values
        above = torch.zeros_like(w).scatter(1, order, above_sorted)
        s0 = ws.sum(-1, keepdim=True)
        amb = amb | (kept & ((above - top_p * s0).abs() <= e * s0))
        nucleus = kept & (above < top_p * s0)
    wide = nucleus | amb | (floating & (kept | amb))
    return nucleus, wide, amb.any(-1)


def _cdf(lg, nucleus, temperature):
    l64 = lg.double()
    t32 = float(torch.tensor(temperature, dtype=torch.float32))
    w = torch.where(nucleus, torch.exp((l64 - l64.max(-1, keepdim=True).values) / t32), torch.zeros_like(l64))
    return w.cumsum(-1) / w.sum(-1, keepdim=True)


def reference_tokens(lg, steps, opts, row0=0, first_step=0, seed=SEED):
    return torch.stack([PF.sample_rows_reference(lg, seed, first_step + s, row0=row0, **opts) for s in range(steps)], dim=1)


def ambiguous_draws(lg, steps, opts) -> int:
    """Draws of ``steps`` steps that the fp64 reference alone cannot name (module docstring)."""
    nucleus, _, amb_rows = analyse(lg, **opts)
    rows = lg.shape[0]
    if opts["temperature"] == 0:
        return 0
    cdf = _cdf(lg, nucleus, opts["temperature"])
    ref = reference_tokens(lg, steps, opts)
    count = 0
    for s in range(steps):
        for r in range(rows):
            if bool(amb_rows[r]):
                count += 1
                continue
            t = int(ref[r, s])
            u = PF.sample_uniform(SEED, r, s)
            below = cdf[r, :t][nucleus[r, :t]]
            lo = float(below[-1]) if below.numel() else None  # the lower edge 0 of the first kept column is no boundary
            hi = float(cdf[r, t]) if bool(nucleus[r, t + 1:].any()) else None
            if (lo is not None and abs(u - lo) <= EPS) or (hi is not None and abs(u - hi) <= EPS):
                count += 1
    return count


def check_draws(lg, got, opts, first_step=0, slack=0.0, seed=SEED) -> int:
    """Every token of ``got [rows, steps]`` against the reference under the two clauses; returns how many
    passed by a clause. With no tolerance at all: a token lies in the reference's nucleus, widened only
    in ambiguous rows. Column ``j`` of ``got`` is step ``first_step + j``; ``slack`` is added to both bounds."""
    nucleus, wide, amb_rows = analyse(lg, slack=slack, **opts)
    rows = lg.shape[0]
    cdf = _cdf(lg, nucleus, opts["temperature"])
    ref = reference_tokens(lg, got.shape[1], opts, first_step=first_step, seed=seed)
    near = 0
    for s in range(got.shape[1]):
        assert bool(wide[torch.arange(rows), got[:, s]].all()), f"step {s}: a token outside the nucleus"
        for r in (got[:, s] != ref[:, s]).nonzero().flatten().tolist():
            near += 1
            if bool(amb_rows[r]):  # the nucleus clause: inside the widened nucleus (checked above)
                continue
            t, want = int(got[r, s]), int(ref[r, s])
            lo, hi = min(t, want), max(t, want)
            assert not bool(nucleus[r, lo + 1:hi].any()), (s, r, t, want, "not the kept neighbour")
            u = PF.sample_uniform(seed, r, first_step + s)
            assert abs(float(cdf[r, lo]) - u) <= EPS + slack, (s, r, t, want, float(cdf[r, lo]), u)
    return near
