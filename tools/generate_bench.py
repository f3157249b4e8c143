#!/usr/bin/env python
"""Token generation throughput on the GPU (needs an MI355X; fails without a GPU).

Models (bfloat16, batchnorm statistics from one training-mode forward):
  chars: [27, 10, 30, 64, 27]           embedding, linear, batchnorm, tanh, linear, softmax (context 3)
  wide:  [4096, 64, 512, 4096, 4096]    the same layers, vocabulary 4096 (context 8)

1. Tokens per second at 1, 16 and 64 rows, ``TOKENS`` new tokens per row and call:
   * device loop: ``model.generate`` (engine/predictor.py: one upload, per token the forward kernels
     and one ``pz::sample_rows`` launch, one download);
   * host loop: what a caller had before ``generate`` existed — per token ``model.predict`` on the
     current windows, ``torch.multinomial`` on the returned probabilities, the windows shifted in
     Python.
   Both are the public API (Python lists in and out), timed by a host clock around a call that ends
   with its result on the host, in the same process, alternating, after a warm-up of both; median
   and interquartile range over the repeats.
2. ``pz::sample_rows`` alone: device-event time per launch over trains of back-to-back launches on
   fixed logits (L2-resident: the launch that precedes it in the loop has just written them), for
   V = 27, 4096 and 65536, with and without top-k.

3. ``--resident``: the one-launch form, ``model.generate(..., loop="resident")``
   (csrc/generate_resident.hip), against the device loop of 1. on the chars model in bfloat16 and
   float32 at 1, 16, 64 and 1024 rows: tokens per second through the public API, both ways, same
   process, alternating, after a warm-up of both; and the device-event time of the resident launch
   alone (trains of back-to-back ``PF.generate_resident`` launches) divided by the steps. Runs only
   this section and writes profiles/generate_resident_latency.txt.

4. ``--top-p``: nucleus sampling. ``pz::sample_rows`` alone as in 2. with ``top_p = 0.9``, alone and
   with ``top_k = 50``, next to the same launch without it and with ``top_k = 50`` only; then tokens
   per second of ``model.generate(top_p=0.9)``, per-token and (chars) ``loop="resident"``, against the
   loop a caller had for top-p before: per token ``model.predict``, then sort, cumulative sum and
   ``torch.multinomial`` on the host. Runs only this section and writes
   profiles/sample_top_p_latency.txt.

Usage: python tools/generate_bench.py [--out profiles/generate_latency.txt] [--quick] [--resident | --top-p]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel  # noqa: E402
from penr_oz_neural_network_torch_amd.ops import functional as PF  # noqa: E402
from penr_oz_neural_network_torch_amd.ops import native  # noqa: E402

ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]
MODELS = {"chars": [27, 10, 30, 64, 27], "wide": [4096, 64, 512, 4096, 4096]}
ROWS = [1, 16, 64]
TOKENS = 64


def _iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def _build(name: str, dtype: str = "bfloat16") -> NeuralNetworkModel:
    torch.manual_seed(0)
    sizes = MODELS[name]
    model = NeuralNetworkModel(f"generate_bench_{name}", sizes, activation_algos=ALGOS, bias_algo="random",
                               dtype=dtype, device="cuda:0")
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, sizes[0], (256, model.context_length), generator=g)
    model.compute_output(ids.tolist(), [[int(i)] for i in torch.randint(0, sizes[-1], (256,), generator=g)])
    return model


def host_loop(model, context: list, steps: int, generator: torch.Generator) -> list:
    """The per-token loop over the public ``predict``: sample on the host, shift the windows."""
    windows = [list(row) for row in context]
    out = [[] for _ in context]
    for _ in range(steps):
        probs = torch.tensor(model.predict(windows))
        picks = torch.multinomial(probs, 1, generator=generator)[:, 0].tolist()
        for row, window, token in zip(out, windows, picks):
            row.append(token)
            window.pop(0)
            window.append(token)
    return out


def model_throughput(name: str, quick: bool) -> list[str]:
    model = _build(name)
    assert model._fused_predictor() is not None, "the bench models must go through the fused predictor"
    length, vocab = model.context_length, MODELS[name][0]
    lines = [f"== {name} {MODELS[name]} bfloat16, context {length}, {TOKENS} new tokens per row and call: "
             "tokens/s, median [interquartile range] ==",
             f"{'rows':>5} | {'device loop (generate)':>28} {'ms/call':>9} | {'host loop (predict + multinomial)':>34} "
             f"{'ms/call':>9} | {'device / host':>13}"]
    g = torch.Generator().manual_seed(2)
    for rows in ROWS:
        context = torch.randint(0, vocab, (rows, length), generator=g).tolist()
        sampler = torch.Generator().manual_seed(3)
        seeds = iter(range(1, 1 << 30))
        reps = 5 if quick else 25
        for _ in range(2):  # warm-up of every shape the timed window uses
            model.generate(context, TOKENS, seed=next(seeds))
            host_loop(model, context, TOKENS, sampler)
        td, th = [], []
        for _ in range(reps):  # alternating; each call ends with its tokens on the host
            t0 = time.perf_counter()
            model.generate(context, TOKENS, seed=next(seeds))
            t1 = time.perf_counter()
            host_loop(model, context, TOKENS, sampler)
            t2 = time.perf_counter()
            td.append(t1 - t0)
            th.append(t2 - t1)
        n = rows * TOKENS
        rd, rh = [n / t for t in td], [n / t for t in th]
        lines.append(f"{rows:>5} | {statistics.median(rd):>17,.0f} [{_iqr(rd):>8,.0f}] {statistics.median(td) * 1e3:>9.3f} | "
                     f"{statistics.median(rh):>23,.0f} [{_iqr(rh):>8,.0f}] {statistics.median(th) * 1e3:>9.3f} | "
                     f"{statistics.median(rd) / statistics.median(rh):>12.2f}x")
    return lines + [""]


def host_loop_top_p(model, context: list, steps: int, generator: torch.Generator, top_p: float) -> list:
    """The per-token loop over the public ``predict`` with nucleus sampling on the host."""
    windows = [list(row) for row in context]
    out = [[] for _ in context]
    for _ in range(steps):
        probs = torch.tensor(model.predict(windows))
        sp, order = probs.sort(dim=-1, descending=True)
        sp = sp.masked_fill(sp.cumsum(-1) - sp >= top_p, 0.0)
        picks = order.gather(1, torch.multinomial(sp, 1, generator=generator))[:, 0].tolist()
        for row, window, token in zip(out, windows, picks):
            row.append(token)
            window.pop(0)
            window.append(token)
    return out


def top_p_throughput(name: str, quick: bool, top_p: float = 0.9) -> list[str]:
    model = _build(name)
    pred = model._fused_predictor()
    assert pred is not None, "the bench models must go through the fused predictor"
    resident = not isinstance(pred.resident_plan(), str)
    length, vocab = model.context_length, MODELS[name][0]
    lines = [f"== {name} {MODELS[name]} bfloat16, context {length}, {TOKENS} new tokens per row and call, top_p = {top_p}: "
             "tokens/s, median [interquartile range] ==",
             f"{'rows':>5} | {'generate(top_p)':>28} {'ms/call':>9} | {'generate(top_p, resident)':>28} {'ms/call':>9} | "
             f"{'host loop (predict + sort + cumsum)':>36} {'ms/call':>9} | {'loop / host':>11} | {'resident / host':>15}"]
    g = torch.Generator().manual_seed(2)
    for rows in ROWS:
        context = torch.randint(0, vocab, (rows, length), generator=g).tolist()
        sampler = torch.Generator().manual_seed(3)
        seeds = iter(range(1, 1 << 30))
        reps = 5 if quick else 25
        calls = [lambda: model.generate(context, TOKENS, seed=next(seeds), top_p=top_p),
                 (lambda: model.generate(context, TOKENS, seed=next(seeds), top_p=top_p, loop="resident")) if resident else None,
                 lambda: host_loop_top_p(model, context, TOKENS, sampler, top_p)]
        for _ in range(2):
            for call in calls:
                if call is not None:
                    call()
        times = [[] for _ in calls]
        for _ in range(reps):  # alternating; each call ends with its tokens on the host
            for t, call in zip(times, calls):
                if call is not None:
                    t0 = time.perf_counter()
                    call()
                    t.append(time.perf_counter() - t0)
        n = rows * TOKENS

        def cell(t, width):
            if not t:
                return f"{'(does not fit in LDS)':>{width + 11}} {'':>9}"
            r = [n / x for x in t]
            return f"{statistics.median(r):>{width},.0f} [{_iqr(r):>8,.0f}] {statistics.median(t) * 1e3:>9.3f}"

        med = [statistics.median(t) if t else None for t in times]
        lines.append(f"{rows:>5} | {cell(times[0], 17)} | {cell(times[1], 17)} | {cell(times[2], 25)} | "
                     f"{med[2] / med[0]:>10.2f}x | " + (f"{med[2] / med[1]:>14.2f}x" if med[1] else f"{'-':>15}"))
    return lines + [""]


RESIDENT_ROWS = [1, 16, 64, 1024]


def resident_throughput(dtype: str, quick: bool) -> list[str]:
    model = _build("chars", dtype)
    pred = model._fused_predictor()
    assert pred is not None and not isinstance(pred.resident_plan(), str), "the chars model must plan resident"
    plan = pred.resident_plan()
    length, vocab = model.context_length, MODELS["chars"][0]
    lines = [f"== chars {MODELS['chars']} {dtype}, context {length}, {TOKENS} new tokens per row and call; LDS plan "
             f"{plan.total} bytes per workgroup ==",
             "   tokens/s through model.generate (lists in and out), median [interquartile range]; launch: device-event",
             "   time of PF.generate_resident alone, per token",
             f"{'rows':>5} | {'device loop (loop=None)':>28} {'ms/call':>9} | {'one launch (loop=resident)':>28} {'ms/call':>9} | "
             f"{'resident / loop':>15} | {'launch us/token':>22}"]
    g = torch.Generator().manual_seed(2)
    for rows in RESIDENT_ROWS:
        context = torch.randint(0, vocab, (rows, length), generator=g).tolist()
        seeds = iter(range(1, 1 << 30))
        reps = 5 if quick else 25
        for _ in range(3):  # warm-up of both
            model.generate(context, TOKENS, seed=next(seeds))
            model.generate(context, TOKENS, seed=next(seeds), loop="resident")
        tl, tr = [], []
        for _ in range(reps):  # alternating; each call ends with its tokens on the host
            t0 = time.perf_counter()
            model.generate(context, TOKENS, seed=next(seeds))
            t1 = time.perf_counter()
            model.generate(context, TOKENS, seed=next(seeds), loop="resident")
            t2 = time.perf_counter()
            tl.append(t1 - t0)
            tr.append(t2 - t1)
        # the launch alone
        seq = torch.zeros(rows, length + TOKENS, device=pred.dev, dtype=torch.int64)
        seq[:, :length] = torch.tensor(context)
        done = torch.zeros(rows, device=pred.dev, dtype=torch.int32)
        params = pred.resident_params(plan)
        iters, trains = (5, 3) if quick else (20, 7)
        for i in range(3):
            PF.generate_resident(seq, done, params, plan.ints, TOKENS, seed=(5, i))
        torch.cuda.synchronize()
        times = []
        for t in range(trains):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                PF.generate_resident(seq, done, params, plan.ints, TOKENS, seed=(6 + t, i))
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / iters / TOKENS)
        n = rows * TOKENS
        rl, rr = [n / t for t in tl], [n / t for t in tr]
        lines.append(f"{rows:>5} | {statistics.median(rl):>17,.0f} [{_iqr(rl):>8,.0f}] {statistics.median(tl) * 1e3:>9.3f} | "
                     f"{statistics.median(rr):>17,.0f} [{_iqr(rr):>8,.0f}] {statistics.median(tr) * 1e3:>9.3f} | "
                     f"{statistics.median(rr) / statistics.median(rl):>14.2f}x | "
                     f"{statistics.median(times):>12.3f} [{_iqr(times):>7.3f}]")
    # where a token's time goes: the launch at 1 row by sampling mode, 64 against 256 steps (the difference
    # is 192 tokens without the launch's fixed cost: parameter copy, prologue, launch interval)
    lines += ["", "   the launch alone at 1 row by sampling mode: us per token from the difference of 256- and 64-step "
              "launches, and the fixed cost per launch that leaves",
              f"{'mode':>12} | {'us/token':>9} | {'fixed us/launch':>15}"]
    context = torch.randint(0, vocab, (1, length), generator=g)
    params = pred.resident_params(plan)

    def launch_us(steps: int, **kw) -> float:
        seq = torch.zeros(1, length + steps, device=pred.dev, dtype=torch.int64)
        seq[:, :length] = context
        done = torch.zeros(1, device=pred.dev, dtype=torch.int32)
        iters, trains = (5, 3) if quick else (20, 7)
        for i in range(3):
            PF.generate_resident(seq, done, params, plan.ints, steps, seed=(7, i), **kw)
        torch.cuda.synchronize()
        times = []
        for t in range(trains):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                PF.generate_resident(seq, done, params, plan.ints, steps, seed=(8 + t, i), **kw)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / iters)
        return statistics.median(times)

    for label, kw in (("greedy", dict(temperature=0.0)), ("T = 0.8", dict(temperature=0.8)),
                      ("top_k = 7", dict(temperature=1.0, top_k=7))):
        short, long_ = launch_us(TOKENS, **kw), launch_us(4 * TOKENS, **kw)
        per = (long_ - short) / (3 * TOKENS)
        lines.append(f"{label:>12} | {per:>9.3f} | {short - TOKENS * per:>15.1f}")
    return lines + [""]


def kernel_times(dev, quick: bool, top_p: bool = False) -> list[str]:
    lines = ["== pz::sample_rows alone: us per launch, device events around trains of back-to-back launches on fixed",
             "   logits, median over the trains [interquartile range]; T = 0.8 ==",
             f"{'V':>6} {'rows':>5} | {'top_k off':>18} | {'top_k = 50':>18} | {'greedy (T = 0)':>18}"]
    modes = ((0.8, None, {}), (0.8, 50, {}), (0.0, None, {}))
    if top_p:
        lines[-1] = (f"{'V':>6} {'rows':>5} | {'options off':>18} | {'top_k = 50':>18} | {'top_p = 0.9':>18} | "
                     f"{'top_p 0.9, top_k 50':>19} | {'min_p = 0.05':>18}")
        modes = ((0.8, None, {}), (0.8, 50, {}), (0.8, None, {"top_p": 0.9}), (0.8, 50, {"top_p": 0.9}),
                 (0.8, None, {"min_p": 0.05}))
    iters, trains = (100, 3) if quick else (1000, 7)
    g = torch.Generator().manual_seed(4)
    for v in (27, 4096, 65536):
        for rows in ROWS:
            logits = (2.0 * torch.randn(rows, v, generator=g)).to(dev)
            seq = torch.zeros(rows, 4, device=dev, dtype=torch.int64)
            done = torch.zeros(rows, device=dev, dtype=torch.int32)
            cells = []
            for temperature, top_k, extra in modes:
                def launch(i):
                    PF.sample_rows(logits, seq, done, i & 3, seed=(5, 6), step=i, temperature=temperature, top_k=top_k,
                                   **extra)
                for i in range(10):
                    launch(i)
                torch.cuda.synchronize()
                times = []
                for _ in range(trains):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(iters):
                        launch(i)
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e3 / iters)
                cells.append(f"{statistics.median(times):>9.2f} [{_iqr(times):>6.2f}]")
            lines.append(f"{v:>6} {rows:>5} | " + " | ".join(cells))
    lines.append("(a launch shorter than the host's launch interval shows that interval, about 5 us, not the kernel)")
    return lines


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="profiles/generate_latency.txt (generate_resident_latency.txt "
                                                "with --resident)")
    ap.add_argument("--quick", action="store_true", help="fewer repeats (a rehearsal, not a measurement)")
    ap.add_argument("--resident", action="store_true", help="only section 3: the one-launch form against the device loop")
    ap.add_argument("--top-p", action="store_true", help="only section 4: nucleus sampling")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sample_top_p_latency.txt" if args.top_p else
                                "generate_resident_latency.txt" if args.resident else "generate_latency.txt")
    if not torch.cuda.is_available():
        print("generate_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 2
    native.require()
    dev = torch.device("cuda:0")
    lines = [f"generate_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
             f"{' (quick: fewer repeats)' if args.quick else ''}", ""]
    if args.top_p:
        lines += kernel_times(dev, args.quick, top_p=True) + [""]
        for name in MODELS:
            lines += top_p_throughput(name, args.quick)
    elif args.resident:
        for dtype in ("bfloat16", "float32"):
            lines += resident_throughput(dtype, args.quick)
    else:
        for name in MODELS:
            lines += model_throughput(name, args.quick)
        lines += kernel_times(dev, args.quick)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
