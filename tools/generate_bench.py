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

Usage: python tools/generate_bench.py [--out profiles/generate_latency.txt] [--quick] [--resident]
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


def kernel_times(dev, quick: bool) -> list[str]:
    lines = ["== pz::sample_rows alone: us per launch, device events around trains of back-to-back launches on fixed",
             "   logits, median over the trains [interquartile range]; T = 0.8 ==",
             f"{'V':>6} {'rows':>5} | {'top_k off':>18} | {'top_k = 50':>18} | {'greedy (T = 0)':>18}"]
    iters, trains = (100, 3) if quick else (1000, 7)
    g = torch.Generator().manual_seed(4)
    for v in (27, 4096, 65536):
        for rows in ROWS:
            logits = (2.0 * torch.randn(rows, v, generator=g)).to(dev)
            seq = torch.zeros(rows, 4, device=dev, dtype=torch.int64)
            done = torch.zeros(rows, device=dev, dtype=torch.int32)
            cells = []
            for temperature, top_k in ((0.8, None), (0.8, 50), (0.0, None)):
                def launch(i):
                    PF.sample_rows(logits, seq, done, i & 3, seed=(5, 6), step=i, temperature=temperature, top_k=top_k)
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
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "generate_resident_latency.txt" if args.resident else "generate_latency.txt")
    if not torch.cuda.is_available():
        print("generate_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 2
    native.require()
    dev = torch.device("cuda:0")
    lines = [f"generate_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
             f"{' (quick: fewer repeats)' if args.quick else ''}", ""]
    if args.resident:
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
