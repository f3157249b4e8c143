#!/usr/bin/env python
"""Sequence scoring throughput on the GPU (needs an MI355X; fails without a GPU).

Models (bfloat16, batchnorm statistics from one training-mode forward):
  chars: [27, 10, 30, 64, 27]           embedding, linear, batchnorm, tanh, linear, softmax (context 3)
  wide:  [4096, 64, 512, 4096, 4096]    the same layers, vocabulary 4096 (context 8)

1. Scored ids per second at 64, 1,024 and 16,384 scored positions (rows of 64 ids):
   * device: ``model.score(seqs, details=False)`` (engine/predictor.py: one upload, the forward kernels on
     chunks of windows, one ``pz::token_logprob`` launch per chunk, two numbers downloaded);
   * host loop: what a caller had before ``score`` existed — ``model.predict`` on the windows (1,024 per
     call, so that the returned Python lists stay bounded), then ``log`` and gather on the host and the
     mean.
   Both are the public API (Python lists in), timed by a host clock around a call that ends with its
   result on the host, in the same process, alternating, after a warm-up of both; median and
   interquartile range over the repeats.
2. ``pz::token_logprob`` alone against ``torch.log_softmax(logits, -1).gather(...)`` on the same fp32
   logits: device-event time per launch over trains of back-to-back launches, V = 27, 4096 and 65536.

Usage: python tools/score_bench.py [--out profiles/score_latency.txt] [--quick]
"""
from __future__ import annotations

import argparse
import math
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
POSITIONS = [64, 1024, 16384]
ROW_IDS = 64       # ids per sequence
HOST_CHUNK = 1024  # windows per predict() call of the host loop
KERNEL_SHAPES = {27: [1024, 16384, 1 << 20], 4096: [64, 1024, 16384], 65536: [1, 16, 256]}


def _iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def _build(name: str, dtype: str = "bfloat16") -> NeuralNetworkModel:
    torch.manual_seed(0)
    sizes = MODELS[name]
    model = NeuralNetworkModel(f"score_bench_{name}", sizes, activation_algos=ALGOS, bias_algo="random",
                               dtype=dtype, device="cuda:0")
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, sizes[0], (256, model.context_length), generator=g)
    model.compute_output(ids.tolist(), [[int(i)] for i in torch.randint(0, sizes[-1], (256,), generator=g)])
    return model


def host_loop(model, seqs: list, pad_token: int = 0) -> dict:
    """The scorer over the public ``predict``: every window, then log and gather on the host."""
    length = model.context_length
    windows, targets = [], []
    for row in seqs:
        padded = [pad_token] * length + row
        for j, t in enumerate(row):
            windows.append(padded[j:j + length])
            targets.append(t)
    total = 0.0
    for i0 in range(0, len(windows), HOST_CHUNK):
        probs = torch.tensor(model.predict(windows[i0:i0 + HOST_CHUNK]), dtype=torch.float64)
        picked = probs.gather(1, torch.tensor(targets[i0:i0 + HOST_CHUNK]).unsqueeze(1))
        total += float(picked.log().sum())
    nll = -total / len(targets)
    return {"tokens": len(targets), "nll": nll, "perplexity": math.exp(nll)}


def model_throughput(name: str, quick: bool) -> list[str]:
    model = _build(name)
    assert model._fused_predictor() is not None, "the bench models must go through the fused predictor"
    vocab = MODELS[name][0]
    lines = [f"== {name} {MODELS[name]} bfloat16, context {model.context_length}, rows of {ROW_IDS} ids: scored ids/s, "
             "median [interquartile range] ==",
             f"{'ids':>6} | {'device (score, details=False)':>30} {'ms/call':>10} | {'host loop (predict + log + gather)':>36} "
             f"{'ms/call':>10} | {'device / host':>13} | nll device / host"]
    g = torch.Generator().manual_seed(2)
    for positions in POSITIONS:
        seqs = torch.randint(0, vocab, (positions // ROW_IDS, ROW_IDS), generator=g).tolist()
        reps = 3 if quick or positions > 1024 else 9
        for _ in range(1 if positions > 1024 else 2):  # warm-up of every shape the timed window uses
            dev = model.score(seqs, details=False)
            host = host_loop(model, seqs)
        td, th = [], []
        for _ in range(reps):  # alternating; each call ends with its result on the host
            t0 = time.perf_counter()
            model.score(seqs, details=False)
            t1 = time.perf_counter()
            host_loop(model, seqs)
            t2 = time.perf_counter()
            td.append(t1 - t0)
            th.append(t2 - t1)
        rd, rh = [positions / t for t in td], [positions / t for t in th]
        lines.append(f"{positions:>6} | {statistics.median(rd):>19,.0f} [{_iqr(rd):>8,.0f}] {statistics.median(td) * 1e3:>10.3f} | "
                     f"{statistics.median(rh):>25,.0f} [{_iqr(rh):>8,.0f}] {statistics.median(th) * 1e3:>10.3f} | "
                     f"{statistics.median(rd) / statistics.median(rh):>12.2f}x | {dev['nll']:.6f} / {host['nll']:.6f}")
    return lines + [""]


def kernel_times(dev, quick: bool) -> list[str]:
    lines = ["== pz::token_logprob alone against torch.log_softmax(logits, -1).gather(1, targets): us per call, device",
             "   events around trains of back-to-back calls on fixed fp32 logits, median over the trains",
             "   [interquartile range]; MiB = the logits ==",
             f"{'V':>6} {'rows':>8} {'MiB':>7} | {'token_logprob + rank':>20} | {'token_logprob':>18} | {'torch composition':>18} | "
             f"{'torch / kernel':>14}"]
    g = torch.Generator().manual_seed(4)
    for v, shapes in KERNEL_SHAPES.items():
        for rows in shapes:
            logits = (2.0 * torch.randn(rows, v, generator=g)).to(dev)
            targets = torch.randint(0, v, (rows,), generator=g).to(dev)
            logprob = torch.empty(rows, device=dev, dtype=torch.float32)
            rank = torch.empty(rows, device=dev, dtype=torch.int32)
            calls = (lambda: PF.token_logprob(logits, targets, logprob, rank),
                     lambda: PF.token_logprob(logits, targets, logprob, None),
                     lambda: torch.log_softmax(logits, -1).gather(1, targets.unsqueeze(1)))
            big = rows * v * 4 > 32 << 20
            iters, trains = (10, 3) if quick else ((50, 7) if big else (500, 7))
            med, cells = [], []
            for call in calls:
                for _ in range(5):
                    call()
                torch.cuda.synchronize()
                times = []
                for _ in range(trains):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        call()
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e3 / iters)
                med.append(statistics.median(times))
                cells.append(f"{statistics.median(times):>9.2f} [{_iqr(times):>6.2f}]")
            lines.append(f"{v:>6} {rows:>8} {rows * v * 4 / 2 ** 20:>7.1f} | {cells[0]:>20} | {cells[1]:>18} | {cells[2]:>18} | "
                         f"{med[2] / med[0]:>13.2f}x")
            del logits
    lines.append("(a call shorter than the host's launch interval shows that interval, about 5 us, not the kernel; the torch")
    lines.append(" composition is two launches and one [rows, V] temporary)")
    return lines


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_latency.txt"))
    ap.add_argument("--quick", action="store_true", help="fewer repeats (a rehearsal, not a measurement)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("score_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 2
    native.require()
    dev = torch.device("cuda:0")
    lines = [f"score_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
             f"{' (quick: fewer repeats)' if args.quick else ''}", ""]
    print("\n".join(lines), flush=True)
    for section in [lambda name=name: model_throughput(name, args.quick) for name in MODELS] + [lambda: kernel_times(dev, args.quick)]:
        part = section()
        print("\n".join(part), flush=True)  # as it comes: the whole run takes minutes
        lines += part
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
