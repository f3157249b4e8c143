#!/usr/bin/env python
"""Top-k selection and classify() latency on the GPU (needs an MI355X; fails without a GPU).

1. ``pz::topk_rows`` alone against ``torch.log_softmax(logits, -1)`` followed by ``torch.topk(k)`` on the same
   fp32 logits: device-event time per call over trains of back-to-back calls, V = 27, 4096 and 65536 at the row
   counts of ``profiles/score_latency.txt``, k = 1, 5 and 64 (27 at V = 27). The two do not compute quite the
   same thing: ``torch.topk`` leaves the order of equal logits open, the kernel takes them by column.
2. ``model.classify(rows, top_k=5)`` against what a caller had before it existed: ``model.predict(rows)``, then a
   Python sort of every returned row. Both are the public API (Python lists in, Python lists out), timed by a
   host clock, alternating, after a warm-up of both; median and interquartile range over the repeats. Models
   (bfloat16, batchnorm statistics from one training-mode forward), 1, 16, 64 and 1024 rows:
     chars: [27, 10, 30, 64, 27]           embedding, linear, batchnorm, tanh, linear, softmax (context 3)
     wide:  [4096, 64, 512, 4096, 4096]    the same layers, vocabulary 4096 (context 8)

Every section measures in one process of its own, started under ``timeout -k 10``; after a section that fails
nothing more is started, and what was measured until then is written with a note.

Usage: python tools/topk_bench.py [--out profiles/topk_latency.txt] [--quick]
"""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ALGOS = ["embedding", "linear", "batchnorm", "tanh", "linear", "softmax"]
MODELS = {"chars": [27, 10, 30, 64, 27], "wide": [4096, 64, 512, 4096, 4096]}
KERNEL_SHAPES = {27: [1024, 16384, 1 << 20], 4096: [64, 1024, 16384], 65536: [1, 16, 256]}
KS = [1, 5, 64]
CLASSIFY_ROWS = [1, 16, 64, 1024]
TOP_K = 5
SECTIONS = [f"kernel:{v}" for v in KERNEL_SHAPES] + [f"classify:{name}" for name in MODELS]
SECTION_SECONDS = 300


def _iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def kernel_times(v: int, quick: bool) -> list[str]:
    import torch
    from penr_oz_neural_network_torch_amd.ops import functional as PF
    dev = torch.device("cuda:0")
    lines = []
    if v == next(iter(KERNEL_SHAPES)):
        lines += [f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}", "",
                  "== pz::topk_rows alone against torch.log_softmax(logits, -1) then torch.topk(k): us per call, device events",
                  "   around trains of back-to-back calls on fixed fp32 logits, median over the trains [interquartile range];",
                  "   MiB = the logits ==",
                  f"{'V':>6} {'rows':>8} {'MiB':>7} {'k':>3} | {'topk_rows':>18} | {'torch composition':>18} | {'torch / kernel':>14}"]
    g = torch.Generator().manual_seed(4)
    for rows in KERNEL_SHAPES[v]:
        logits = (2.0 * torch.randn(rows, v, generator=g)).to(dev)
        for k in sorted({min(k, v) for k in KS}):
            idx = torch.empty(rows, k, device=dev, dtype=torch.int32)
            logprob = torch.empty(rows, k, device=dev, dtype=torch.float32)
            calls = (lambda: PF.topk_rows(logits, k, idx, logprob),
                     lambda: torch.topk(torch.log_softmax(logits, -1), k, dim=-1))
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
            lines.append(f"{v:>6} {rows:>8} {rows * v * 4 / 2 ** 20:>7.1f} {k:>3} | {cells[0]:>18} | {cells[1]:>18} | "
                         f"{med[1] / med[0]:>13.2f}x")
        del logits
    if v == list(KERNEL_SHAPES)[-1]:
        lines += ["(a call shorter than the host's launch interval shows that interval, about 5 us, not the kernel; the torch",
                  " composition is a log-softmax launch with one [rows, V] temporary, then torch.topk's launches)", ""]
    return lines


def host_sort(model, rows: list, k: int) -> dict:
    """What a caller did before classify(): the whole softmax rows, then a stable descending sort of each."""
    probs = model.predict(rows)
    classes = [sorted(range(len(p)), key=p.__getitem__, reverse=True)[:k] for p in probs]
    return {"classes": classes, "probabilities": [[p[c] for c in cs] for p, cs in zip(probs, classes)]}


def classify_times(name: str, quick: bool) -> list[str]:
    import torch
    from penr_oz_neural_network_torch_amd.models import NeuralNetworkModel
    torch.manual_seed(0)
    sizes = MODELS[name]
    model = NeuralNetworkModel(f"topk_bench_{name}", sizes, activation_algos=ALGOS, bias_algo="random", dtype="bfloat16",
                               device="cuda:0")
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, sizes[0], (256, model.context_length), generator=g)
    model.compute_output(ids.tolist(), [[int(i)] for i in torch.randint(0, sizes[-1], (256,), generator=g)])
    assert model._fused_predictor() is not None, "the bench models must go through the fused predictor"
    lines = [f"== {name} {sizes} bfloat16, context {model.context_length}: ms per call, host clock, lists in and lists out, "
             "median [interquartile range] ==",
             f"{'rows':>6} | {'classify(rows, top_k=5)':>26} | {'predict(rows) + Python sort':>30} | {'host / classify':>15} | same classes"]
    lost = []
    for rows in CLASSIFY_ROWS:
        x = torch.randint(0, sizes[0], (rows, model.context_length), generator=g).tolist()
        reps = 5 if quick else (15 if rows >= 1024 else 41)
        for _ in range(2):  # warm-up of both
            dev = model.classify(x, top_k=TOP_K)
            host = host_sort(model, x, TOP_K)
        same = sum(a == b for a, b in zip(dev["classes"], host["classes"]))
        td, th = [], []
        for _ in range(reps):  # alternating; each call ends with its result on the host
            t0 = time.perf_counter()
            model.classify(x, top_k=TOP_K)
            t1 = time.perf_counter()
            host_sort(model, x, TOP_K)
            t2 = time.perf_counter()
            td.append((t1 - t0) * 1e3)
            th.append((t2 - t1) * 1e3)
        lines.append(f"{rows:>6} | {statistics.median(td):>15.3f} [{_iqr(td):>8.3f}] | {statistics.median(th):>19.3f} [{_iqr(th):>8.3f}] | "
                     f"{statistics.median(th) / statistics.median(td):>14.2f}x | {same} of {rows}")
        if statistics.median(td) > statistics.median(th):
            lost.append(str(rows))
    if lost:
        lines.append(f"(classify was SLOWER than predict + sort at {', '.join(lost)} rows: {sizes[-1]} probabilities per row are cheap to")
        lines.append(" download and sort, and the selection launch plus the exp on the device cost more than they save)")
    return lines + [""]


def run_section(section: str, quick: bool) -> int:
    import torch
    if not torch.cuda.is_available():
        print("topk_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 2
    from penr_oz_neural_network_torch_amd.ops import native
    native.require()
    kind, what = section.split(":")
    lines = kernel_times(int(what), quick) if kind == "kernel" else classify_times(what, quick)
    print("\n".join(lines), flush=True)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_latency.txt"))
    ap.add_argument("--quick", action="store_true", help="fewer repeats (a rehearsal, not a measurement)")
    ap.add_argument("--section", choices=SECTIONS, help="measure this section in this process and print it")
    args = ap.parse_args(argv)
    if args.section:
        return run_section(args.section, args.quick)
    text = f"topk_bench{' (quick: fewer repeats)' if args.quick else ''}\n\n"
    status = 0
    for section in SECTIONS:  # one process each, under a time limit; nothing starts after a failure
        cmd = ["timeout", "-k", "10", str(SECTION_SECONDS), sys.executable, os.path.abspath(__file__), "--section", section]
        res = subprocess.run(cmd + (["--quick"] if args.quick else []), stdout=subprocess.PIPE, text=True, cwd=ROOT)
        print(res.stdout, end="", flush=True)
        text += res.stdout
        if res.returncode != 0:
            note = f"(section {section} ended with status {res.returncode}: nothing after it was started)\n"
            print(note, end="", file=sys.stderr)
            text += note
            status = res.returncode
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)
    return status


if __name__ == "__main__":
    sys.exit(main())
