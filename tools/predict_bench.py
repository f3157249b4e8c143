#!/usr/bin/env python
"""Inference latency of the GPU serving path (needs an MI355X; fails without a GPU).

Model: [1024, 4096, 4096, 1024] relu, relu, softmax, bf16 (the bench.py flagship family).

1. ``model.predict`` (engine/predictor.py) against ``model.compute_output`` without a target (the
   autograd layer loop, the only GPU inference path before ``predict`` existed) at 1, 8, 16, 64 and
   8192 rows: median wall time per call, both measured in the same process, alternating, each call
   ending in the device-to-host copy of its result. Two levels: the public API (Python lists in
   and out, so list <-> tensor conversion is inside) and the device path (a device tensor in, a
   device tensor out, then one synchronise).
2. Per layer shape: ``PF.gemm_skinny`` against ``PF.gemm`` (which takes its generic kernel below 64
   rows) on the same operands at M = 1 and M = 16: device-event time per launch over a long
   back-to-back train of launches, and W's bytes over that time. "hot": the same W every launch (it
   fits the 256 MiB Infinity Cache, so this is a cache rate, not HBM); "rotating": launches cycle
   through enough copies of W (> 256 MiB in all) that each read misses the caches.

3. ``--w8`` (a run of its own, written to profiles/predict_w8_latency.txt): weight-only e4m3
   inference. Per layer shape, ``PF.gemm_skinny_w8`` against ``PF.gemm_skinny`` on the dequantised
   bf16 copies of the same weights, hot and rotating, M = 1 and 16, the two kernels' trains
   alternating, with interquartile ranges; end to end, the flagship model's device path with
   ``weights="fp8"`` against the default at 1, 8 and 16 rows; and the max abs difference of the two
   predictions on 64 rows.

Usage: python tools/predict_bench.py [--out profiles/predict_latency.txt] [--quick] [--w8]
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

SIZES = [1024, 4096, 4096, 1024]
ALGOS = ["relu", "relu", "softmax"]
ROWS = [1, 8, 16, 64, 8192]
HBM_COPY_TBS = 6.29  # MI355X copy rate (MI355X_MICROARCH)
LLC_BYTES = 256 << 20


def _median_pair(fn_new, fn_old, warmup: int, reps: int) -> tuple[float, float, float, float]:
    """Alternating timings of two callables that end synchronised; (median, spread) of each in ms."""
    for _ in range(warmup):
        fn_new()
        fn_old()
    tn, to = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn_new()
        t1 = time.perf_counter()
        fn_old()
        t2 = time.perf_counter()
        tn.append((t1 - t0) * 1e3)
        to.append((t2 - t1) * 1e3)

    def iqr(v):
        q = statistics.quantiles(v, n=4)
        return q[2] - q[0]
    return statistics.median(tn), iqr(tn), statistics.median(to), iqr(to)


def model_latency(model, quick: bool) -> list[str]:
    dev = model.device
    lines = ["== predict vs compute_output (no target): median ms per call [interquartile range] ==",
             f"{'rows':>6} | {'API predict':>22} {'API compute_output':>22} {'ratio':>6} | "
             f"{'device predict':>22} {'device layer loop':>22} {'ratio':>6}"]
    g = torch.Generator().manual_seed(1)
    pred = model._fused_predictor()
    assert pred is not None, "the flagship model must go through the fused predictor"
    for rows in ROWS:
        x = torch.randn(rows, SIZES[0], generator=g)
        data = x[0].tolist() if rows == 1 else x.tolist()
        xd = (x[0] if rows == 1 else x).to(dev)
        big = rows >= 1024
        reps = (3 if big else 30) if quick else (7 if big else 300)
        a = _median_pair(lambda: model.predict(data), lambda: model.compute_output(data), 2 if big else 5, reps)

        def dev_new():
            pred.forward(xd)
            torch.cuda.synchronize(dev)

        def dev_old():
            with torch.no_grad():
                model._forward(xd, None)
            torch.cuda.synchronize(dev)
        reps = (10 if big else 30) if quick else (50 if big else 300)
        d = _median_pair(dev_new, dev_old, 5, reps)
        lines.append(f"{rows:>6} | {a[0]:>13.4f} [{a[1]:>6.4f}] {a[2]:>13.4f} [{a[3]:>6.4f}] {a[2] / a[0]:>5.2f}x | "
                     f"{d[0]:>13.4f} [{d[1]:>6.4f}] {d[2]:>13.4f} [{d[3]:>6.4f}] {d[2] / d[0]:>5.2f}x")
    # same answers: predict against compute_output on 64 rows
    x = torch.randn(64, SIZES[0], generator=g).tolist()
    diff = (torch.tensor(model.predict(x)) - torch.tensor(model.compute_output(x)[0])).abs().max().item()
    lines.append(f"max |predict - compute_output| on 64 rows: {diff:.3e} (softmax outputs, bf16 pipelines)")
    return lines


def _event_time(launch, n_ops: int, iters: int, trains: int) -> float:
    """Median over `trains` of the device-event time per launch of `iters` back-to-back launches (us);
    launch(i) issues launch number i (n_ops operand sets are cycled by the caller)."""
    for i in range(max(n_ops, 10)):
        launch(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(trains):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            launch(i)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out)


def layer_kernels(dev, quick: bool) -> list[str]:
    lines = ["", "== per layer: gemm_skinny vs PF.gemm (generic kernel below 64 rows), bf16, bias + relu fused ==",
             "   us per launch = device events around a back-to-back train of launches (host launch cost is inside",
             "   when a kernel is shorter than the host's launch interval); TB/s = bytes of W / that time.",
             f"   MI355X copy rate for comparison: {HBM_COPY_TBS} TB/s (HBM). 'hot' W (<= 32 MiB) stays in the 256 MiB",
             "   Infinity Cache between launches: a rate above the HBM figure there is a cache rate, not HBM bandwidth.",
             f"{'K':>5} {'N':>5} {'M':>3} | {'skinny hot us':>13} {'TB/s':>6} | {'skinny rotating us':>18} {'TB/s':>6} | "
             f"{'PF.gemm hot us':>14} {'TB/s':>6} | {'speed-up (hot)':>14}"]
    iters, trains = (200, 3) if quick else (2000, 5)
    g = torch.Generator().manual_seed(2)
    epi = PF.epi_spec(act=PF.ACT_RELU)
    for k, n in zip(SIZES[:-1], SIZES[1:]):
        wbytes = k * n * 2
        copies = LLC_BYTES // wbytes + 2  # > 256 MiB of distinct weights in rotation
        ws = [(0.03 * torch.randn(k, n, generator=g)).to(torch.bfloat16).to(dev) for _ in range(copies)]
        bias = torch.randn(n, generator=g).to(dev)
        for m in (1, 16):
            x = torch.randn(m, k, generator=g).to(torch.bfloat16).to(dev)
            out = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
            assert PF.gemm_skinny_eligible(x, ws[0], out)
            hot = _event_time(lambda i: PF.gemm_skinny(x, ws[0], out, bias=bias, act=PF.ACT_RELU), 1, iters, trains)
            rot = _event_time(lambda i: PF.gemm_skinny(x, ws[i % copies], out, bias=bias, act=PF.ACT_RELU), copies,
                              iters, trains)
            old = _event_time(lambda i: PF.gemm(x, True, ws[0], False, out, bias=bias, mode=PF.EPI_FWD, epi=epi), 1,
                              max(50, iters // 10), trains)
            lines.append(f"{k:>5} {n:>5} {m:>3} | {hot:>13.2f} {wbytes / hot / 1e6:>6.2f} | {rot:>18.2f} "
                         f"{wbytes / rot / 1e6:>6.2f} | {old:>14.2f} {wbytes / old / 1e6:>6.2f} | {old / hot:>13.1f}x")
        del ws
    return lines


W8_SHAPES = [(1024, 4096), (4096, 4096), (4096, 1024), (8192, 8192)]


def _iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def _event_trains_pair(launch_a, launch_b, n_ops: int, iters: int, trains: int):
    """Trains of `iters` back-to-back launches of a and of b, alternating; (median, IQR) of the
    device-event time per launch (us) of each."""
    for i in range(max(n_ops, 10)):
        launch_a(i)
        launch_b(i)
    torch.cuda.synchronize()
    res = ([], [])
    for _ in range(trains):
        for launch, out in ((launch_a, res[0]), (launch_b, res[1])):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                launch(i)
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(res[0]), _iqr(res[0]), statistics.median(res[1]), _iqr(res[1])


def w8_layer_kernels(dev, quick: bool) -> list[str]:
    lines = ["== per layer: gemm_skinny_w8 (e4m3 W, 1 B/weight) vs gemm_skinny on the dequantised bf16 copies of the SAME",
             "   weights (2 B/weight), bias + relu fused, bf16 output; trains of back-to-back launches, the two kernels'",
             "   trains alternating; us per launch = median over the trains [interquartile range]. 'hot': one W every",
             "   launch (Infinity Cache / L2 resident); 'rotating': launches cycle through > 256 MiB of distinct W8 (and",
             "   twice that of bf16), so every read misses the caches. ratio = w8 / bf16 time (bytes halve: 0.5 is the floor).",
             f"{'K':>5} {'N':>5} {'M':>3} | {'w8 hot us':>16} {'bf16 hot us':>16} {'ratio':>6} | "
             f"{'w8 rotating us':>16} {'bf16 rotating us':>16} {'ratio':>6} {'w8 TB/s':>8} {'bf16 TB/s':>9}"]
    iters, trains = (100, 4) if quick else (1000, 9)
    g = torch.Generator(device=dev).manual_seed(2)
    for k, n in W8_SHAPES:
        copies = LLC_BYTES // (k * n) + 2  # > 256 MiB of distinct e4m3 weights in rotation
        w8s, scales, wbs = [], [], []
        for _ in range(copies):
            w8, scale = PF.quantize_cols(0.03 * torch.randn(k, n, generator=g, device=dev))
            w8s.append(w8)
            scales.append(scale)
            wbs.append(PF.dequantize_cols(w8, scale))
        bias = torch.randn(n, generator=g, device=dev)
        for m in (1, 16):
            x = torch.randn(m, k, generator=g, device=dev).to(torch.bfloat16)
            out8 = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
            out16 = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
            assert PF.gemm_skinny_w8_eligible(x, w8s[0], scales[0], out8) and PF.gemm_skinny_eligible(x, wbs[0], out16)

            def run8(i):
                PF.gemm_skinny_w8(x, w8s[i], scales[i], out8, bias=bias, act=PF.ACT_RELU)

            def run16(i):
                PF.gemm_skinny(x, wbs[i], out16, bias=bias, act=PF.ACT_RELU)
            hot = _event_trains_pair(lambda i: run8(0), lambda i: run16(0), 1, iters, trains)
            rot = _event_trains_pair(lambda i: run8(i % copies), lambda i: run16(i % copies), copies, iters, trains)
            lines.append(f"{k:>5} {n:>5} {m:>3} | {hot[0]:>8.2f} [{hot[1]:>5.2f}] {hot[2]:>8.2f} [{hot[3]:>5.2f}] "
                         f"{hot[0] / hot[2]:>6.2f} | {rot[0]:>8.2f} [{rot[1]:>5.2f}] {rot[2]:>8.2f} [{rot[3]:>5.2f}] "
                         f"{rot[0] / rot[2]:>6.2f} {k * n / rot[0] / 1e6:>8.2f} {2 * k * n / rot[2] / 1e6:>9.2f}")
        del w8s, scales, wbs
        torch.cuda.empty_cache()
    return lines


def w8_model_latency(model, quick: bool) -> list[str]:
    dev = model.device
    pred = model._fused_predictor()
    assert pred is not None, "the flagship model must go through the fused predictor"
    lines = ["", "== end to end, device path (device tensor in and out, one synchronise): predict from e4m3 weights vs the",
             "   default bf16 copies, median ms per call [interquartile range], alternating. A call is dominated by",
             "   launch and host cost, not by its ~20 us of kernels: the kernels' gain shows only in part ==",
             f"{'rows':>6} | {'weights=fp8':>22} {'default':>22} {'fp8 / default':>14}"]
    g = torch.Generator().manual_seed(1)
    for rows in (1, 8, 16):
        x = torch.randn(rows, SIZES[0], generator=g)
        xd = (x[0] if rows == 1 else x).to(dev)

        def dev_fp8():
            pred.forward(xd, weights="fp8")
            torch.cuda.synchronize(dev)

        def dev_default():
            pred.forward(xd)
            torch.cuda.synchronize(dev)
        d = _median_pair(dev_fp8, dev_default, 5, 30 if quick else 300)
        lines.append(f"{rows:>6} | {d[0]:>13.4f} [{d[1]:>6.4f}] {d[2]:>13.4f} [{d[3]:>6.4f}] {d[0] / d[2]:>13.2f}x")
    x = torch.randn(64, SIZES[0], generator=g).tolist()
    diff = (torch.tensor(model.predict(x, weights="fp8")) - torch.tensor(model.predict(x))).abs().max().item()
    top = torch.tensor(model.predict(x)).max().item()
    lines.append(f"max |predict(weights='fp8') - predict| on 64 rows: {diff:.3e} (softmax outputs, largest output {top:.3e}; "
                 "untrained random weights)")
    return lines


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_latency.txt"))
    ap.add_argument("--quick", action="store_true", help="fewer repeats (a rehearsal, not a measurement)")
    ap.add_argument("--kernels-only", action="store_true", help="only the per-layer kernel comparison")
    ap.add_argument("--w8", action="store_true",
                    help="the weight-only e4m3 section instead (default --out: profiles/predict_w8_latency.txt)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("predict_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 2
    native.require()
    dev = torch.device("cuda:0")
    lines = [f"predict_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
             f"{' (quick: fewer repeats)' if args.quick else ''}",
             f"model {SIZES} {ALGOS} bfloat16", ""]
    if args.w8:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "predict_w8_latency.txt")
        lines += w8_layer_kernels(dev, args.quick)
        if not args.kernels_only:
            torch.manual_seed(0)
            model = NeuralNetworkModel("predict_bench", SIZES, activation_algos=ALGOS, dtype="bfloat16", device="cuda:0")
            lines += w8_model_latency(model, args.quick)
            del model
    elif not args.kernels_only:
        torch.manual_seed(0)
        model = NeuralNetworkModel("predict_bench", SIZES, activation_algos=ALGOS, dtype="bfloat16", device="cuda:0")
        lines += model_latency(model, args.quick)
        del model
    if not args.w8:
        lines += layer_kernels(dev, args.quick)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
