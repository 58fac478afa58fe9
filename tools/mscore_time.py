#!/usr/bin/env python3
"""Times ciao_margin_stats_multi (csrc/mscore_kernels.h: K models' per-sample statistics in one pass over A) on cuda:0.  Device events
after warm runs, the median of CIAO_REPEATS (default 9) repeats; calls of 50 ms and more: 5 repeats.

Per shape (N = 10^7: d = 1024 fp64 and fp32, d = 50 and d = 255 fp64), loss and K in {16, 256}, from the same run on the same box:

  new   Context.margin_stats_multi, the whole call (pointer table upload, both kernels, the copy back)
  (a)   K x the two-call path of scoring.score -- Context.row_dots + Context.margin_stats, timed once and multiplied by K
        condition: new < (a) at every shape
  (b)   one ciao_full_gradient pass over the same PackedF (ratio recorded only)
  (c)   d = 1024: ciao_full_gradient_multi at the same K, plus K x ciao_margin_stats alone on given dots (timed once, multiplied)
        condition: new <= (c)
  and the fraction of the MFMA peak of 2 N d K flops (fp64 78.6, fp32 157.3 TFLOP/s; recorded only)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ciao_loader
ciao_loader.load()
from ciaoalgorithms_jl_amd.device import Context, PackedF

torch.cuda.set_device(0)
ctx = Context(0)
dev = torch.device("cuda", 0)
N = int(float(os.environ.get("CIAO_N", "1e7")))
REPEATS = int(os.environ.get("CIAO_REPEATS", "9"))
SHAPES = [(1024, torch.float64), (1024, torch.float32), (50, torch.float64), (255, torch.float64)]
if os.environ.get("CIAO_SHAPES"):                       # e.g. "1024:f64,50:f64"
    SHAPES = [(int(v.split(":")[0]), torch.float64 if v.endswith("f64") else torch.float32) for v in os.environ["CIAO_SHAPES"].split(",")]
KS = [int(v) for v in os.environ.get("CIAO_K", "16,256").split(",")]
PEAK = {torch.float64: 78.6e12, torch.float32: 157.3e12}


def median_ms(fn, warm=2):
    for _ in range(warm):
        fn()
    ctx.synchronize()
    ts = []
    for i in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
        if ts[-1] >= 50.0 and i >= 4:
            break
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


print(f"# N = {N}; median (min .. max) of {REPEATS} repeats (5 for calls of 50 ms and more), device events, ms", flush=True)
for d, dt in SHAPES:
    name = "f64" if dt == torch.float64 else "f32"
    A = torch.empty((N, d), dtype=dt, device=dev)
    ctx.synth_normal(A, 0, seed=7, scale=1.0 / np.sqrt(d))
    gen = torch.Generator(device="cuda").manual_seed(d)
    xs = [0.5 * torch.randn(d, dtype=dt, device=dev, generator=gen) for _ in range(max(KS))]
    avs = [torch.empty_like(x) for x in xs]
    dots = torch.empty(N, dtype=dt, device=dev)
    for loss in ("ls", "logistic"):
        b = torch.empty(N, dtype=dt, device=dev)
        F = PackedF.least_squares(A, b, float(N)) if loss == "ls" else PackedF.logistic(A, b)
        ctx.synth_targets(F, xs[0], noise=0.01, labels=(loss == "logistic"), seed=7, b_out=b)
        t_pass = median_ms(lambda: ctx.full_gradient(F, xs[0], avs[0]))
        k_pass = ctx.last_kernel()
        t_dots = median_ms(lambda: ctx.row_dots(F, xs[0], out=dots))
        t_stat = median_ms(lambda: ctx.margin_stats(F, dots, 1.0))
        t_score = median_ms(lambda: ctx.margin_stats(F, ctx.row_dots(F, xs[0], out=dots), 1.0))
        print(f"{name} d={d} {loss}: (b) ciao_full_gradient {fmt(t_pass)} [{k_pass}]  row_dots {fmt(t_dots)}  margin_stats {fmt(t_stat)}  "
              f"score = row_dots + margin_stats {fmt(t_score)}", flush=True)
        for K in KS:
            t_new = median_ms(lambda: ctx.margin_stats_multi(F, xs[:K]))
            k_new = ctx.last_kernel()
            a = K * t_score[0]
            flops = 2.0 * N * d * K
            line = (f"{name} d={d} {loss} K={K}: new {fmt(t_new)}  (a) K x score {a:.1f}  new / (a) {t_new[0] / a:.4f}  "
                    f"condition new < (a): {'met' if t_new[0] < a else 'MISSED'}  new / (b) {t_new[0] / t_pass[0]:.2f}  "
                    f"MFMA {flops / (t_new[0] * 1e-3) / PEAK[dt]:.3f} of peak")
            if d == 1024:
                t_multi = median_ms(lambda: ctx.full_gradient_multi(F, xs[:K], avs[:K]))
                k_multi = ctx.last_kernel()
                c = t_multi[0] + K * t_stat[0]
                line += (f"\n    (c) ciao_full_gradient_multi {fmt(t_multi)} + K x margin_stats {K * t_stat[0]:.3f} = {c:.3f}  new / (c) "
                         f"{t_new[0] / c:.3f}  condition new <= (c): {'met' if t_new[0] <= c else 'MISSED'}  [{k_multi}]")
            print(line + f"\n    [{k_new}]", flush=True)
        del F, b
    del A, xs, avs, dots
    torch.cuda.empty_cache()
ctx.synchronize()
ctx.close()
