#!/usr/bin/env python3
"""Times ciao_margin_stats_multi_rows (csrc/mscore_kernels.h, the MscoreRows instantiations: K models with offsets over a row LIST in
one pass) on cuda:0.  Device events after warm runs, the median of CIAO_REPEATS (default 9) repeats; calls of
50 ms and more: 5 repeats.  Nothing is gated: the ratios are recorded.

Per shape (N = 10^7: d = 1024 fp64 and fp32, d = 255 fp64; tools/mscore_time.py's), logistic rows, K in {16, 256}, from one run:

  (i)   Context.margin_stats_multi without a list (the kernel of section 8.11) against margin_stats_multi(rows=, offsets=) on the
        identity list, a sorted random 20 % list and a sorted random 80 % list; per list the time, the ratio to the call without a
        list, and the ratio per row touched
  (ii)  the same lists through K x scoring.score(rows=, intercept=) -- what cv.logistic_cv(score_together=True) replaces -- timed
        once and multiplied by K
  (iii) one cv.logistic_cv run (CIAO_CV_N rows, default N; d = 255 fp64, 5 folds, 4 weights, gap 1e-6): wall time with and without
        intercept, with and without score_together"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ciao_loader
ciao_loader.load()
from ciaoalgorithms_jl_amd import cv as CV
from ciaoalgorithms_jl_amd.device import Context, PackedF
from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_mu_max
from ciaoalgorithms_jl_amd.scoring import score

torch.cuda.set_device(0)
ctx = Context(0)
dev = torch.device("cuda", 0)
N = int(float(os.environ.get("CIAO_N", "1e7")))
CV_N = int(float(os.environ.get("CIAO_CV_N", str(N))))
REPEATS = int(os.environ.get("CIAO_REPEATS", "9"))
SHAPES = [(1024, torch.float64), (1024, torch.float32), (255, torch.float64)]
if os.environ.get("CIAO_SHAPES"):                       # e.g. "1024:f64,255:f64"
    SHAPES = [(int(v.split(":")[0]), torch.float64 if v.endswith("f64") else torch.float32) for v in os.environ["CIAO_SHAPES"].split(",")]
KS = [int(v) for v in os.environ.get("CIAO_K", "16,256").split(",")]


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


def lists(n):
    g = torch.Generator(device="cpu").manual_seed(n % 1000003)
    perm = torch.randperm(n, generator=g, dtype=torch.int64)
    return [("identity", torch.arange(n, dtype=torch.int64, device=dev)),
            ("sorted 20 %", torch.sort(perm[:n // 5]).values.contiguous().to(dev)),
            ("sorted 80 %", torch.sort(perm[:4 * n // 5]).values.contiguous().to(dev))]


def problem(n, d, dt, seed=7):
    A = torch.empty((n, d), dtype=dt, device=dev)
    ctx.synth_normal(A, 0, seed=seed, scale=1.0 / np.sqrt(d))
    gen = torch.Generator(device="cuda").manual_seed(d)
    x0 = 0.5 * torch.randn(d, dtype=dt, device=dev, generator=gen)
    b = torch.empty(n, dtype=dt, device=dev)
    F = PackedF.logistic(A, b)
    ctx.synth_targets(F, x0, noise=0.01, labels=True, seed=seed, b_out=b)
    return F, gen


print(f"# N = {N}; median (min .. max) of {REPEATS} repeats (5 for calls of 50 ms and more), device events, ms; logistic rows", flush=True)
for d, dt in SHAPES:
    name = "f64" if dt == torch.float64 else "f32"
    F, gen = problem(N, d, dt)
    xs = [0.5 * torch.randn(d, dtype=dt, device=dev, generator=gen) for _ in range(max(KS))]
    offs = [0.01 * (k % 7 - 3) for k in range(max(KS))]
    rows = lists(N)
    for K in KS:
        t_all = median_ms(lambda: ctx.margin_stats_multi(F, xs[:K]))
        print(f"{name} d={d} K={K}: (i) without a list {fmt(t_all)}  [{ctx.last_kernel()}]", flush=True)
        for what, r in rows:
            t = median_ms(lambda: ctx.margin_stats_multi(F, xs[:K], rows=r, offsets=offs[:K], check_rows=False))
            k_new = ctx.last_kernel()
            t_one = median_ms(lambda: score(ctx, F, xs[0], rows=r, intercept=offs[1]))
            frac = r.numel() / N
            print(f"    {what}: (i) {fmt(t)}  / no list {t[0] / t_all[0]:.3f}  per row touched {t[0] / t_all[0] / frac:.3f}   "
                  f"(ii) K x score(rows=) {K * t_one[0]:.1f} (one: {fmt(t_one)})  one pass / (ii) {t[0] / (K * t_one[0]):.4f}\n        [{k_new}]", flush=True)
    del F, xs, rows
    torch.cuda.empty_cache()

# (iii) one cross-validation
F, _ = problem(CV_N, 255, torch.float64, seed=11)
top = logistic_mu_max(DeviceRows(ctx, F), intercept=True)
mus = [0.5 * top, 0.25 * top, 0.1 * top, 0.03 * top]
print(f"# (iii) logistic_cv: N = {CV_N}, d = 255 fp64, 5 folds, 4 weights, gap 1e-6, subproblem cd; wall seconds of one run each", flush=True)
for intercept in (False, True):
    for together in (False, True):
        ctx.synchronize()
        t0 = time.perf_counter()
        res = CV.logistic_cv(ctx, F, mus, folds=5, gap=1e-6, intercept=intercept, score_together=together)
        ctx.synchronize()
        print(f"intercept={intercept} score_together={together}: {time.perf_counter() - t0:.3f} s  best={res.best} one_se={res.one_se} "
              f"converged={int(res.converged.sum())}/{res.converged.numel()} mean loss {[round(float(v), 6) for v in res.mean]}", flush=True)
ctx.synchronize()
ctx.close()
