#!/usr/bin/env python3
"""Times the row pass of the step sizes from the data (ciao_row_sqnorms: rowsq_partial_kernel + rowsq_final_kernel, csrc/rowsq_kernels.h)
beside the full-gradient pass over the SAME PackedF, on cuda:0.  Device events after warm runs, the median of CIAO_REPEATS (default 11)
repeats.

  shape lines   d = 1024 fp64, d = 1024 fp32, d = 4096 fp32 (condition: the row pass takes at most 1.25 x the full-gradient pass),
                d = 50 and d = 255 fp32 / fp64 (recorded only), each at the largest N of CIAO_N (default 10^7, 5 10^6, 2 10^6) that fits;
                ms of both, their ratio, the achieved TB/s of N d sizeof(T) bytes; the row pass is timed with its N-vector and without
                (the summary alone, as lipschitz_max asks for it: that call waits for its four numbers, so its time is the host's)

ciao_full_gradient is what the library did before the row pass existed: the comparison needs no second library."""
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
from ciaoalgorithms_jl_amd.device import Context, PackedF

torch.cuda.set_device(0)
ctx = Context(0)
dev = torch.device("cuda", 0)
SIZES = [int(float(v)) for v in os.environ.get("CIAO_N", "1e7,5e6,2e6").split(",")]
REPEATS = int(os.environ.get("CIAO_REPEATS", "11"))
BUDGET = float(os.environ.get("CIAO_BYTES", "170e9"))     # the largest matrix tried


def median_ms(fn, warm=2):
    for _ in range(warm):
        fn()
    ctx.synchronize()
    ts = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def host_ms(fn, warm=2):
    """a call that synchronises: wall clock around it, the stream idle before"""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(REPEATS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def problem(d, dt):
    es = 8 if dt == torch.float64 else 4
    for N in SIZES:
        if N * d * es > BUDGET:
            continue
        try:
            A = torch.empty((N, d), dtype=dt, device=dev)
        except torch.OutOfMemoryError:
            continue
        ctx.synth_normal(A, 0, seed=7, scale=1.0 / np.sqrt(d))
        b = torch.empty(N, dtype=dt, device=dev)
        F = PackedF.least_squares(A, b, float(N))
        ctx.synth_targets(F, torch.randn(d, dtype=dt, device=dev), noise=0.01, labels=False, seed=7, b_out=b)
        return N, F
    raise SystemExit(f"no N of {SIZES} fits at d = {d}")


print(f"# median (min .. max) of {REPEATS} repeats, device events, ms; TB/s of N d sizeof(T) bytes", flush=True)
for d, dt, conditioned in ((1024, torch.float64, True), (1024, torch.float32, True), (4096, torch.float32, True),
                           (50, torch.float32, False), (50, torch.float64, False), (255, torch.float32, False), (255, torch.float64, False)):
    N, F = problem(d, dt)
    name = "f64" if dt == torch.float64 else "f32"
    x = 0.5 * torch.randn(d, dtype=dt, device=dev)
    av = torch.empty_like(x)
    out = torch.empty(N, dtype=torch.float64, device=dev)
    t_pass = median_ms(lambda: ctx.full_gradient(F, x, av))
    k_pass = ctx.last_kernel()
    t_row = median_ms(lambda: ctx.row_sqnorms(F, out))
    k_row = ctx.last_kernel()
    t_sum = host_ms(lambda: ctx.row_sqnorm_stats(F))
    nbytes = N * d * (8 if dt == torch.float64 else 4)
    ratio = t_row[0] / t_pass[0]
    verdict = ("  condition <= 1.25: " + ("met" if ratio <= 1.25 else "MISSED")) if conditioned else "  (recorded only)"
    print(f"{name} d={d} N={N}  ciao_full_gradient {t_pass[0]:.3f} ({t_pass[1]:.3f} .. {t_pass[2]:.3f}) = {nbytes / t_pass[0] * 1e-9:.2f} TB/s  "
          f"ciao_row_sqnorms {t_row[0]:.3f} ({t_row[1]:.3f} .. {t_row[2]:.3f}) = {nbytes / t_row[0] * 1e-9:.2f} TB/s  ratio {ratio:.3f}{verdict}\n"
          f"    summary alone (host clock, synchronises) {t_sum[0]:.3f} ({t_sum[1]:.3f} .. {t_sum[2]:.3f})\n"
          f"    [{k_pass}] [{k_row}]", flush=True)
    del F, x, av, out
    torch.cuda.empty_cache()
ctx.synchronize()
ctx.close()
