#!/usr/bin/env python3
"""Times the two passes of column standardisation (csrc/colmom_kernels.h) on cuda:0.  Device events after warm runs, the median of
CIAO_REPEATS (default 11) repeats.

  moments lines   ciao_col_moments (colmom_partial_kernel + colmom_final_kernel) beside the full-gradient pass over the SAME PackedF:
                  d = 1024 fp64, d = 1024 fp32, d = 4096 fp32 (condition: the moments pass takes at most 1.25 x the full-gradient pass),
                  d = 50 and d = 255 fp32 / fp64 (recorded only), each at the largest N of CIAO_N (default 10^7, 5 10^6, 2 10^6) that
                  fits; ms of both, their ratio, the achieved TB/s of N d sizeof(T) bytes
  scaling lines   ciao_scale_columns in place (colscale_kernel) beside torch's A.sub_(c).mul_(s) on the same tensor -- what there was before
                  the kernel: two passes, each N d read and N d written -- at the three conditioned shapes (condition: the kernel is
                  faster); the TB/s of the kernel's 2 N d sizeof(T) bytes, to set beside the mixed read / write ceiling of
                  profiles/r05_box_ceilings.txt (recorded only)

ciao_full_gradient and torch's own operations are what existed before these passes: the comparison needs no second library."""
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


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


print(f"# median (min .. max) of {REPEATS} repeats, device events, ms; TB/s of N d sizeof(T) bytes (scaling: of 2 N d sizeof(T))", flush=True)
for d, dt, conditioned in ((1024, torch.float64, True), (1024, torch.float32, True), (4096, torch.float32, True),
                           (50, torch.float32, False), (50, torch.float64, False), (255, torch.float32, False), (255, torch.float64, False)):
    N, F = problem(d, dt)
    name = "f64" if dt == torch.float64 else "f32"
    x = 0.5 * torch.randn(d, dtype=dt, device=dev)
    av = torch.empty_like(x)
    s1, s2 = (torch.empty(d, dtype=torch.float64, device=dev) for _ in range(2))
    t_pass = median_ms(lambda: ctx.full_gradient(F, x, av))
    k_pass = ctx.last_kernel()
    t_mom = median_ms(lambda: ctx.col_moments(F, None, s1, s2))
    k_mom = ctx.last_kernel()
    nbytes = N * d * (8 if dt == torch.float64 else 4)
    ratio = t_mom[0] / t_pass[0]
    verdict = ("  condition <= 1.25: " + ("met" if ratio <= 1.25 else "MISSED")) if conditioned else "  (recorded only)"
    print(f"{name} d={d} N={N}  ciao_full_gradient {fmt(t_pass)} = {nbytes / t_pass[0] * 1e-9:.2f} TB/s  "
          f"ciao_col_moments {fmt(t_mom)} = {nbytes / t_mom[0] * 1e-9:.2f} TB/s  ratio {ratio:.3f}{verdict}\n"
          f"    [{k_pass}] [{k_mom}]", flush=True)
    if conditioned:
        # centre and scale close to 0 and 1: the repeats work on their own output, which must stay finite
        c = 1e-3 * torch.randn(d, dtype=torch.float64, device=dev)
        s = 1.0 + 1e-3 * torch.randn(d, dtype=torch.float64, device=dev)
        ct, st = c.to(dt), s.to(dt)
        t_torch = median_ms(lambda: F.A.sub_(ct).mul_(st))
        t_scale = median_ms(lambda: ctx.scale_columns(F, c, s, inplace=True))
        k_scale = ctx.last_kernel()
        assert bool(torch.isfinite(F.A[:4]).all())
        faster = t_scale[0] < t_torch[0]
        print(f"{name} d={d} N={N}  torch A.sub_(c).mul_(s) {fmt(t_torch)}  ciao_scale_columns in place {fmt(t_scale)} = "
              f"{2 * nbytes / t_scale[0] * 1e-9:.2f} TB/s  torch / kernel {t_torch[0] / t_scale[0]:.2f}  condition faster: "
              f"{'met' if faster else 'MISSED'}\n    [{k_scale}]", flush=True)
    del F, x, av, s1, s2
    torch.cuda.empty_cache()
ctx.synchronize()
ctx.close()
