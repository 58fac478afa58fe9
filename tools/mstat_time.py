#!/usr/bin/env python3
"""Times the per-sample reduction (ciao_margin_stats: mstat_partial_kernel + mstat_final_kernel, csrc/mstat_kernels.h) beside the full pass
it follows, on cuda:0.  Device events after a warm-up, the median of CIAO_REPEATS (default 9) repeats.

  pass      ciao_full_gradient at N = CIAO_N (default 10^7), d = 1024, fp64: the bench's default problem (82 GB)
  stats     ciao_margin_stats at that N on a d = 1 problem (it reads dots and b only), both losses, both types, and its share of the pass
  cert      certificate() against certificate(samples=True) at d = 1024 and at d = 50, both losses

CIAO_PASS_ONLY=1: the first line only (so that a library without the new entry points -- the parent commit's, selected with
CIAO_HIP_LIB -- can be timed by the same script in the same session)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ciao_loader
ciao_loader.load()
from ciaoalgorithms_jl_amd import _lib as L
from ciaoalgorithms_jl_amd.device import Context, PackedF, ProxG

if os.environ.get("CIAO_PASS_ONLY"):      # a library from before the per-sample entry points: do not ask it for them
    for name in ("ciao_row_dots", "ciao_margin_stats", "ciao_certificate_samples"):
        L.SIGNATURES.pop(name, None)
torch.cuda.set_device(0)
ctx = Context(0)
dev = torch.device("cuda", 0)
N = int(float(os.environ.get("CIAO_N", "1e7")))
REPEATS = int(os.environ.get("CIAO_REPEATS", "9"))
which = os.environ.get("CIAO_HIP_LIB", "product library")


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
    A = torch.empty((N, d), dtype=dt, device=dev)
    ctx.synth_normal(A, 0, seed=7, scale=1.0 / np.sqrt(d))
    xt = torch.randn(d, dtype=dt, device=dev)
    b, y = torch.empty(N, dtype=dt, device=dev), torch.empty(N, dtype=dt, device=dev)
    Fls = PackedF.least_squares(A, b, float(N))
    ctx.synth_targets(Fls, xt, noise=0.01, labels=False, seed=7, b_out=b)
    Flg = PackedF.logistic(A, y)
    ctx.synth_targets(Flg, xt, noise=0.1, labels=True, seed=7, b_out=y)
    return Fls, Flg, 0.5 * xt


print(f"# {which}; N = {N}; median (min .. max) of {REPEATS} repeats, device events, ms", flush=True)
Fls, Flg, x = problem(1024, torch.float64)
av = torch.empty_like(x)
t_pass = median_ms(lambda: ctx.full_gradient(Fls, x, av))
print(f"pass  f64 d=1024 ls  ciao_full_gradient  {t_pass[0]:.3f} ({t_pass[1]:.3f} .. {t_pass[2]:.3f})  [{ctx.last_kernel()}]", flush=True)
if os.environ.get("CIAO_PASS_ONLY"):
    sys.exit(0)

for dt in (torch.float64, torch.float32):
    A1 = torch.ones((N, 1), dtype=dt, device=dev)
    dots = 4.0 * torch.randn(N, dtype=dt, device=dev)
    for loss in ("logistic", "ls"):
        b = torch.where(torch.randn(N, dtype=dt, device=dev) >= 0, 1.0, -1.0).to(dt) if loss == "logistic" else torch.randn(N, dtype=dt, device=dev)
        F1 = PackedF.logistic(A1, b) if loss == "logistic" else PackedF.least_squares(A1, b, 1.0)
        for s in ((1.0, 0.25) if loss == "logistic" else (1.0,)):
            t = median_ms(lambda: ctx.margin_stats(F1, dots, s))
            share = f"  = {100 * t[0] / t_pass[0]:.2f} % of the f64 d=1024 pass" if dt == torch.float64 else ""
            print(f"stats {'f64' if dt == torch.float64 else 'f32'} {loss} s={s}  ciao_margin_stats  {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}){share}  "
                  f"[{ctx.last_kernel()}]", flush=True)
    del A1, dots, b, F1

g = ProxG(L.PROX_L1, lam=1e-3)


def cert_lines(d, Fls, Flg, x):
    for loss, F in (("ls", Fls), ("logistic", Flg)):
        t0 = median_ms(lambda: ctx.certificate(F, g, x, 0.5))
        t1 = median_ms(lambda: ctx.certificate(F, g, x, 0.5, samples=True))
        print(f"cert  f64 d={d} {loss}  certificate() {t0[0]:.3f} ({t0[1]:.3f} .. {t0[2]:.3f})  certificate(samples=True) {t1[0]:.3f} "
              f"({t1[1]:.3f} .. {t1[2]:.3f})  = +{100 * (t1[0] - t0[0]) / t0[0]:.2f} %", flush=True)


cert_lines(1024, Fls, Flg, x)
del Fls, Flg, x, av
torch.cuda.empty_cache()
cert_lines(50, *problem(50, torch.float64))
ctx.synchronize()
ctx.close()
