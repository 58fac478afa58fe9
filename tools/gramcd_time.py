#!/usr/bin/env python3
"""Times the coordinate-descent route of the d-space lasso (csrc/gramcd_kernels.h, gram.lasso_cd) against the FISTA route (gram.lasso_path)
on cuda:0 and writes profiles/gramcd_kernel_times.txt (--out: another file).  A report: no ratio is promised.

One run on one box; every comparison comes from that run.  Each step is a fresh child process (this script with --shape / --newton-step)
under its own time limit (CIAO_STEP_SECONDS, default 420); a step that fails or runs out of time ends the run -- nothing more is started
on the device -- and is recorded as such.

Per d in 255, 1024, 4096: LeastSquares rows (CIAO_CD_N rows, default 20000, Gaussian / sqrt(d), targets from a d / 5-sparse vector plus
noise), their statistics from gram_stats on the device, and the 8-model path mu_max 2^-k, k = 1 .. 8, to the relative gap 1e-9, every
tensor on the device, wall clock around a synchronise, the median of CIAO_REPEATS (default 3) repeats after a warm run:
    lasso_path(method="cd", ctx=ctx)      sweeps over all models, launches
    lasso_path(method="fista")            iterations (with its eigvalsh for the step)
and one ciao_gram_cd launch of the 8 models alone (cold start, tol = 1e-7 sum b^2, 1024 sweeps allowed), device events: per model its
sweeps and non-zero updates; the launch's time over the LONGEST model's updates is the time per update (the models run side by side),
updates / sweeps the updates per sweep; and the sparsest model (k = 1) launched alone.  Seeded: two runs time the same problems.

--newton-step (after the shapes; alone with --newton-only): logistic rows at d = 1024 fp64, N = CIAO_NEWTON_N (default 10^7), mu = 0.1
mu_max, gap CIAO_NEWTON_GAP (default 1e-6), as tools/gram_time.py --newton: one newton.logistic_newton solve with subproblem="fista" (the
default) and one with subproblem="cd", wall clock."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [255, 1024, 4096]
GAP = 1e-9


def setup():
    import torch
    sys.path.insert(0, ROOT)
    import ciao_loader
    ciao_loader.load()
    from ciaoalgorithms_jl_amd.device import Context
    torch.cuda.set_device(0)
    return Context(0), torch.device("cuda", 0)


def one_shape(d):
    import numpy as np
    import torch
    ctx, dev = setup()
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.device import PackedF
    N = int(float(os.environ.get("CIAO_CD_N", "20000")))
    torch.manual_seed(7)
    repeats = int(os.environ.get("CIAO_REPEATS", "3"))
    f64 = dict(dtype=torch.float64, device=dev)
    A = torch.empty((N, d), **f64)
    ctx.synth_normal(A, 0, seed=7, scale=1.0 / np.sqrt(d))
    b = torch.empty(N, **f64)
    F = PackedF.least_squares(A, b, float(N))
    x_true = torch.zeros(d, **f64)
    x_true[::5] = 2.0 * torch.randn(len(x_true[::5]), **f64)
    ctx.synth_targets(F, x_true, noise=0.1, labels=False, seed=7, b_out=b)
    st = GR.gram_stats(ctx, F)
    mus = [GR.mu_max(st) * 0.5 ** k for k in range(1, 9)]

    def wall(fn):
        fn()
        ts = []
        for _ in range(repeats):
            ctx.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ctx.synchronize()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return out, (statistics.median(ts), min(ts), max(ts))

    fmt = lambda t: f"{t[0]:.2f} ({t[1]:.2f} .. {t[2]:.2f})"
    cd, t_cd = wall(lambda: GR.lasso_path(st, mus, gap=GAP, method="cd", ctx=ctx))
    fi, t_fi = wall(lambda: GR.lasso_path(st, mus, gap=GAP, method="fista"))
    worst = max(abs(a.objective - c.objective) / max(1.0, a.objective) for a, c in zip(cd.certificates, fi.certificates))
    # one launch alone
    c = st.lam / st.N
    tau = torch.tensor([m / c for m in mus], **f64)
    diag = torch.diagonal(st.G)
    inv = torch.where(diag > 0, 1.0 / diag, torch.zeros_like(diag)).contiguous()
    tol = GR.CD_FIRST_TOL * st.sum_bb
    ts = []
    for _ in range(repeats + 1):
        X = torch.zeros((len(mus), d), **f64)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        e0.record()
        _, _, stat = ctx.gram_cd(st.G, st.u, inv, tau, X, tol, 1024, R=None)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    t_k = statistics.median(ts[1:])
    stat = stat.cpu().numpy()
    longest = float(stat[:, 1].max())
    ts1 = []
    for _ in range(repeats + 1):                  # the sparsest model alone: what a sweep over mostly idle coordinates costs
        X = torch.zeros((1, d), **f64)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        e0.record()
        _, _, stat1 = ctx.gram_cd(st.G, st.u, inv, tau[:1].contiguous(), X, tol, 1024, R=None)
        e1.record()
        e1.synchronize()
        ts1.append(e0.elapsed_time(e1))
    t_1 = statistics.median(ts1[1:])
    stat1 = stat1.cpu().numpy()
    print(f"f64 d={d} N={N} K={len(mus)} gap {GAP:g}  lasso_path(cd) {fmt(t_cd)} ms, sweeps (all models) {cd.iterations}, converged {sum(cd.converged)}/{len(mus)}  "
          f"lasso_path(fista) {fmt(t_fi)} ms, iterations {fi.iterations}, converged {sum(fi.converged)}/{len(mus)}  cd / fista {t_cd[0] / t_fi[0]:.3f}  "
          f"max relative objective difference {worst:.1e}  nonzeros {[int((x != 0).sum()) for x in cd.x]}\n"
          f"    one launch, cold, tol {tol:.3g}: {t_k:.3f} ms  sweeps {stat[:, 0].astype(int).tolist()}  updates {stat[:, 1].astype(int).tolist()}  "
          f"states {stat[:, 3].astype(int).tolist()}  time per update of the longest model {1e3 * t_k / max(longest, 1.0):.2f} us  "
          f"updates per sweep {[round(float(u / s), 1) for u, s in zip(stat[:, 1], stat[:, 0])]}\n"
          f"    the sparsest model alone: {1e3 * t_1:.1f} us for {int(stat1[0, 0])} sweeps and {int(stat1[0, 1])} updates\n    [{ctx.last_kernel()}]", flush=True)
    ctx.synchronize()
    ctx.close()


def newton_step():
    import numpy as np
    import torch
    ctx, dev = setup()
    from ciaoalgorithms_jl_amd.device import PackedF
    from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_mu_max, logistic_newton
    d, N = 1024, int(float(os.environ.get("CIAO_NEWTON_N", "1e7")))
    gap = float(os.environ.get("CIAO_NEWTON_GAP", "1e-6"))
    torch.manual_seed(7)
    A = torch.empty((N, d), dtype=torch.float64, device=dev)
    ctx.synth_normal(A, 0, seed=7, scale=1.0 / np.sqrt(d))
    y = torch.empty(N, dtype=torch.float64, device=dev)
    F = PackedF.logistic(A, y)
    x_true = torch.zeros(d, dtype=torch.float64, device=dev)
    x_true[::5] = 4.0 * torch.randn(len(x_true[::5]), dtype=torch.float64, device=dev)
    ctx.synth_targets(F, x_true, noise=0.0, labels=True, seed=7, b_out=y)
    rows = DeviceRows(ctx, F)
    mu = 0.1 * logistic_mu_max(rows)
    logistic_newton(rows, mu, gap=gap, max_outer=1, subproblem="cd")       # warm: code objects, the workspace of the Gram pass
    for sub in ("fista", "cd", "fista", "cd"):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = logistic_newton(rows, mu, gap=gap, subproblem=sub)
        ctx.synchronize()
        t = time.perf_counter() - t0
        c = r.certificate
        print(f"logistic_newton(subproblem={sub!r}) f64 d={d} N={N} mu=0.1 mu_max gap asked {gap:g}: {t:.2f} s wall, outer {r.outer}, passes gram "
              f"{r.passes.gram} first-order {r.passes.first_order}, {r.reason}, gap {c.gap:.3e}, objective {c.objective:.9f}, nonzeros {int((r.x != 0).sum())}",
              flush=True)
    ctx.synchronize()
    ctx.close()


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "--shape":
        one_shape(int(sys.argv[2]))
        return
    if len(sys.argv) >= 2 and sys.argv[1] == "--newton-step":
        newton_step()
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "gramcd_kernel_times.txt")
    limit = int(os.environ.get("CIAO_STEP_SECONDS", "420"))
    lines = [f"# tools/gramcd_time.py: wall clock around a synchronise, median (min .. max) of {os.environ.get('CIAO_REPEATS', '3')} repeats after a warm "
             "run, ms; the single launch by device events; one run, one box"]
    steps = [] if "--newton-only" in sys.argv else [["--shape", str(d)] for d in SHAPES]
    if "--no-newton" not in sys.argv:
        steps.append(["--newton-step"])
    for step in steps:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), *step], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{' '.join(step)}: no result within {limit} s; the run ends here")
            break
        if r.returncode != 0:
            lines.append(f"{' '.join(step)}: exit status {r.returncode}; the run ends here\n    " + r.stderr.strip().replace("\n", "\n    ")[-2000:])
            break
        lines.append(r.stdout.rstrip())
        print(r.stdout.rstrip(), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
