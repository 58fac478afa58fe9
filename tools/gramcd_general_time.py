#!/usr/bin/env python3
"""Times the general coordinate-descent kernel (csrc/gramcdg_kernels.h, Context.gram_cd_general) on cuda:0 and
writes profiles/gramcd_general_kernel_times.txt (--out: another file).  A report: no ratio is promised.

One run on one box; every comparison comes from that run.  Each step is a fresh child process (this script with --shape ...) under its
own time limit (CIAO_STEP_SECONDS, default 300); a step that fails or runs out of time ends the run -- nothing more is started on the
device -- and is recorded as such.  The problems are tools/gramcd_time.py's: per d in 255, 1024, 4096, LeastSquares rows (CIAO_CD_N,
default 20000, Gaussian / sqrt(d), targets from a d / 5-sparse vector plus noise), the 8-model path mu_max 2^-k, k = 1 .. 8.  Seeded.

  1. defaults, new kernel against old: ONE launch of the 8 models, cold, tol = 1e-7 sum b^2, 1024 sweeps allowed, by device events, the
     median of CIAO_REPEATS (default 3) launches after a warm one: ciao_gram_cd, then ciao_gram_cd_general with the defaults, in the
     same process; their ratio; that the two results are the same bits.
  2. the non-negative path (lower = 0 for every coordinate), the same launch: with the product library, and -- where
     --plain-idle LIB names an experiment build with -DCIAO_GRAMCDG_PLAIN_IDLE (tools/exp_build.sh) -- with that library in a child of
     its own: what the sign-aware idle test buys.  Same bits either way (the test decides cost only).
  3. the d-space part of a 5-fold cross-validation plus refit for the 8 weights at gap 1e-6 (cv.lasso_cv_from_stats on the folds'
     statistics, made once): fused=True against fused=False, wall clock around a synchronise, median of the repeats after a warm run;
     with --parent-tree DIR (a built checkout of the parent commit) the parent's lasso_cv_from_stats on the same statistics too.
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [255, 1024, 4096]


def setup(tree):
    import torch
    sys.path.insert(0, tree)
    import ciao_loader
    ciao_loader.load()
    from ciaoalgorithms_jl_amd.device import Context
    torch.cuda.set_device(0)
    return Context(0), torch.device("cuda", 0)


def problem(ctx, dev, d):
    import numpy as np
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    N = int(float(os.environ.get("CIAO_CD_N", "20000")))
    torch.manual_seed(7)
    f64 = dict(dtype=torch.float64, device=dev)
    A = torch.empty((N, d), **f64)
    ctx.synth_normal(A, 0, seed=7, scale=1.0 / np.sqrt(d))
    b = torch.empty(N, **f64)
    F = PackedF.least_squares(A, b, float(N))
    x_true = torch.zeros(d, **f64)
    x_true[::5] = 2.0 * torch.randn(len(x_true[::5]), **f64)
    ctx.synth_targets(F, x_true, noise=0.1, labels=False, seed=7, b_out=b)
    return F


def one_shape(d, what, tree):
    import torch
    ctx, dev = setup(tree)
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd import gram as GR
    repeats = int(os.environ.get("CIAO_REPEATS", "3"))
    f64 = dict(dtype=torch.float64, device=dev)
    F = problem(ctx, dev, d)
    fmt = lambda t: f"{t[0]:.2f} ({t[1]:.2f} .. {t[2]:.2f})"
    flags = ctx.lib.ciao_build_flags().decode() or "product"

    def events(fn):
        ts = []
        for _ in range(repeats + 1):
            X = torch.zeros((8, d), **f64)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            e0.record()
            out = fn(X)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return out, statistics.median(ts[1:])

    if what in ("kernels", "nonneg"):
        st = GR.gram_stats(ctx, F)
        mus = [GR.mu_max(st) * 0.5 ** k for k in range(1, 9)]
        c = st.lam / st.N
        tau = torch.tensor([m / c for m in mus], **f64)
        diag = torch.diagonal(st.G)
        inv = torch.where(diag > 0, 1.0 / diag, torch.zeros_like(diag)).contiguous()
        tol = GR.CD_FIRST_TOL * st.sum_bb
        same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))
        if what == "kernels":
            (Xo, _, So), t_old = events(lambda X: ctx.gram_cd(st.G, st.u, inv, tau, X, tol, 1024, R=None))
            k_old = ctx.last_kernel()
            (Xn, _, Sn), t_new = events(lambda X: ctx.gram_cd_general(st.G, st.u, inv, tau, X, tol, 1024, R=None))
            S = Sn.cpu().numpy()
            print(f"f64 d={d} K=8 defaults, one launch, cold, tol {tol:.3g}: ciao_gram_cd {t_old:.3f} ms  ciao_gram_cd_general {t_new:.3f} ms  general / plain "
                  f"{t_new / t_old:.3f}  same bits {same(Xo, Xn) and same(So, Sn)}  sweeps {S[:, 0].astype(int).tolist()}  updates {S[:, 1].astype(int).tolist()}\n"
                  f"    [{k_old}]\n    [{ctx.last_kernel()}]", flush=True)
        else:
            lo = torch.zeros(d, **f64)
            (Xn, _, Sn), t_nn = events(lambda X: ctx.gram_cd_general(st.G, st.u, inv, tau, X, tol, 1024, lo=lo, R=None))
            S = Sn.cpu().numpy()
            digest = int(Xn.view(torch.int64).sum().item()) & 0xFFFFFFFF
            print(f"f64 d={d} K=8 non-negative ({flags}), one launch, cold: {t_nn:.3f} ms  sweeps {S[:, 0].astype(int).tolist()}  updates {S[:, 1].astype(int).tolist()}  "
                  f"states {S[:, 3].astype(int).tolist()}  nonzeros {[int((x != 0).sum()) for x in Xn]}  bits of X (sum of the words mod 2^32) {digest:08x}", flush=True)
    else:
        lists = CV.fold_lists(F.N, 5, seed=0, device=dev)
        stats = CV.fold_stats(ctx, F, lists)
        mus = [GR.mu_max(GR.add_stats(stats)) * 0.5 ** k for k in range(1, 9)]

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

        if what == "cv":
            one, t_one = wall(lambda: CV.lasso_cv_from_stats(stats, mus, ctx=ctx, fused=False))
            al, t_all = wall(lambda: CV.lasso_cv_from_stats(stats, mus, ctx=ctx, fused=True))
            eq = torch.equal(one.mse.view(torch.int64), al.mse.view(torch.int64)) and all(torch.equal(a, b) for a, b in zip(one.path.x, al.path.x))
            print(f"f64 d={d} 5 folds + refit, 8 weights, gap 1e-6, d-space part: fused=False {fmt(t_one)} ms  fused=True {fmt(t_all)} ms  fused / unfused "
                  f"{t_all[0] / t_one[0]:.3f}  same table and path {eq}  converged {sum(al.path.converged)}/8  best {al.best} one_se {al.one_se}\n"
                  f"    [{ctx.last_kernel()}]", flush=True)
        else:   # "cv-parent": the parent commit's tree has no fused keyword
            one, t_one = wall(lambda: CV.lasso_cv_from_stats(stats, mus, ctx=ctx))
            print(f"f64 d={d} 5 folds + refit, 8 weights, gap 1e-6, d-space part, the PARENT commit's tree: {fmt(t_one)} ms  best {one.best} one_se {one.one_se}",
                  flush=True)
    ctx.synchronize()
    ctx.close()


def main():
    arg = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
    if "--shape" in sys.argv:
        one_shape(int(arg("--shape")), arg("--what"), arg("--tree") or ROOT)
        return
    out = arg("--out") or os.path.join(ROOT, "profiles", "gramcd_general_kernel_times.txt")
    plain, parent = arg("--plain-idle"), arg("--parent-tree")
    limit = int(os.environ.get("CIAO_STEP_SECONDS", "300"))
    lines = [f"# tools/gramcd_general_time.py: single launches by device events, cross-validation by wall clock around a synchronise, median (min .. max) of "
             f"{os.environ.get('CIAO_REPEATS', '3')} repeats after a warm run, ms; one run, one box"]
    steps = []
    for d in SHAPES:
        steps.append((["--shape", str(d), "--what", "kernels"], {}))
        steps.append((["--shape", str(d), "--what", "nonneg"], {}))
        if plain:
            steps.append((["--shape", str(d), "--what", "nonneg"], {"CIAO_HIP_LIB": os.path.abspath(plain)}))
        steps.append((["--shape", str(d), "--what", "cv"], {}))
        if parent:
            steps.append((["--shape", str(d), "--what", "cv-parent", "--tree", os.path.abspath(parent)], {}))
    for step, env in steps:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), *step], capture_output=True, text=True, timeout=limit, env={**os.environ, **env})
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
