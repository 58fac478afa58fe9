#!/usr/bin/env python3
"""Times the first-order passes over a list of rows (ciao_list_dots, ciao_list_combine; csrc/list_kernels.h) on cuda:0 and writes
profiles/list_passes_kernel_times.txt (--out: another file).  Follows tools/gram_rows_time.py.

ONE run on one box; every comparison comes from that run.  Each shape is a STEP: a fresh child process (this script with --shape) under
its own time limit (CIAO_STEP_SECONDS, default 300); a step that fails or runs out of time ends the run -- nothing more is started on the
device -- and is recorded as such.  Shapes, at the largest N of CIAO_N (default 10^7, 5 10^6, 2 10^6) that fits:

    d = 1024 fp64, d = 1024 fp32, d = 255 fp64

Per shape, device events after a warm run, the median of CIAO_REPEATS (default 5) repeats, ms:
    ciao_row_sqnorms, ciao_col_sqnorms      the two norm passes: the same bytes, kernels this change does not touch
    list_dots / list_combine, no list       idx = NULL
    ... identity list                       idx = 0 .. N-1
    ... sorted random 80 % / 20 %           rows drawn without repeats, ascending (a training fold and its held-out rows)
    torch, the same lists                   A.index_select(0, idx) @ x and A.index_select(0, idx).T @ c: a gathered copy, then the product
With CIAO_HIP_LIB_X_CACHE naming an experiment build (make EXP=... EXTRA=-DCIAO_LISTDOT_X_CACHE: x of listdot_kernel read through the
cache, not from LDS) a further child times list_dots on that library in the same run.

The last step is one cv.logistic_cv (5 folds, 4 weights, d = 255 fp64): total time and pass counts only."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1024, "f64"), (1024, "f32"), (255, "f64")]


def setup(d, name):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import ciao_loader
    ciao_loader.load()
    from ciaoalgorithms_jl_amd.device import Context, PackedF
    torch.cuda.set_device(0)
    ctx = Context(0)
    dev = torch.device("cuda", 0)
    dt = torch.float64 if name == "f64" else torch.float32
    es = 8 if name == "f64" else 4
    sizes = [int(float(v)) for v in os.environ.get("CIAO_N", "1e7,5e6,2e6").split(",")]
    budget = float(os.environ.get("CIAO_BYTES", "100e9"))
    for N in sizes:
        if N * d * es > budget:
            continue
        try:
            A = torch.empty((N, d), dtype=dt, device=dev)
        except torch.OutOfMemoryError:
            continue
        ctx.synth_normal(A, 0, seed=7, scale=1.0 / np.sqrt(d))
        b = torch.empty(N, dtype=dt, device=dev)
        F = PackedF.logistic(A, b)
        ctx.synth_targets(F, torch.randn(d, dtype=dt, device=dev), noise=0.5, labels=True, seed=7, b_out=b)
        return ctx, F, N, dt
    raise SystemExit(f"no N of {sizes} fits at d = {d}")


def timer(ctx):
    import torch
    repeats = int(os.environ.get("CIAO_REPEATS", "5"))

    def median_ms(fn, warm=1):
        for _ in range(warm):
            fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        ts = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)
    return median_ms


fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def lists_of(N, dev):
    import torch
    gen = torch.Generator(device="cpu")
    gen.manual_seed(11)
    perm = torch.randperm(N, generator=gen)
    cut = N // 5
    return {"identity": torch.arange(N, dtype=torch.int64, device=dev), "80 %": torch.sort(perm[cut:]).values.contiguous().to(dev),
            "20 %": torch.sort(perm[:cut]).values.contiguous().to(dev)}


def one_shape(d, name, x_cache_only=False):
    import torch
    ctx, F, N, dt = setup(d, name)
    dev = F.A.device
    median_ms = timer(ctx)
    x = torch.randn(d, dtype=dt, device=dev)
    lists = lists_of(N, dev)
    out_n = torch.empty(N, dtype=torch.float64, device=dev)
    out_d = torch.empty(d, dtype=torch.float64, device=dev)
    c = torch.randn(N, dtype=torch.float64, device=dev)
    if x_cache_only:
        flags = ctx.lib.ciao_build_flags().decode()
        t0 = median_ms(lambda: ctx.list_dots(F, x, out=out_n))
        r = lists["80 %"]
        t1 = median_ms(lambda: ctx.list_dots(F, x, rows=r, out=out_n[:len(r)], check_rows=False))
        print(f"    x through the cache [{flags}]: list_dots no list {fmt(t0)}  80 % {fmt(t1)}", flush=True)
        ctx.close()
        return
    t_row = median_ms(lambda: ctx.row_sqnorms(F, out_n))
    t_col = median_ms(lambda: ctx.col_sqnorms(F, out_d))
    t_dn = median_ms(lambda: ctx.list_dots(F, x, out=out_n))
    k_d = ctx.last_kernel()
    whole_d = out_n.clone()
    t_cn = median_ms(lambda: ctx.list_combine(F, c, out=out_d))
    k_c = ctx.last_kernel()
    whole_c = out_d.clone()
    res = {}
    for lname, r in lists.items():
        M = len(r)
        cm = c[:M].contiguous()
        res[lname, "dots"] = median_ms(lambda: ctx.list_dots(F, x, rows=r, out=out_n[:M], check_rows=False))
        if lname == "identity":
            same_d = torch.equal(out_n.view(torch.int64), whole_d.view(torch.int64))
            k_dr = ctx.last_kernel()
        res[lname, "comb"] = median_ms(lambda: ctx.list_combine(F, cm, rows=r, out=out_d, check_rows=False))
        if lname == "identity":
            same_c = torch.equal(out_d.view(torch.int64), whole_c.view(torch.int64))
            k_cr = ctx.last_kernel()
    tor = {}
    cT = c.to(dt)
    for lname in ("80 %", "20 %"):
        r = lists[lname]
        M = len(r)
        cm = cT[:M].contiguous()
        tor[lname, "dots"] = median_ms(lambda: F.A.index_select(0, r) @ x)
        tor[lname, "comb"] = median_ms(lambda: F.A.index_select(0, r).T @ cm)
    t_row2 = median_ms(lambda: ctx.row_sqnorms(F, out_n))
    t_col2 = median_ms(lambda: ctx.col_sqnorms(F, out_d))
    rb, cb = min(t_row[0], t_row2[0]), min(t_col[0], t_col2[0])
    nbytes = N * d * (8 if name == "f64" else 4)
    tbs = lambda ms, frac=1.0: f"{frac * nbytes / ms * 1e-9:.2f} TB/s"
    print(f"{name} d={d} N={N}  ciao_row_sqnorms {fmt(t_row)} again {fmt(t_row2)} = {tbs(rb)}  ciao_col_sqnorms {fmt(t_col)} again {fmt(t_col2)} = {tbs(cb)}\n"
          f"    list_dots no list {fmt(t_dn)} = {tbs(t_dn[0])}  / ciao_row_sqnorms {t_dn[0] / rb:.3f}   identity list {fmt(res['identity', 'dots'])}  / ciao_row_sqnorms {res['identity', 'dots'][0] / rb:.3f}  same bits: {same_d}\n"
          f"    list_combine no list {fmt(t_cn)} = {tbs(t_cn[0])}  / ciao_col_sqnorms {t_cn[0] / cb:.3f}   identity list {fmt(res['identity', 'comb'])}  / ciao_col_sqnorms {res['identity', 'comb'][0] / cb:.3f}  same bits: {same_c}\n"
          + "".join(f"    sorted random {l}: list_dots {fmt(res[l, 'dots'])} = {tbs(res[l, 'dots'][0], f)}  torch index_select @ x {fmt(tor[l, 'dots'])}  list / torch {res[l, 'dots'][0] / tor[l, 'dots'][0]:.3f}\n"
                    f"    sorted random {l}: list_combine {fmt(res[l, 'comb'])} = {tbs(res[l, 'comb'][0], f)}  torch index_select.T @ c {fmt(tor[l, 'comb'])}  list / torch {res[l, 'comb'][0] / tor[l, 'comb'][0]:.3f}\n"
                    for l, f in (("80 %", 0.8), ("20 %", 0.2)))
          + f"    [{k_d}]\n    [{k_dr}]\n    [{k_c}]\n    [{k_cr}]", flush=True)
    ctx.synchronize()
    ctx.close()


def one_cv():
    import torch
    ctx, F, N, dt = setup(255, "f64")
    from ciaoalgorithms_jl_amd.cv import logistic_cv
    from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_mu_max
    top = logistic_mu_max(DeviceRows(ctx, F))
    mus = [f * top for f in (0.5, 0.25, 0.1, 0.03)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = logistic_cv(ctx, F, mus, folds=5, seed=0, gap=1e-6)
    torch.cuda.synchronize()
    dt_s = time.perf_counter() - t0
    print(f"logistic_cv f64 d=255 N={N}, 5 folds x 4 weights, gap 1e-6: {dt_s:.2f} s in all; converged {int(res.converged.sum())} of {res.converged.numel()} fold solves; "
          f"best {res.best} one_se {res.one_se}; mean held-out log-loss {[round(float(v), 6) for v in res.mean]}\n"
          f"    the refit on all rows: (Gram passes, first-order passes) per weight {[tuple(r.passes) for r in res.path]}", flush=True)
    ctx.close()


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--shape":
        one_shape(int(sys.argv[2]), sys.argv[3], x_cache_only="--x-cache" in sys.argv)
        return
    if len(sys.argv) >= 2 and sys.argv[1] == "--cv":
        one_cv()
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "list_passes_kernel_times.txt")
    limit = int(os.environ.get("CIAO_STEP_SECONDS", "300"))
    lines = [f"# tools/list_passes_time.py: median (min .. max) of {os.environ.get('CIAO_REPEATS', '5')} repeats, device events, ms; ONE run, one box"]
    alt = os.environ.get("CIAO_HIP_LIB_X_CACHE")
    steps = []
    for d, name in SHAPES:
        steps.append((f"{name} d={d}", ["--shape", str(d), name], None))
        if alt:
            steps.append((f"{name} d={d} x through the cache", ["--shape", str(d), name, "--x-cache"], alt))
    steps.append(("logistic_cv", ["--cv"], None))
    for what, args, lib in steps:
        env = dict(os.environ)
        if lib:
            env["CIAO_HIP_LIB"] = lib
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit, env=env)
        except subprocess.TimeoutExpired:
            lines.append(f"{what}: no result within {limit} s; the run ends here")
            break
        if r.returncode != 0:
            lines.append(f"{what}: exit status {r.returncode}; the run ends here\n    " + r.stderr.strip().replace("\n", "\n    ")[-2000:])
            break
        lines.append(r.stdout.rstrip())
        print(r.stdout.rstrip(), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
