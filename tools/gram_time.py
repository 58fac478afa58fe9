#!/usr/bin/env python3
"""Times the Gram statistics (csrc/gram_kernels.h) on cuda:0 and writes profiles/gram_weighted_kernel_times.txt (--out: another file;
profiles/gram_kernel_times.txt is the record of the run before the weighted column existed and is not written any more).

One run on one box; every comparison comes from that run.  Each shape is a STEP: a fresh child process (this script with --shape) under
its own time limit (CIAO_STEP_SECONDS, default 420); a step that fails or runs out of time ends the run -- nothing more is started on the
device -- and is recorded as such.  Shapes, at the largest N of CIAO_N (default 10^7, 5 10^6, 2 10^6) that fits:

    d = 1024 fp64 (the condition), d = 1024 fp32, d = 4096 fp32, d = 50 fp64, d = 255 fp64

Per shape, device events after a warm run, the median of CIAO_REPEATS (default 5) repeats, ms:
    ciao_gram                  G, u, colsum, bsum in one call (gram_partial_kernel + gram_final_kernel)
    ciao_gram_weighted         the same call with a weight per row (uniform in [0, 1)) on the same matrix, and its ratio to ciao_gram:
                               the same MFMAs, one multiply per parked element of one panel, 8 N bytes of weights per tile column
    torch A.T @ A              in A's dtype: what there was before the kernel, for G alone
    torch A.T @ b + sums       A.T @ b, A.sum(0), b.sum(), (b * b).sum(): the further passes that route needs
    ciao_full_gradient         one pass over the same rows (the HBM yardstick)
    stepsize.smoothness        what smoothness_exact replaces (wall clock: it synchronises)
    fraction of the fp64 MFMA peak: N d (d + 1) flops (the upper triangle, which is all the kernel owes) / time / 78.6 TFLOP/s

The one condition: at d = 1024 fp64 ciao_gram takes no longer than torch's A.T @ A alone.

--newton (a step of its own, after the shapes; alone with `--newton-only`): logistic rows at d = 1024 fp64, labels from a sparse
logistic model, mu = 0.1 mu_max: the wall time of one newton.logistic_newton solve to CIAO_NEWTON_GAP (default 1e-6), then SVRG
(m = N, gamma = 1 / (7 L_max)) from x = 0, the certificate taken after every epoch, until the same gap or CIAO_SVRG_EPOCHS (default
12) epochs.  A report: no figure is promised."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1024, "f64", True), (1024, "f32", False), (4096, "f32", False), (50, "f64", False), (255, "f64", False)]
PEAK = 78.6e12


def one_shape(d, name):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import ciao_loader
    ciao_loader.load()
    from ciaoalgorithms_jl_amd.device import Context, PackedF
    from ciaoalgorithms_jl_amd.stepsize import smoothness
    torch.cuda.set_device(0)
    ctx = Context(0)
    dev = torch.device("cuda", 0)
    dt = torch.float64 if name == "f64" else torch.float32
    es = 8 if name == "f64" else 4
    sizes = [int(float(v)) for v in os.environ.get("CIAO_N", "1e7,5e6,2e6").split(",")]
    repeats = int(os.environ.get("CIAO_REPEATS", "5"))
    budget = float(os.environ.get("CIAO_BYTES", "170e9"))

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

    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    F = None
    for N in sizes:
        if N * d * es > budget:
            continue
        try:
            A = torch.empty((N, d), dtype=dt, device=dev)
        except torch.OutOfMemoryError:
            continue
        ctx.synth_normal(A, 0, seed=7, scale=1.0 / np.sqrt(d))
        b = torch.empty(N, dtype=dt, device=dev)
        F = PackedF.least_squares(A, b, float(N))
        ctx.synth_targets(F, torch.randn(d, dtype=dt, device=dev), noise=0.01, labels=False, seed=7, b_out=b)
        break
    if F is None:
        raise SystemExit(f"no N of {sizes} fits at d = {d}")
    G = torch.empty((d, d), dtype=torch.float64, device=dev)
    u, cs, bs, bs3 = (torch.empty(n, dtype=torch.float64, device=dev) for n in (d, d, 2, 3))
    t_gram = median_ms(lambda: ctx.gram(F, G, u, cs, bs))
    k_gram = ctx.last_kernel()
    w = torch.rand(N, dtype=torch.float64, device=dev)
    t_wgram = median_ms(lambda: ctx.gram(F, G, u, cs, bs3, weights=w))
    k_wgram = ctx.last_kernel()
    t_gram2 = median_ms(lambda: ctx.gram(F, G, u, cs, bs))      # ciao_gram again, after the weighted call: the same run's drift
    out = torch.empty((d, d), dtype=dt, device=dev)
    t_ata = median_ms(lambda: torch.matmul(A.T, A, out=out))
    rel = float((out.double() - G).abs().max() / G.abs().max())
    t_atb = median_ms(lambda: (A.T @ b, A.sum(0), b.sum(), (b * b).sum()))
    x = 0.5 * torch.randn(d, dtype=dt, device=dev)
    av = torch.empty_like(x)
    t_pass = median_ms(lambda: ctx.full_gradient(F, x, av))
    t0 = time.perf_counter()
    est, upper = smoothness(ctx, F)
    t_smooth = (time.perf_counter() - t0) * 1e3
    frac = N * d * (d + 1) / (t_gram[0] * 1e-3) / PEAK
    print(f"{name} d={d} N={N}  ciao_gram {fmt(t_gram)}  ciao_gram_weighted {fmt(t_wgram)}  ciao_gram again {fmt(t_gram2)}  "
          f"weighted / unweighted {t_wgram[0] / min(t_gram[0], t_gram2[0]):.3f}  torch A.T @ A {fmt(t_ata)}  torch A.T @ b + sums {fmt(t_atb)}  "
          f"ciao_full_gradient {fmt(t_pass)}  stepsize.smoothness {t_smooth:.1f}  "
          f"ciao_gram / (A.T @ A) {t_gram[0] / t_ata[0]:.3f}  fraction of the fp64 MFMA peak {frac:.3f}  max |A.T @ A - G| / max |G| {rel:.1e}\n"
          f"    [{k_gram}]\n    [{k_wgram}]", flush=True)
    ctx.synchronize()
    ctx.close()


def newton_step():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import ciao_loader
    ciao_loader.load()
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import solvers as S
    from ciaoalgorithms_jl_amd.device import Context, PackedF, ProxG
    from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_mu_max, logistic_newton
    from ciaoalgorithms_jl_amd.sampling import IndexStream
    from ciaoalgorithms_jl_amd.stepsize import lipschitz_max
    torch.cuda.set_device(0)
    ctx = Context(0)
    dev = torch.device("cuda", 0)
    d, N = 1024, int(float(os.environ.get("CIAO_NEWTON_N", "1e7")))
    gap = float(os.environ.get("CIAO_NEWTON_GAP", "1e-6"))
    A = torch.empty((N, d), dtype=torch.float64, device=dev)
    ctx.synth_normal(A, 0, seed=7, scale=1.0 / np.sqrt(d))
    y = torch.empty(N, dtype=torch.float64, device=dev)
    F = PackedF.logistic(A, y)
    x_true = torch.zeros(d, dtype=torch.float64, device=dev)
    x_true[::5] = 4.0 * torch.randn(len(x_true[::5]), dtype=torch.float64, device=dev)
    ctx.synth_targets(F, x_true, noise=0.0, labels=True, seed=7, b_out=y)
    rows = DeviceRows(ctx, F)
    mu = 0.1 * logistic_mu_max(rows)
    ctx.synchronize()
    t0 = time.perf_counter()
    r = logistic_newton(rows, mu, gap=gap)
    ctx.synchronize()
    t_newton = time.perf_counter() - t0
    c = r.certificate
    print(f"logistic_newton f64 d={d} N={N} mu=0.1 mu_max gap asked {gap:g}: {t_newton:.2f} s wall, outer {r.outer}, passes gram {r.passes.gram} "
          f"first-order {r.passes.first_order}, {r.reason}, gap {c.gap:.3e}, objective {c.objective:.9f}, nonzeros {int((r.x != 0).sum())}", flush=True)
    g = ProxG(L.PROX_L1, lam=mu)
    gamma = 1.0 / (7.0 * lipschitz_max(ctx, F))
    epochs = int(os.environ.get("CIAO_SVRG_EPOCHS", "12"))
    it = iter(S.iterator(S.SVRG(np.float64, γ=gamma), np.zeros(d), F=F, g=g, N=N, ctx=ctx, stream=IndexStream(1)))
    t0 = time.perf_counter()
    t_cert, reached = 0.0, None
    for k in range(1, epochs + 1):
        state = next(it)
        ctx.synchronize()
        t1 = time.perf_counter()
        cs = ctx.certificate(F, g, S.solution(state), gamma, samples=True)
        t_cert += time.perf_counter() - t1
        print(f"    SVRG epoch {k}: {time.perf_counter() - t0 - t_cert:.2f} s (certificates excluded), gap {cs.gap:.3e}, objective {cs.objective:.9f}", flush=True)
        if cs.gap <= gap * max(1.0, cs.objective):
            reached = k
            break
    t_svrg = time.perf_counter() - t0 - t_cert
    print(f"SVRG (m = N, gamma = 1 / (7 L_max)) to the same gap: " + (f"{reached} epochs, {t_svrg:.2f} s" if reached else
          f"not reached in {epochs} epochs ({t_svrg:.2f} s): gap {cs.gap:.3e}") + f"; logistic_newton / SVRG so far {t_newton / t_svrg:.3f}", flush=True)
    ctx.synchronize()
    ctx.close()


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--shape":
        one_shape(int(sys.argv[2]), sys.argv[3])
        return
    if len(sys.argv) >= 2 and sys.argv[1] == "--newton-step":
        newton_step()
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "gram_weighted_kernel_times.txt")
    limit = int(os.environ.get("CIAO_STEP_SECONDS", "420"))
    lines = [f"# tools/gram_time.py: median (min .. max) of {os.environ.get('CIAO_REPEATS', '5')} repeats, device events, ms; one run, one box"]
    verdict = "the condition (d = 1024 fp64: ciao_gram <= torch A.T @ A): not measured"
    failed = False
    for d, name, conditioned in ([] if "--newton-only" in sys.argv else SHAPES):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(d), name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name} d={d}: no result within {limit} s; the run ends here")
            failed = True
            break
        if r.returncode != 0:
            lines.append(f"{name} d={d}: exit status {r.returncode}; the run ends here\n    " + r.stderr.strip().replace("\n", "\n    ")[-2000:])
            failed = True
            break
        lines.append(r.stdout.rstrip())
        print(r.stdout.rstrip(), flush=True)
        if conditioned:
            ratio = float(r.stdout.split("ciao_gram / (A.T @ A) ")[1].split()[0])
            verdict = f"the condition (d = 1024 fp64: ciao_gram <= torch A.T @ A): ratio {ratio:.3f}: {'met' if ratio <= 1.0 else 'MISSED'}"
    lines.append("# " + verdict)
    if ("--newton" in sys.argv or "--newton-only" in sys.argv) and not failed:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--newton-step"], capture_output=True, text=True, timeout=limit)
            lines.append(r.stdout.rstrip() if r.returncode == 0 else f"newton step: exit status {r.returncode}\n    " + r.stderr.strip().replace("\n", "\n    ")[-2000:])
        except subprocess.TimeoutExpired:
            lines.append(f"newton step: no result within {limit} s")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("# " + verdict)


if __name__ == "__main__":
    main()
