#!/usr/bin/env python3
"""Times the Gram statistics (csrc/gram_kernels.h) on cuda:0 and writes profiles/gram_kernel_times.txt (--out: another file).

One run on one box; every comparison comes from that run.  Each shape is a STEP: a fresh child process (this script with --shape) under
its own time limit (CIAO_STEP_SECONDS, default 420); a step that fails or runs out of time ends the run -- nothing more is started on the
device -- and is recorded as such.  Shapes, at the largest N of CIAO_N (default 10^7, 5 10^6, 2 10^6) that fits:

    d = 1024 fp64 (the condition), d = 1024 fp32, d = 4096 fp32, d = 50 fp64, d = 255 fp64

Per shape, device events after a warm run, the median of CIAO_REPEATS (default 5) repeats, ms:
    ciao_gram                  G, u, colsum, bsum in one call (gram_partial_kernel + gram_final_kernel)
    torch A.T @ A              in A's dtype: what there was before the kernel, for G alone
    torch A.T @ b + sums       A.T @ b, A.sum(0), b.sum(), (b * b).sum(): the further passes that route needs
    ciao_full_gradient         one pass over the same rows (the HBM yardstick)
    stepsize.smoothness        what smoothness_exact replaces (wall clock: it synchronises)
    fraction of the fp64 MFMA peak: N d (d + 1) flops (the upper triangle, which is all the kernel owes) / time / 78.6 TFLOP/s

The one condition: at d = 1024 fp64 ciao_gram takes no longer than torch's A.T @ A alone."""
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
    u, cs, bs = (torch.empty(n, dtype=torch.float64, device=dev) for n in (d, d, 2))
    t_gram = median_ms(lambda: ctx.gram(F, G, u, cs, bs))
    k_gram = ctx.last_kernel()
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
    print(f"{name} d={d} N={N}  ciao_gram {fmt(t_gram)}  torch A.T @ A {fmt(t_ata)}  torch A.T @ b + sums {fmt(t_atb)}  "
          f"ciao_full_gradient {fmt(t_pass)}  stepsize.smoothness {t_smooth:.1f}  "
          f"ciao_gram / (A.T @ A) {t_gram[0] / t_ata[0]:.3f}  fraction of the fp64 MFMA peak {frac:.3f}  max |A.T @ A - G| / max |G| {rel:.1e}\n"
          f"    [{k_gram}]", flush=True)
    ctx.synchronize()
    ctx.close()


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--shape":
        one_shape(int(sys.argv[2]), sys.argv[3])
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "gram_kernel_times.txt")
    limit = int(os.environ.get("CIAO_STEP_SECONDS", "420"))
    lines = [f"# tools/gram_time.py: median (min .. max) of {os.environ.get('CIAO_REPEATS', '5')} repeats, device events, ms; one run, one box"]
    verdict = "the condition (d = 1024 fp64: ciao_gram <= torch A.T @ A): not measured"
    for d, name, conditioned in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(d), name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name} d={d}: no result within {limit} s; the run ends here")
            break
        if r.returncode != 0:
            lines.append(f"{name} d={d}: exit status {r.returncode}; the run ends here\n    " + r.stderr.strip().replace("\n", "\n    ")[-2000:])
            break
        lines.append(r.stdout.rstrip())
        print(r.stdout.rstrip(), flush=True)
        if conditioned:
            ratio = float(r.stdout.split("ciao_gram / (A.T @ A) ")[1].split()[0])
            verdict = f"the condition (d = 1024 fp64: ciao_gram <= torch A.T @ A): ratio {ratio:.3f}: {'met' if ratio <= 1.0 else 'MISSED'}"
    lines.append("# " + verdict)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("# " + verdict)


if __name__ == "__main__":
    main()
