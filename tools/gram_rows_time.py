#!/usr/bin/env python3
"""Times the Gram statistics over a list of rows (ciao_gram_rows; csrc/gram_kernels.h: gram_partial_kernel<Indexed<...>>) on cuda:0 and
writes profiles/gram_rows_kernel_times.txt (--out: another file).  Follows tools/gram_time.py.

ONE run on one box; every comparison comes from that run.  Each shape is a STEP: a fresh child process (this script with --shape) under
its own time limit (CIAO_STEP_SECONDS, default 420); a step that fails or runs out of time ends the run -- nothing more is started on the
device -- and is recorded as such.  Shapes, at the largest N of CIAO_N (default 10^7, 5 10^6, 2 10^6) that fits:

    d = 1024 fp64, d = 1024 fp32, d = 255 fp64

Per shape, device events on the context's stream after a warm run, the median of CIAO_REPEATS (default 5) repeats, ms:
    ciao_gram                          the whole matrix (before and after the list calls: the same run's drift)
    ciao_gram_rows, identity           idx = 0 .. N-1: the same rows through the list, and its ratio to ciao_gram
    ciao_gram_rows, sorted half        N / 2 rows drawn without repeats, ascending
    ciao_gram_rows, unsorted half      the same rows in the order drawn
    five folds by lists                the five cv.fold_lists lists, five calls: together one pass's worth of rows
    five folds by 0/1 weights          five ciao_gram_weighted calls over all N rows with the same folds as 0/1 weights: what the lists replace

The claim to confirm: the five list calls cost less than the five weighted passes.  How much less is the result, not a condition."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1024, "f64"), (1024, "f32"), (255, "f64")]


def one_shape(d, name):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import ciao_loader
    ciao_loader.load()
    from ciaoalgorithms_jl_amd.cv import fold_lists
    from ciaoalgorithms_jl_amd.device import Context, PackedF
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
    gen = torch.Generator(device="cpu")
    gen.manual_seed(11)
    half = torch.randperm(N, generator=gen)[:N // 2].to(dev)
    half_sorted = torch.sort(half).values.contiguous()
    ident = torch.arange(N, dtype=torch.int64, device=dev)
    folds = fold_lists(N, 5, seed=0, device=dev)
    masks = []
    for r in folds:
        m = torch.zeros(N, dtype=torch.float64, device=dev)
        m[r] = 1.0
        masks.append(m)
    rows_call = lambda r: ctx.gram(F, G, u, cs, bs, rows=r, check_rows=False)
    t_gram = median_ms(lambda: ctx.gram(F, G, u, cs, bs))
    k_gram = ctx.last_kernel()
    whole = [t.clone() for t in (G, u, cs, bs)]
    t_ident = median_ms(lambda: rows_call(ident))
    k_rows = ctx.last_kernel()
    same = all(torch.equal(a.view(torch.int64), e.view(torch.int64)) for a, e in zip((G, u, cs, bs), whole))
    t_sorted = median_ms(lambda: rows_call(half_sorted))
    t_unsorted = median_ms(lambda: rows_call(half))
    t_lists = median_ms(lambda: [rows_call(r) for r in folds])
    t_masks = median_ms(lambda: [ctx.gram(F, G, u, cs, bs3, weights=m) for m in masks])
    k_w = ctx.last_kernel()
    t_gram2 = median_ms(lambda: ctx.gram(F, G, u, cs, bs))
    base = min(t_gram[0], t_gram2[0])
    print(f"{name} d={d} N={N}  ciao_gram {fmt(t_gram)}  again {fmt(t_gram2)}  ciao_gram_rows identity {fmt(t_ident)}  identity / ciao_gram {t_ident[0] / base:.3f}  "
          f"identity list gives ciao_gram's bits: {same}\n"
          f"    sorted random half {fmt(t_sorted)}  unsorted random half {fmt(t_unsorted)}  half / whole: sorted {t_sorted[0] / base:.3f} unsorted {t_unsorted[0] / base:.3f}\n"
          f"    five folds by lists {fmt(t_lists)}  five folds by 0/1 weights {fmt(t_masks)}  lists / weights {t_lists[0] / t_masks[0]:.3f}  lists / one ciao_gram {t_lists[0] / base:.3f}\n"
          f"    [{k_gram}]\n    [{k_rows}]\n    [{k_w}]", flush=True)
    ctx.synchronize()
    ctx.close()


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--shape":
        one_shape(int(sys.argv[2]), sys.argv[3])
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "gram_rows_kernel_times.txt")
    limit = int(os.environ.get("CIAO_STEP_SECONDS", "420"))
    lines = [f"# tools/gram_rows_time.py: median (min .. max) of {os.environ.get('CIAO_REPEATS', '5')} repeats, device events, ms; ONE run, one box"]
    claim = []
    for d, name in SHAPES:
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
        claim.append((name, d, float(r.stdout.split("lists / weights ")[1].split()[0])))
    verdict = "the claim (five list calls cost less than five 0/1-weighted passes): " + (
        ", ".join(f"{n} d={d}: {v:.3f}" for n, d, v in claim) + (": confirmed" if claim and all(v < 1 for _, _, v in claim) else ": NOT confirmed")
        if claim else "not measured")
    lines.append("# " + verdict)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("# " + verdict)


if __name__ == "__main__":
    main()
