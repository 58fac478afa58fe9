#!/usr/bin/env python3
"""retune_scales.py PARITY_OBSERVED.json [--write] -- set every `scale=` of tests/test_gpu_parity.py and tests/test_gpu_complex.py from what a GPU run
observed: scale = 10 x (largest error in eps units seen at that call site, per dtype, over all parametrisations), rounded up to two
significant digits, floor 8; one number when both dtypes agree, else {64: a, 32: b}; `scale64=` (Float32 against the Float64 oracle
on the same data) likewise, never above BASELINE's 840 eps32.  The log comes from a run of the same file (line numbers must match):
CIAO_PARITY_CALIBRATE=1 python -m pytest tests/test_gpu_parity.py -m gpu   ->  gpurun_out/parity_observed.json."""
import json
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("test_gpu_parity.py", "test_gpu_complex.py", "test_gpu_wide_chain.py", "test_gpu_long_rows.py", "test_gpu_small_mfma.py",
         "test_gpu_feature_padding.py", "test_gpu_multi_rhs.py", "test_gpu_every_kernel.py", "test_gpu_layouts.py")


def nice(x):
    """x rounded DOWN to two significant digits, floor 8: the allowed scale never exceeds 10 x the observed error (and is at least 9 x it)"""
    x = max(x, 8.0)
    e = math.floor(math.log10(x)) - 1
    m = math.floor(x / 10 ** e + 1e-9)
    v = m * 10 ** e
    return int(v) if v == int(v) else v


def retune(fname, log, write):
    """per call site and type: scale = 10 x the largest error seen; `scale=` becomes a number when only one type is seen at the site
    or both get the same value, else {64: a, 32: b}; `scale64=` (form (i): Float32 against the Float64 oracle) likewise, capped at
    BASELINE's 840 eps32 (a site that would need more FAILS the retune: the tolerance is the contract)"""
    path = os.path.join(ROOT, "tests", fname)
    worst, worst64 = {}, {}
    for r in log:
        if r["line"] <= 0 or r.get("file") != fname:   # (records without a file are hand-written ones: tests/test_gpu_configs.py)
            continue
        bits = 64 if r["dtype"] == "float64" else 32
        tgt = worst64 if r.get("form") == "f64 oracle" else worst
        d = tgt.setdefault(r["line"], {})
        d[bits] = max(d.get(bits, 0.0), r["ratio"])
    lines = open(path).read().split("\n")
    changed, rc = 0, 0
    for ln in sorted(set(worst) | set(worst64)):
        src = lines[ln - 1]
        if "close(" not in src:
            print(f"{fname} line {ln}: no close( call there -- the log does not belong to this file", file=sys.stderr)
            return 1
        out = src
        if ln in worst:
            vals = {b: nice(10.0 * v) for b, v in worst[ln].items()}
            # (a site seen in one type only gets a one-key dict: the other type there would be a KeyError, not an unmeasured bound)
            new = str(next(iter(vals.values()))) if len(vals) == 2 and len(set(vals.values())) == 1 else \
                "{" + ", ".join(f"{b}: {vals[b]}" for b in sorted(vals, reverse=True)) + "}"
            if re.search(r"scale=(\{[^}]*\}|[^,)]+)", out):
                out = re.sub(r"scale=(\{[^}]*\}|[^,)]+)", f"scale={new}", out, count=1)
            elif ", what=" in out:
                out = out.replace(", what=", f", scale={new}, what=", 1)
            else:
                out = re.sub(r"\)\s*$", f", scale={new})", out, count=1)
        if ln in worst64:
            v = nice(10.0 * worst64[ln][32])
            if worst64[ln][32] > 840.0:
                print(f"{fname}:{ln}: Float32 against the Float64 oracle observed {worst64[ln][32]:.0f} eps32 > 840 (1e-4): OUTSIDE BASELINE", file=sys.stderr)
                rc = 1
            v = min(v, 840)
            if re.search(r"scale64=[^,)]+", out):
                out = re.sub(r"scale64=[^,)]+", f"scale64={v}", out, count=1)
            else:
                code, sep, comment = re.match(r"^(.*?\))(\s{2,}#.*)?()$", out).group(1, 2, 3) if re.match(r"^(.*?\))(\s{2,}#.*)?()$", out) else (out, None, "")
                out = re.sub(r"\)\s*$", f", scale64={v})", code, count=1) + (sep or "")
        if out != src:
            changed += 1
            lines[ln - 1] = out
        print(f"{fname}:{ln:5d}  observed {worst.get(ln)} / f64-oracle {worst64.get(ln)}  ->  {out.strip()[:110]}")
    if write:
        open(path, "w").write("\n".join(lines))
        print(f"{fname}: {changed} call sites rewritten")
    return rc


def main():
    log = json.load(open(sys.argv[1]))
    rc = 0
    for f in FILES:
        rc |= retune(f, log, "--write" in sys.argv)
    return rc


if __name__ == "__main__":
    sys.exit(main())
