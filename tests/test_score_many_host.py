"""The K-model scores without a GPU: the numpy twin of ciao_margin_stats_multi against hand-computed values, scoring.best, the
entry point's signature in header, binding, Julia module and INTEGRATION.md, and its refusal of a NULL context before any launch."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_numpy_twin_against_hand_computed_values(ciao):
    import ciaoalgorithms_jl_amd.host_route as HR
    A = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, -1.0], [2.0, 2.0, 0.0], [-1.0, 0.0, 0.0]])
    xs = [np.array([1.0, -1.0, 0.0]), np.array([0.0, 0.0, 0.5])]         # dots: (1, -1, 0, -1) and (1, -0.5, 0, 0)
    b = np.array([1.0, 1.0, -2.0, 0.5])
    ls = HR.host_margin_stats_multi("ls", A, xs, b)
    # r = (0, -2, 2, -1.5): sum r^2 = 10.25;  r = (0, -1.5, 2, -0.5): sum r^2 = 6.5;  sum b = 0.5, sum b^2 = 6.25
    assert ls == [(10.25, 0.5, 6.25, 2.0), (6.5, 0.5, 6.25, 2.0)]
    y = np.array([1.0, -1.0, 1.0, -1.0])
    lg = HR.host_margin_stats_multi("logistic", A, xs, y, s=[1.0, 0.0])
    # model 0: t = (1, 1, 0, 1): three softplus(-1) and one log 2; E(1) = sum h(sigma(-t)); one t <= 0; min t = 0
    sp1 = math.log1p(math.exp(-1.0))
    h = lambda u: u * math.log(u) + (1 - u) * math.log(1 - u)
    sg = math.exp(-1.0) / (1 + math.exp(-1.0))
    assert lg[0][0] == pytest.approx(3 * sp1 + math.log(2), rel=1e-15) and lg[0][2:] == (1.0, 0.0)
    assert lg[0][1] == pytest.approx(3 * h(sg) + h(0.5), rel=1e-14)
    # model 1: t = (1, 0.5, 0, 0) at s = 0: no entropy; two t <= 0
    assert lg[1][0] == pytest.approx(sp1 + math.log1p(math.exp(-0.5)) + 2 * math.log(2), rel=1e-15)
    assert lg[1][1:] == (0.0, 2.0, 0.0)
    # K calls of the single twin, s = None is s = 1
    assert HR.host_margin_stats_multi("logistic", A, xs, y) == [HR.host_margin_stats("logistic", A @ x, y, 1.0) for x in xs]


def test_best(ciao):
    from ciaoalgorithms_jl_amd.scoring import LeastSquaresScore, LogisticScore, best
    nan = math.nan
    assert best([LogisticScore(nan, 1.0, 1.0), LogisticScore(0.5, 0.9, 0.1), LogisticScore(0.25, 0.8, 0.1), LogisticScore(0.25, 1.0, 2.0)]) == 2
    assert best([LeastSquaresScore(2.0, 0.1, 1.0), LeastSquaresScore(nan, nan, nan), LeastSquaresScore(2.0, 0.9, 0.5)]) == 0
    assert best([LeastSquaresScore(3.0, 0.1, 1.0)]) == 0
    for empty in ([], [LogisticScore(nan, 1.0, 1.0)]):
        with pytest.raises(ValueError):
            best(empty)


def test_signature_everywhere_and_null_context_refused(ciao):
    L = ciao._lib
    name = "ciao_margin_stats_multi"
    assert L.SIGNATURES[name] == (C.c_int32, [C.c_void_p, C.POINTER(L.Problem), C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)])
    hdr = open(os.path.join(ROOT, "include", "ciao_hip.h")).read()
    m = re.search(r"CIAO_API int32_t " + name + r"\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 6
    assert int(re.search(r"#define CIAO_ABI_VERSION (\d+)", hdr).group(1)) == 3 == L.ABI_VERSION      # additive: the version stays
    jl = open(os.path.join(ROOT, "ciaoalgorithms.jl_amd", "julia", "CIAOAlgorithmsAMD", "src", "CIAOAlgorithmsAMD.jl")).read()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"ccall((:{name}, libciao)" in jl and "function score_many(" in jl and f":{name}" in md
    lib = L.load()
    assert hasattr(lib, name)
    out = (C.c_double * 4)()
    tab = (C.c_void_p * 1)(None)
    assert lib.ciao_margin_stats_multi(None, None, 1, tab, None, out) == L.ERR_ARG      # before any launch: an argument error, not a crash
    assert b"NULL" in lib.ciao_last_error()
    from ciaoalgorithms_jl_amd import certificate, device, scoring
    assert callable(scoring.score_many) and callable(device.Context.margin_stats_multi) and callable(certificate.gaps_together)
    solvers = open(os.path.join(ROOT, "ciaoalgorithms.jl_amd", "solvers.py")).read()
    assert "margin_stats_multi" not in solvers and "score_many" not in solvers and "gaps_together" not in solvers
