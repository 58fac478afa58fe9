"""ciaoalgorithms.jl_amd -- MI355X-native finite-sum inner loops (SVRG / SAGA+SAG / Finito / LFinito) behind the
CIAOAlgorithms.jl solver API.

The directory name contains a dot, so it is loaded under the importable alias `ciaoalgorithms_jl_amd`
(see /ciao_loader.py).  Layout:
    csrc/            HIP kernels (gfx950) + the extern "C" ABI  -> libciao_hip.so (declared in /include/ciao_hip.h)
    _lib.py          ctypes binding of that ABI (what a Julia `ccall` would bind)
    device.py        Context / PackedF / ProxG: torch device tensors -> ABI calls
    operators.py     ProximalOperators-style descriptions of f_i and g, and their packing
    sampling.py      injected index streams (the reference's RNG draws are an explicit input here)
    solvers.py       SVRG / SAGA / SAG / Finito constructors, functors, iterator(), solution()
    parallel.py      row sharding + torch.distributed (RCCL) all-reduce hook
    gram.py          Gram statistics (plain and with a weight per row) and what follows from them in d-space: GramLasso, lasso_path, lasso_cd (coordinate descent: ciao_gram_cd; with bounds, penalty factors, a ridge: ciao_gram_cd_general)
    cv.py            K-fold cross-validation of the lasso path in d-space: the folds' Gram statistics from passes over row lists (ciao_gram_rows)
                     and of the l1-logistic path (logistic_cv): every fold a problem on a row list (ciao_list_dots, ciao_list_combine)
    newton.py        a proximal Newton path for l1-logistic rows on the weighted Gram pass (DeviceRows / HostRows)
    julia/           the Julia wrapper module (written against the same ABI; cannot run in this image)
Importing this package does not need a GPU; creating a Context does.  There is no CPU fallback.
"""
from . import _lib
from .sampling import FixedStream, IndexStream

__all__ = ["_lib", "IndexStream", "FixedStream"]
# the coordinate-descent route of the d-space lasso (DESIGN.md sections 8.14 and 8.17), by name from the package
_ELSEWHERE = {"lasso_cd": "gram", "host_gram_cd": "host_route", "constrained_gaps": "gram", "host_gram_cd_general": "host_route"}


def __getattr__(name):
    # torch-dependent modules are imported lazily so that `import ciaoalgorithms_jl_amd` stays cheap
    import importlib
    for mod in ("solvers", "operators", "device", "parallel"):
        m = importlib.import_module(f"{__name__}.{mod}")
        if hasattr(m, name):
            return getattr(m, name)
        if name == mod:
            return m
    if name in _ELSEWHERE:
        return getattr(importlib.import_module(f"{__name__}.{_ELSEWHERE[name]}"), name)
    raise AttributeError(name)
