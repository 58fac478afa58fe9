"""bench.py's options: a plain run times the sweep and nothing else (the secondary figures need --full), --steps is the number of
timed steps, and --dump-outputs writes the last timed step's outputs, the same from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL_ONLY = ("cpu_baseline", "svrg_updates_per_sec", "saga_updates_per_sec", "finito_samples_per_sec", "full_pass_K_solves",
             "extras_file", "chain_figures_error")


def test_options():
    import bench
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out", "--steps", "7"])
    assert a.full is True and a.dump_outputs == "out" and a.steps == 7
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_plain_run_dumps_the_last_steps_outputs(tmp_path, dtype):
    """Two runs with the same arguments dump the same outputs, and those are the LAST step's: a run one step shorter ends at the
    iterate the last step started from, and the dumped x is the prox step from it with the dumped av (x+ = prox(x - gamma av))."""
    N, steps, warmup = 200_000, 5, 2
    base = ["--gpus", "1", "--warmup", str(warmup), "--rows-per-gpu", str(N), "--dtype", dtype]
    outs = []
    for k, n_steps in enumerate((steps, steps, steps - 1)):
        j = _bench(base + ["--steps", str(n_steps), "--dump-outputs", str(tmp_path / f"run{k}")])
        assert j["steps"] == n_steps and j["warmup"] == warmup and j["dtype"] == dtype and j["unit"] == "updates/s"
        assert j["value"] > 0 and j["ms_per_step"] > 0 and j["higher_is_better"] is True
        assert j["roofline"]["kernel_launches"] == n_steps, "the timed region is exactly --steps sweeps"
        assert not [key for key in FULL_ONLY if key in j], "a plain run measures the sweep only"
        got = {n: np.load(tmp_path / f"run{k}" / f"{n}.npy") for n in ("x", "av")}
        for v in got.values():
            assert v.shape == (1024,) and v.dtype == (np.float64 if dtype == "f64" else np.float32) and np.isfinite(v).all()
        assert np.abs(got["x"]).max() > 0 and np.abs(got["av"]).max() > 0
        outs.append(got)
    tol = 1e-12 if dtype == "f64" else 1e-5
    for n in ("x", "av"):
        np.testing.assert_allclose(outs[1][n], outs[0][n], rtol=tol, atol=tol * np.abs(outs[0][n]).max())

    # the bench's Lasso: gamma = 1 / (7 * 1.3 N), NormL1(1e-3); the line states both (gamma to 6 digits)
    gamma, lam = 1.0 / (7.0 * 1.3 * N), 1e-3
    assert j["config"]["gamma"] == pytest.approx(gamma, rel=1e-5) and j["config"]["g"] == "NormL1(0.001)"
    x_prev, x_last, av = (outs[2]["x"].astype(np.float64), outs[0]["x"].astype(np.float64), outs[0]["av"].astype(np.float64))
    v = x_prev - gamma * av
    want = np.sign(v) * np.maximum(np.abs(v) - gamma * lam, 0.0)
    unit = 8 * np.finfo(np.float64 if dtype == "f64" else np.float32).eps * max(np.abs(x_prev).max(), np.abs(gamma * av).max())
    assert np.abs(x_last - want).max() <= unit, "x.npy is the prox step of the last timed step from its start with av.npy"
    assert np.abs(x_last - x_prev).max() > 100 * unit, "the check tells the last iterate from the one before it"
