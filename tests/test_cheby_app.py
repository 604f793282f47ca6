"""mpi_jacobi2d --cheby and gmt_kernel_bench --only=cheby: the report lines, the
--json keys, --check against the app's own serial Chebyshev iterations (within
1e-10 * max|u0|, the bound of --cg --check) on 1, 2 and 4 ranks of the CPU
backend and on one rank of the GPU, exit status 4 at an unreachable tolerance,
and the refusals (--periodic, --cg, a bad --rho)."""
import json
import os
import re
import subprocess

import pytest

from cheby_worker import pick_rtol
from native_util import ROOT, have_mpi, run_app

KEYS = ("solver", "rho", "iters", "residual_iters", "checks", "converged", "solve_ms", "r0", "residual_max")
CHECK_OK = r"check\s*: max\|diff\| vs serial chebyshev = [0-9.eE+-]+ \(bound [0-9.eE+-]+\) OK"


def _reference_pick():
    from gpu_mpi_tests_amd import engine

    rho = engine.cheby_rho(60, 64)
    _, ser = engine.serial_cheby(60, 64, 120, rho, init="random", seed=0, resid_every=10)
    return rho, ser, pick_rtol(ser, 10, 4)


def _check_report(out, j, rho, ser, c):
    assert "solver    = chebyshev" in out and "converged : yes" in out, out
    shown = float(re.search(r"rho       = ([0-9.e+-]+)", out).group(1))
    assert abs(shown - rho) <= 1e-15 * rho, (shown, rho)
    m = re.search(r"iters     : (\d+) \(criterion met at (\d+), (\d+) checks, lag 1\)", out)
    assert m, out
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == ((c + 1) * 10, c * 10, c + 2), (out, c)
    assert re.search(r"TIME solve: [0-9.]+ ms", out) and re.search(r"TIME iter : [0-9.]+ ms per iteration", out), out
    res = float(re.search(r"residual  : ([0-9.e+-]+)", out).group(1))
    assert abs(res - ser[c * 10][0]) <= 1e-9 * ser[c * 10][0], (res, ser[c * 10])  # ten printed digits
    assert "true resid" not in out and re.search(CHECK_OK, out), out
    for k in KEYS:
        assert k in j, j
    assert j["solver"] == "chebyshev" and j["converged"] is True and j["iters"] == (c + 1) * 10, j
    assert j["residual_iters"] == c * 10 and j["checks"] == c + 2 and abs(j["rho"] - rho) <= 1e-8, j
    assert abs(j["r0"] - ser[0][0]) <= 1e-8 * ser[0][0], (j, ser[0])  # nine digits in the record


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
@pytest.mark.parametrize("np_", [1, 2, 4])
def test_app_cheby(np_, tmp_path):
    """mpi_jacobi2d 64 400 --ny=60 --init=random --cheby --rtol=R --check --json on the CPU backend."""
    rho, ser, (c, rtol) = _reference_pick()
    js = tmp_path / "out.json"
    p = run_app("mpi_jacobi2d", "64", "400", "--ny=60", "--init=random", "--cheby", f"--rtol={rtol!r}", "--check",
                f"--json={js}", np=np_)
    _check_report(p.stdout, json.loads(js.read_text().strip().splitlines()[-1]), rho, ser, c)


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
def test_app_cheby_cap_fixed_count_rho_and_refusals():
    """An unreachable --tol exits 4 at the (rounded-up) cap; --cheby alone runs n_iter iterations; --rho is
    reported as given; --source goes through --check; --periodic, --cg and a bad --rho are refused."""
    p = run_app("mpi_jacobi2d", "64", "25", "--ny=60", "--init=random", "--cheby", "--tol=1e-300", "--lag=2", np=2,
                check=False)
    assert p.returncode == 4, p.stdout + p.stderr
    assert "converged : no" in p.stdout and "rounded up to a multiple of 10" in p.stdout, p.stdout
    assert re.search(r"iters     : 30 \(criterion met at 30, 4 checks, lag 2\)", p.stdout), p.stdout
    f = run_app("mpi_jacobi2d", "64", "40", "--ny=60", "--init=random", "--cheby", "--rho=0.9375", "--check",
                "--source=random", np=2)
    assert "solver    = chebyshev" in f.stdout and re.search(r"iters     : 40 \(fixed count", f.stdout), f.stdout
    assert re.search(r"rho       = 0\.9375\n", f.stdout) and re.search(CHECK_OK, f.stdout), f.stdout
    for extra, word in ((["--periodic"], "periodic"), (["--cg"], "exclusive"), (["--rho=1.0"], "rho"),
                        (["--rho=-0.1"], "rho")):
        bad = run_app("mpi_jacobi2d", "64", "30", "--ny=60", "--cheby", *extra, np=1, check=False)
        assert bad.returncode != 0 and word in (bad.stdout + bad.stderr), (extra, bad.stdout + bad.stderr)
        assert "solver" not in bad.stdout, bad.stdout


def test_kernel_bench_cheby_host():
    """gmt_kernel_bench --only=cheby on the CPU backend: one line per variant, each beside its DAXPY."""
    out = run_app("gmt_kernel_bench", "--only=cheby", "--cheby-n=64", "--iters=2", "--reps=1").stdout
    for k in ("cheby_step", "cheby_step_f"):
        assert len(re.findall(rf"^{k}\s+v0\s+64x64 best", out, re.M)) == 1, out
        assert re.search(rf"{k} GB/s / daxpy GB/s = [0-9.]+", out), out
    assert len(re.findall(r"^daxpy\s+v[12]", out, re.M)) == 2, out


@pytest.mark.gpu
def test_app_cheby_gpu(tmp_path):
    """One rank on the GPU: the same report, --check against the host's serial iterations."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = os.path.join(ROOT, "build", "bin", "mpi_jacobi2d")
    assert os.path.exists(exe), f"{exe} not built"
    rho, ser, (c, rtol) = _reference_pick()
    js = tmp_path / "out.json"
    p = subprocess.run(["timeout", "-k", "10", "100", exe, "64", "400", "--ny=60", "--init=random", "--cheby",
                        f"--rtol={rtol!r}", "--check", f"--json={js}"], capture_output=True, text=True, timeout=120,
                       cwd="/tmp")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "backend=hip" in p.stdout, p.stdout
    _check_report(p.stdout, json.loads(js.read_text().strip().splitlines()[-1]), rho, ser, c)
