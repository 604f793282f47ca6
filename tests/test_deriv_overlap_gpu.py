"""``mpi_stencil2d_gt --overlap`` and ``engine.deriv_step_bench`` on a real
MI355X: oversubscribed ranks sharing the GPU, the halo exchange on a
high-priority stream beside gmt_stencil5_2d_interior, then the band kernels of
gmt_stencil5_2d_edges behind an event (gmt/deriv.hpp).

--check raises the field by 1.0 before every exchange and compares every
overlapped step's derivative with the analytic one: an edges kernel that ran
before its ghost cells arrived, or read cells of an earlier step, is off by
scale / 12 = n_global / 96 per cell; ``step_err`` is held against half of that
over 205 steps per test.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

BIN = os.path.join(ROOT, "build", "bin")
MPIRUN = "/opt/conda/bin/mpirun"
N_LOCAL = 64
ARGS = [str(N_LOCAL), "200", "--no-managed", "--tests=deriv", "--n-other=4096", "--check", "--overlap"]
STEP_RE = (r"^STEP dim:(\d), device , buf:(\d); serial=([0-9.]+), overlap=([0-9.]+), step_err=([0-9.]+) "
           r"\[([\w-]+)\]$")


def _app(args, np_, timeout=120, **env):
    cmd = ["timeout", "-k", "10", str(timeout), MPIRUN, "-np", str(np_), os.path.join(BIN, "mpi_stencil2d_gt"), *args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout + 30, cwd="/tmp",
                          env=dict(os.environ, **env))


@pytest.mark.parametrize("np_", [2, 3])
@pytest.mark.parametrize("transport", ["ipc", "mpi-host"])
def test_app_overlapped_steps(np_, transport):
    p = _app(ARGS + [f"--transport={transport}"], np_)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    out = p.stdout
    steps = re.findall(STEP_RE, out, re.M)
    errs = [float(v) for v in re.findall(r"^TEST .* err=([0-9.]+)", out, re.M)]
    assert len(steps) == 4 and len(errs) == 4, out
    threshold = N_LOCAL * np_ / 192
    for (dim, buf, serial, overlap, step_err, tag), err in zip(steps, errs):
        print(f"np {np_} {transport} dim {dim} buf {buf}: serial {serial} s, overlap {overlap} s, "
              f"step_err {step_err} (threshold {threshold}), err {err}")
        assert tag == transport
        assert float(serial) > 0 and float(overlap) > 0
        assert float(step_err) < threshold, out
        assert err < 1e-5, out
    checks = re.findall(r"# halo check dim:\d buf:\d \(([\w-]+)\): (\d+) bad ghost cells, (\d+) exchanges", out)
    assert len(checks) == 4 and all(t == transport and int(b) == 0 and int(n) == 410 for t, b, n in checks), out


def test_app_overlapped_step_catches_a_stale_ghost_cell():
    """GMT_CORRUPT_GHOST=1:20: one ghost cell of rank 1 goes back to the last
    step's value between finish() and the edges kernel of iteration 20."""
    p = _app(ARGS + ["--transport=ipc", "--dim=0", "--buf=0"], 2, GMT_CORRUPT_GHOST="1:20")
    assert p.returncode == 5, p.stdout[-3000:] + p.stderr[-3000:]
    (step,) = re.findall(STEP_RE, p.stdout, re.M)
    print(f"step_err {step[4]}, threshold {N_LOCAL * 2 / 192}")
    assert float(step[4]) > N_LOCAL * 2 / 192, p.stdout
    assert "# halo check dim:0 buf:0 (ipc): 1 bad ghost cells" in p.stdout, p.stdout


def test_engine_deriv_step_bench_single_rank():
    from gpu_mpi_tests_amd import engine
    from gpu_mpi_tests_amd.parallel import dist as gd

    r = engine.deriv_step_bench(N_LOCAL, 300, n_iter=4, n_warmup=1, env=gd.init(device="cuda"), check=True)
    for d in (0, 1):
        v = r[f"dim{d}"]
        print(f"dim {d}: {v}")
        assert v["serial_median_s"] > 0 and v["overlap_median_s"] > 0
        assert v["err_norm"] < 1e-6  # test_engine_deriv_bench_single_rank's bar, same shape
        assert 0 <= v["step_err_max"] < N_LOCAL / 192
        assert v["bad_ghosts"] == 0
