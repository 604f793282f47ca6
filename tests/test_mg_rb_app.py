"""mpi_jacobi2d --mg --smoother=rb on the CPU backend under MPI: the `smoother`
report line after `solver`, the --json key, --check against the app's own serial
V-cycles with red-black sweeps (max|diff| exactly 0) on 1 and 4 ranks, unfused
and with --fuse; --smoother without --mg and an unknown smoother are refused;
without --smoother the output has no `smoother` line; and gmt_kernel_bench
--only=mg times gmt_mg_smooth_rb beside gmt_mg_smooth_k."""
import json
import re

import pytest

from native_util import have_mpi, run_app
from test_mg_app import CHECK_OK

NY, NX = 127, 255
SMOOTHER_LINE = r"^solver    = multigrid\nsmoother  = rb \(omega ([0-9.]+)\)$"


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
@pytest.mark.parametrize("np_,dims,extra", [(1, (1, 1), []), (1, (1, 1), ["--fuse=4", "--nu=2,1"]), (4, (2, 2), []),
                                            (4, (2, 2), ["--fuse=3", "--tblock", "--tsteps=4", "--omega=0.8"])])
def test_app_mg_rb(np_, dims, extra, tmp_path):
    js = tmp_path / "out.json"
    args = ["mpi_jacobi2d", str(NX), "4", f"--ny={NY}", "--init=random", "--mg", "--check",
            f"--dims={dims[0]}x{dims[1]}", f"--json={js}", *extra]
    p = run_app(*args, "--smoother=rb", np=np_)
    out = p.stdout
    m = re.search(SMOOTHER_LINE, out, re.M)
    assert m, out
    assert float(m.group(1)) == (0.8 if "--omega=0.8" in extra else 1.0), out
    assert re.search(CHECK_OK, out), out
    diff = float(re.search(r"max\|diff\| vs serial multigrid = ([0-9.eE+-]+)", out).group(1))
    assert diff == 0.0, out
    j = json.loads(js.read_text().strip().splitlines()[-1])
    assert j["smoother"] == "rb" and j["solver"] == "multigrid", j
    # without --smoother: no line, the key says jacobi, another residual
    q = run_app(*args, np=np_)
    assert not re.search(r"^smoother ", q.stdout, re.M), q.stdout
    assert re.search(CHECK_OK, q.stdout), q.stdout
    j0 = json.loads(js.read_text().strip().splitlines()[-1])
    assert j0["smoother"] == "jacobi" and j0["residual_max"] != j["residual_max"], (j0, j)
    # --smoother=jacobi is the default, to every printed digit
    r = run_app(*args, "--smoother=jacobi", np=np_)
    assert not re.search(r"^smoother ", r.stdout, re.M), r.stdout
    j1 = json.loads(js.read_text().strip().splitlines()[-1])
    assert j1["smoother"] == "jacobi" and j1["residual_max"] == j0["residual_max"] and j1["r0"] == j0["r0"], (j0, j1)


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
def test_app_smoother_refusals():
    p = run_app("mpi_jacobi2d", str(NX), "4", f"--ny={NY}", "--smoother=rb", np=1, check=False)
    assert p.returncode != 0 and "--smoother needs --mg" in p.stdout + p.stderr and "solver" not in p.stdout
    p = run_app("mpi_jacobi2d", str(NX), "4", f"--ny={NY}", "--cg", "--smoother=rb", np=1, check=False)
    assert p.returncode != 0 and "--smoother needs --mg" in p.stdout + p.stderr and "solver" not in p.stdout
    for bad in ("--smoother=x", "--smoother=gs", "--smoother=1"):
        p = run_app("mpi_jacobi2d", str(NX), "4", f"--ny={NY}", "--mg", bad, np=1, check=False)
        assert p.returncode != 0 and "--smoother must be jacobi or rb" in p.stdout + p.stderr and "solver" not in p.stdout


def test_kernel_bench_mg_rb_host():
    """gmt_kernel_bench --only=mg on the CPU backend: a row for h = 1, 2, 4 with and without f, each beside
    gmt_mg_smooth_k of k = h, after the bitwise comparison with h launches of h = 1."""
    out = run_app("gmt_kernel_bench", "--only=mg", "--mg-n=63", "--iters=2", "--reps=1").stdout
    for h in (1, 2, 4):
        for f in ("", "_f"):
            assert re.search(rf"mg_smooth_rb{h}{f} bitwise {h} x mg_smooth_rb1: yes", out), out
            assert re.search(rf"mg_smooth_rb{h}{f} ms / mg_smooth_k{h}{f} ms = [0-9.]+", out), out
