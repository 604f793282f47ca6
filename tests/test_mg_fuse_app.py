"""mpi_jacobi2d --mg --fuse=K on the CPU backend under MPI: the `fuse` report
line and the --json keys, --check against the app's own serial V-cycles with
max|diff| exactly 0 (fusing changes no bit), on 1 rank (every level fused), on 2
ranks of a plain engine (ghost depth 1: the fine level stays unfused) and on 2
ranks with --tblock --tsteps=2 (the fine level fused); --fuse=1 is refused; and
gmt_kernel_bench --only=mg times the fused smoother beside k single sweeps."""
import json
import re

import pytest

from native_util import have_mpi, run_app
from test_mg_app import CHECK_OK

NY, NX = 127, 255
FUSE_LINE = r"fuse      = (\d+) \(fine level (\d+), (\d+) of (\d+) levels fused\)"


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
@pytest.mark.parametrize("np_,dims,extra,tsteps", [(1, (1, 1), [], 1), (2, (1, 2), [], 1),
                                                   (2, (2, 1), ["--tblock", "--tsteps=2"], 2)])
def test_app_mg_fuse(np_, dims, extra, tsteps, tmp_path):
    from gpu_mpi_tests_amd import engine

    depths = engine.mg_fuse_depths(NY, NX, dims, 2, tsteps)
    js = tmp_path / "out.json"
    args = ["mpi_jacobi2d", str(NX), "4", f"--ny={NY}", "--init=random", "--mg", "--check",
            f"--dims={dims[0]}x{dims[1]}", f"--json={js}", *extra]
    p = run_app(*args, "--fuse=2", np=np_)
    out = p.stdout
    m = re.search(FUSE_LINE, out)
    assert m, out
    assert tuple(int(g) for g in m.groups()) == (2, depths[0], sum(d >= 2 for d in depths), len(depths)), (out, depths)
    assert depths[0] == (2 if np_ == 1 or tsteps >= 2 else 1), depths
    assert re.search(CHECK_OK, out), out
    diff = float(re.search(r"max\|diff\| vs serial multigrid = ([0-9.eE+-]+)", out).group(1))
    assert diff == 0.0, out
    j = json.loads(js.read_text().strip().splitlines()[-1])
    assert (j["fuse"], j["fuse_fine"], j["fuse_levels"]) == (2, depths[0], sum(d >= 2 for d in depths)), j
    # without --fuse: no line, the keys say so, the same residual to every printed digit
    q = run_app(*args, np=np_)
    assert not re.search(r"^fuse ", q.stdout, re.M), q.stdout
    j0 = json.loads(js.read_text().strip().splitlines()[-1])
    assert (j0["fuse"], j0["fuse_fine"], j0["fuse_levels"]) == (0, 1, 0), j0
    assert j0["r0"] == j["r0"] and j0["residual_max"] == j["residual_max"] and j0["cycles"] == j["cycles"], (j0, j)


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
def test_app_fuse_refusals():
    for bad in ("--fuse=1", "--fuse=5", "--fuse=-2"):
        p = run_app("mpi_jacobi2d", str(NX), "4", f"--ny={NY}", "--mg", bad, np=1, check=False)
        assert p.returncode != 0 and "--fuse must be 0 or 2..4" in p.stdout + p.stderr and "solver" not in p.stdout


def test_kernel_bench_mg_fused_host():
    """gmt_kernel_bench --only=mg on the CPU backend: a row for k = 2, 3, 4 with and without f, each beside k
    single sweeps and DAXPY, after the bitwise comparison of the two."""
    out = run_app("gmt_kernel_bench", "--only=mg", "--mg-n=63", "--iters=2", "--reps=1").stdout
    for k in (2, 3, 4):
        for nm in (f"mg_smooth_k{k}", f"mg_smooth_k{k}_f"):
            assert re.search(rf"{nm} bitwise {k} x mg_smooth: yes", out), out
            assert re.search(rf"{nm} ms / {k} x mg_smooth ms = [0-9.]+, GB/s / daxpy GB/s = [0-9.]+", out), out
