"""mpi_jacobi2d --mg --fuse-resid on the CPU backend under MPI: the `resid`
report line and the --json keys, --check against the app's own serial V-cycles
with max|diff| exactly 0 (fusing changes no bit), on 1 rank, on 2 ranks of a
plain engine (ghost depth 1: the fine level stays unfused) and on 2 ranks with
--tblock --tsteps=2 (the fine level fused); and gmt_kernel_bench --only=mg times
the fused transfer beside the two kernels."""
import json
import re

import pytest

from native_util import have_mpi, run_app
from test_mg_app import CHECK_OK

NY, NX = 127, 255
RESID_LINE = r"resid     = fused \((\d+) of (\d+) levels\)"


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
@pytest.mark.parametrize("np_,dims,extra,tsteps", [(1, (1, 1), [], 1), (2, (1, 2), ["--fuse=2"], 1),
                                                   (2, (2, 1), ["--tblock", "--tsteps=2", "--smoother=rb"], 2)])
def test_app_mg_fuse_resid(np_, dims, extra, tsteps, tmp_path):
    from gpu_mpi_tests_amd import engine

    levels = engine.mg_resid_levels(NY, NX, dims, tsteps)
    nlev = len(engine.mg_levels(NY, NX, dims))
    js = tmp_path / "out.json"
    args = ["mpi_jacobi2d", str(NX), "4", f"--ny={NY}", "--init=random", "--mg", "--check",
            f"--dims={dims[0]}x{dims[1]}", f"--json={js}", *extra]
    p = run_app(*args, "--fuse-resid", np=np_)
    out = p.stdout
    m = re.search(RESID_LINE, out)
    assert m, out
    assert tuple(int(g) for g in m.groups()) == (len(levels), nlev - 1), (out, levels)
    assert (0 in levels) == (np_ == 1 or tsteps >= 2), levels
    assert re.search(CHECK_OK, out), out
    diff = float(re.search(r"max\|diff\| vs serial multigrid = ([0-9.eE+-]+)", out).group(1))
    assert diff == 0.0, out
    j = json.loads(js.read_text().strip().splitlines()[-1])
    assert (j["fuse_resid"], j["resid_levels"], j["resid_mask"]) == (True, len(levels), sum(1 << l for l in levels)), j
    # without --fuse-resid: no line, the keys say so, the same residual to every printed digit
    q = run_app(*args, np=np_)
    assert not re.search(r"^resid ", q.stdout, re.M), q.stdout
    j0 = json.loads(js.read_text().strip().splitlines()[-1])
    assert (j0["fuse_resid"], j0["resid_levels"], j0["resid_mask"]) == (False, 0, 0), j0
    assert j0["r0"] == j["r0"] and j0["residual_max"] == j["residual_max"] and j0["cycles"] == j["cycles"], (j0, j)


def test_kernel_bench_mg_resid_host():
    """gmt_kernel_bench --only=mg on the CPU backend: a row for the fused transfer with and without f, each beside
    gmt_cg_apply mode 1 + gmt_mg_restrict, after the bitwise comparison of the two."""
    out = run_app("gmt_kernel_bench", "--only=mg", "--mg-n=63", "--iters=2", "--reps=1").stdout
    for nm in ("mg_resid_restrict", "mg_resid_restrict_f"):
        assert re.search(rf"{nm} bitwise cg_apply \+ mg_restrict: yes", out), out
        assert re.search(rf"{nm} ms / \(cg_apply \+ mg_restrict\) ms = [0-9.]+, bytes model [0-9/]+", out), out
