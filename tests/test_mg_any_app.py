"""mpi_jacobi2d --mg --coarsen=any and gmt_kernel_bench --only=mg with an even
size, on the CPU backend: at 256 x 766 (y general once, x general on every
level) --check passes against the app's own serial V-cycles with the
table-driven transfers (bound 1e-10 * max|u0|) on 1 and 4 ranks, the report
has the `coarsen` and `levels` lines, --json carries `coarsen`, the cycle
counts are engine.serial_mg(coarsen="any")'s; without --coarsen the same size
is refused with the nested text; a bad --coarsen is refused."""
import json
import re

import pytest

from native_util import have_mpi, run_app
from test_mg_app import CHECK_OK

NY, NX, RTOL = 256, 766, 1e-6


def _reference(dims):
    from gpu_mpi_tests_amd import engine

    levels = engine.mg_levels(NY, NX, dims, coarsen="any")
    _, ser = engine.serial_mg(NY, NX, 12, init="random", seed=0, max_levels=len(levels), coarsen="any")
    thr = RTOL * ser[0][0]
    c = next(i for i, (r, _) in enumerate(ser) if r <= thr)
    assert 1 <= c <= 10 and all(abs(r - thr) > 0.01 * thr for r, _ in ser), (thr, ser)
    return levels, ser, c


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
@pytest.mark.parametrize("np_,dims", [(1, (1, 1)), (4, (2, 2))])
def test_app_mg_any(np_, dims, tmp_path):
    from gpu_mpi_tests_amd import engine

    levels, ser, c = _reference(dims)
    js = tmp_path / "out.json"
    p = run_app("mpi_jacobi2d", str(NX), "12", f"--ny={NY}", "--init=random", "--mg", "--coarsen=any",
                f"--rtol={RTOL!r}", "--check", f"--dims={dims[0]}x{dims[1]}", f"--json={js}", np=np_)
    out = p.stdout
    assert "solver    = multigrid" in out and "coarsen   = any" in out and "converged : yes" in out, out
    rho = engine.cheby_rho(*levels[-1])
    m = re.search(r"levels    = (\d+) \(coarsest (\d+) x (\d+), (\d+) iterations, rho ([0-9.e+-]+)\)", out)
    assert m, out
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (len(levels), *levels[-1]), (out, levels)
    assert int(m.group(4)) == engine.mg_coarse_iters(rho), (out, rho)
    m = re.search(r"cycles    : (\d+) \(criterion met at (\d+), (\d+) checks, lag 1\)", out)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (c + 1, c, c + 2), (out, c)
    res = float(re.search(r"residual  : ([0-9.e+-]+)", out).group(1))
    assert abs(res - ser[c][0]) <= 1e-9 * ser[c][0], (res, ser[c])  # ten printed digits
    assert re.search(CHECK_OK, out), out
    j = json.loads(js.read_text().strip().splitlines()[-1])
    assert j["solver"] == "multigrid" and j["coarsen"] == "any" and j["levels"] == len(levels), j
    assert j["converged"] is True and j["cycles"] == c + 1 and j["residual_cycles"] == c, j


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
def test_app_coarsen_default_and_refusals(tmp_path):
    """Without --coarsen the size is refused as before (the text may now name the way out); --coarsen=nested is
    the default; a bad value is refused; a nested size reports `coarsen = nested` and carries it in --json."""
    for extra in ([], ["--coarsen=nested"]):
        bad = run_app("mpi_jacobi2d", str(NX), "5", f"--ny={NY}", "--mg", *extra, np=1, check=False)
        text = bad.stdout + bad.stderr
        assert bad.returncode != 0 and "solver" not in bad.stdout, text
        assert f"--mg has no coarse level for {NY} x {NX}: nx + 1 and ny + 1 must be even (8191 and 32767 coarsen, " \
               "8192 does not)" in text and "--coarsen=any" in text, text
    bad = run_app("mpi_jacobi2d", str(NX), "5", f"--ny={NY}", "--mg", "--coarsen=all", np=1, check=False)
    assert bad.returncode != 0 and "--coarsen" in bad.stdout + bad.stderr and "solver" not in bad.stdout
    bad = run_app("mpi_jacobi2d", "2", "5", "--ny=2", "--mg", "--coarsen=any", np=1, check=False)
    assert bad.returncode != 0 and "no coarse level" in bad.stdout + bad.stderr, bad.stdout + bad.stderr
    js = tmp_path / "out.json"
    ok = run_app("mpi_jacobi2d", "127", "3", "--ny=63", "--init=random", "--mg", "--check", f"--json={js}", np=1)
    assert "coarsen   = nested" in ok.stdout and re.search(CHECK_OK, ok.stdout), ok.stdout
    assert json.loads(js.read_text().strip().splitlines()[-1])["coarsen"] == "nested"
    # a fixed count with cycle options and a source through the general transfers
    f = run_app("mpi_jacobi2d", "94", "4", "--ny=62", "--init=random", "--mg", "--coarsen=any", "--nu=1,2",
                "--omega=0.7", "--levels=3", "--check", "--source=random", np=2)
    assert re.search(r"levels    = 3 \(coarsest 14 x 22,", f.stdout) and re.search(CHECK_OK, f.stdout), f.stdout


def test_kernel_bench_mg_even_host():
    """gmt_kernel_bench --only=mg --mg-n=64 on the CPU backend: the nested kernels at 63 and the two
    table-driven transfers at 64, each beside its DAXPY, and the ratio line."""
    out = run_app("gmt_kernel_bench", "--only=mg", "--mg-n=64", "--iters=2", "--reps=1").stdout
    for k in ("mg_smooth", "mg_smooth_f", "mg_restrict", "mg_prolong_add"):
        assert len(re.findall(rf"^{k}\s+v0\s+63x63 best", out, re.M)) == 1, out
    for k in ("mg_restrict_tab", "mg_prolong_add_tab"):
        assert len(re.findall(rf"^{k}\s+v0\s+64x64 best", out, re.M)) == 1, out
        assert re.search(rf"{k} GB/s / daxpy GB/s = [0-9.]+", out), out
    assert re.search(r"mg_restrict_tab ms / mg_restrict ms at 63 = [0-9.]+, mg_prolong_add_tab ms / mg_prolong_add ms = "
                     r"[0-9.]+", out), out
    assert len(re.findall(r"^daxpy\s+v[1-6]", out, re.M)) == 6, out
