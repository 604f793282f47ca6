"""residual_norm and solve-to-tolerance of the native Jacobi engine on the CPU
backend (JacobiSolver::residual_norm / solve, NativeJacobi.residual_norm /
solve, mpi_jacobi2d --tol / --rtol).

residual_norm is read-only (the field, and what later sweeps compute, are
unchanged), repeatable and equal to the NumPy residual of the serial solve.
solve() is asked for a tolerance that the NumPy reference series first meets
at a chosen check c (solve_worker.pick_rtol: at least 2.5% from either
neighbouring check, where summation order moves a value by 1e-11), so the
deciding check, the sweeps advanced behind it (lag), the number of checks and
the final field (bitwise the serial solve of `sweeps` sweeps) are all fixed
numbers, on every rank alike."""
import json
import math
import os
import re
import subprocess
import sys

import pytest

from conftest import free_port
from native_util import ROOT, ensure_host_build, have_mpi, run_app
from solve_worker import pick_rtol, ref_residuals

WORKER = os.path.join(ROOT, "tests", "solve_worker.py")


def _worker(cfg, np_=1, transport="rccl"):
    ensure_host_build()
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    if np_ == 1:
        cmd = [sys.executable, WORKER, json.dumps(cfg)]
    else:
        env["GMT_TRANSPORT"] = transport
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(np_),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), WORKER, json.dumps(cfg)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def check_residual_norm(r, ny, nx, periodic, n1):
    """The residual_norm part of a worker result against NumPy."""
    assert r["unchanged"] and r["rn_same"], r
    assert r["rn"][0] == r["rn"][1], r["rn"]  # a second call returns the identical pair
    ref = ref_residuals(ny, nx, periodic, tuple(sorted({0, n1})))
    for got, s in ((r["rn"][0], 0), (r["rn"][2], n1)):
        for g, w in zip(got, ref[s]):
            assert abs(g - w) <= 1e-11 * max(1.0, w), (s, got, ref[s])
    assert r["run_equal"], r  # no stale or double-exchanged ghost: the later sweeps are the serial ones


def check_case(case, got, ny, nx, periodic, every, c):
    """One solve case whose tolerance the reference first meets at check c."""
    res, lag = got["res"], case.get("lag", 1)
    assert got["same"], got  # the same dict on every rank
    assert res["converged"] == 1 and res["failed"] == 0, res
    assert res["residual_sweeps"] == c * every, res
    assert res["sweeps"] == (c + lag) * every, res
    assert res["checks"] == c + lag + 1, res
    k = 0 if case.get("norm", "l2") == "l2" else 1
    ser = ref_residuals(ny, nx, periodic, tuple(i * every for i in range(c + 1)))
    assert abs(res["residual"] - ser[c * every][k]) <= 1e-11 * max(1.0, ser[c * every][k]), (res, ser[c * every])
    assert abs(res["residual_max"] - ser[c * every][1]) <= 1e-11, (res, ser[c * every])
    assert abs(res["r0"] - ser[0][k]) <= 1e-11 * max(1.0, ser[0][k]), (res, ser[0])
    assert got["equal"], got  # interior() is bitwise serial_jacobi(sweeps)


def solve_cases(ny, nx, periodic, every, specs, check_every=None):
    """specs: (c, lag, norm) -> the worker's case dicts with their rtol."""
    out = []
    for c, lag, norm in specs:
        rtol, _ = pick_rtol(ny, nx, periodic, every, c, norm)
        out.append(dict(rtol=rtol, norm=norm, lag=lag, max_sweeps=12 * every,
                        check_every=every if check_every is None else check_every))
    return out


BAD = [dict(tol=1.0, max_sweeps=0), dict(tol=1.0, max_sweeps=25, check_every=12), dict(tol=1.0, max_sweeps=-12, check_every=12),
       dict(tol=1.0, max_sweeps=24, check_every=-1), dict(tol=1.0, max_sweeps=24, check_every=12, lag=-1),
       dict(tol=1.0, max_sweeps=24, check_every=12, lag=9), dict(max_sweeps=24, check_every=12),
       dict(tol=-1.0, max_sweeps=24, check_every=12), dict(tol=1.0, max_sweeps=24, check_every=12, norm="l1")]


@pytest.mark.parametrize("tsteps,every,periodic,pre", [(1, 12, False, (5, 7)), (8, 16, True, (11, 13)),
                                                       (20, 20, False, (27, 13))])
def test_one_rank(tsteps, every, periodic, pre):
    """60 x 64 on one rank: lag 0, 1 and 3, both norms, single sweeps and
    fused passes; a tolerance already met, a cap reached, every argument error."""
    ny, nx = 60, 64
    specs = [(4, 1, "l2"), (3, 0, "max"), (5, 3, "l2"), (6, 0, "l2")]
    cases = solve_cases(ny, nx, periodic, every, specs)
    r0 = ref_residuals(ny, nx, periodic, (0,))[0][0]
    extra = [dict(tol=2.0 * r0, lag=0, max_sweeps=3 * every, check_every=every),   # met at check 0
             dict(tol=2.0 * r0, lag=1, max_sweeps=3 * every, check_every=every),
             dict(rtol=1e-30, lag=1, max_sweeps=3 * every, check_every=every)]     # out of reach: the cap
    r = _worker(dict(ny=ny, nx=nx, tsteps=tsteps, periodic=periodic, pre=pre, cases=cases + extra, bad=BAD))
    assert r["tsteps"] == tsteps
    check_residual_norm(r, ny, nx, periodic, pre[0])
    for (c, _, _), case, got in zip(specs, cases, r["cases"]):
        check_case(case, got, ny, nx, periodic, every, c)
    met0, met1, cap = (g["res"] for g in r["cases"][len(cases):])
    assert (met0["converged"], met0["sweeps"], met0["residual_sweeps"], met0["checks"]) == (1, 0, 0, 1), met0
    # with lag 1 the device is one check ahead when the host sees check 0
    assert (met1["converged"], met1["sweeps"], met1["residual_sweeps"], met1["checks"]) == (1, every, 0, 2), met1
    assert (cap["converged"], cap["failed"], cap["sweeps"], cap["residual_sweeps"], cap["checks"]) == \
        (0, 0, 3 * every, 3 * every, 4), cap
    assert all(g["equal"] and g["same"] for g in r["cases"]), r["cases"]
    assert r["bad"] == [True] * len(BAD), r["bad"]


@pytest.mark.parametrize("np_,transport,ny,nx,tsteps,every,dims,periodic,overlap", [
    (2, "rccl", 60, 64, 20, 20, (2, 1), False, False),
    (2, "ipc", 300, 700, 12, 12, (1, 2), True, True),
    (4, "rccl", 300, 700, 8, 16, (2, 2), True, False),
    (4, "ipc", 60, 64, 1, 12, (2, 2), False, True),
])
def test_ranks(np_, transport, ny, nx, tsteps, every, dims, periodic, overlap):
    """2 and 4 ranks over the host emulations of RCCL and IPC: every rank
    takes the same decision at the same check."""
    specs = [(4, 1, "l2"), (3, 0, "max"), (5, 3, "l2")]
    cases = solve_cases(ny, nx, periodic, every, specs)
    pre = (tsteps + 3, 9)
    r = _worker(dict(ny=ny, nx=nx, tsteps=tsteps, dims=dims, periodic=periodic, overlap=overlap, pre=pre,
                     cases=cases), np_, transport)
    assert r["transport"] == f"{transport}-host", r
    check_residual_norm(r, ny, nx, periodic, pre[0])
    for (c, _, _), case, got in zip(specs, cases, r["cases"]):
        check_case(case, got, ny, nx, periodic, every, c)


def _analytic_series(ny, nx, every, n):
    """L2 residuals of the app's analytic field (x^3 + y^2, Dirichlet) at sweeps i * every."""
    from gpu_mpi_tests_amd import engine

    u = engine.initial_field(ny, nx)
    un = u.copy()
    out = []
    for s in range(n * every + 1):
        if s % every == 0:
            d = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1])) - u[1:-1, 1:-1]
            out.append(math.sqrt(math.fsum((d * d).ravel().tolist())))
        un[1:-1, 1:-1] = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1]))
        u, un = un, u
    return out


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
@pytest.mark.parametrize("np_", [1, 2, 4])
def test_app_solve(np_, tmp_path):
    """mpi_jacobi2d 64 600 --ny=60 --tblock --tsteps=12 --rtol=R --check: the
    new lines and JSON keys; the cap 600 is a multiple of 12."""
    ser = _analytic_series(60, 64, 12, 12)
    c = 6
    rtol = math.sqrt(ser[c - 1] * ser[c]) / ser[0]
    js = tmp_path / "out.json"
    p = run_app("mpi_jacobi2d", "64", "600", "--ny=60", "--tblock", "--tsteps=12", f"--rtol={rtol!r}", "--check",
                f"--json={js}", np=np_)
    out = p.stdout
    assert "converged : yes" in out, out
    m = re.search(r"sweeps    : (\d+) \(criterion met at (\d+), (\d+) checks, lag 1\)", out)
    assert m, out
    met = int(m.group(2))
    assert int(m.group(1)) == met + 12 and int(m.group(3)) == met // 12 + 2, out
    # the analytic field decays about 1% per check: the crossing may sit within rounding of a check
    assert abs(met - c * 12) <= 12, (met, ser)
    assert re.search(r"TIME solve: [0-9.]+ ms", out), out
    assert re.search(r"residual  : [0-9.e+-]+", out), out
    assert re.search(r"check\s*: max\|diff\| vs serial = [0-9.eE+-]+ OK", out), out
    j = json.loads(js.read_text().strip().splitlines()[-1])
    for k in ("converged", "sweeps", "residual_sweeps", "checks", "solve_ms", "r0", "residual_max"):
        assert k in j, j
    assert j["converged"] is True and j["sweeps"] == int(m.group(1)) and j["residual_sweeps"] == met, j
    # the JSON record keeps 9 significant digits; the report line prints 11
    assert abs(j["r0"] - ser[0]) <= 1e-8 * ser[0], (j, ser[0])
    assert abs(j["residual"] - ser[met // 12]) <= 1e-8 * ser[met // 12], (j, ser)
    shown = float(re.search(r"residual  : ([0-9.e+-]+)", out).group(1))
    assert abs(shown - ser[met // 12]) <= 1e-10 * ser[met // 12], (shown, ser)


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
def test_app_cap_and_plain_run():
    """An unreachable --tol exits 4 at the (rounded-up) cap; without the flags
    the app prints none of the new lines."""
    p = run_app("mpi_jacobi2d", "64", "30", "--ny=60", "--tblock", "--tsteps=12", "--tol=1e-300", "--lag=2", np=2,
                check=False)
    assert p.returncode == 4, p.stdout + p.stderr
    assert "converged : no" in p.stdout and "rounded up to a multiple of 12" in p.stdout, p.stdout
    assert re.search(r"sweeps    : 36 \(criterion met at 36, 4 checks, lag 2\)", p.stdout), p.stdout
    q = run_app("mpi_jacobi2d", "64", "30", "--ny=60", "--tblock", "--tsteps=12", "--warmup=2", np=2)
    for word in ("converged", "sweeps    :", "TIME solve", "solve     ="):
        assert word not in q.stdout, q.stdout
    assert "steps     = 30 (warmup 2)" in q.stdout and "residual  :" in q.stdout, q.stdout
