"""Geometric multigrid of the native Jacobi engine on the CPU backend
(JacobiSolver::mg, NativeJacobi.mg) against the NumPy definition
engine.serial_mg, on 1, 2, 4 and 6 ranks over the host emulations of RCCL and
IPC (tests/mg_worker.py under torch.distributed.run).

Global 255 x 767: the fine level crosses the 512-column workgroup seam; seven
coarse levels down to 1 x 5 on grids with one process row.  A grid with two
process rows stops at 3 x 11, because a rank must keep a coarse row: the level
table is engine.mg_levels' on every grid, and serial_mg runs with that many
levels.
Field: after n cycles interior() is BITWISE serial_mg on every process grid
(every rank's share is gathered), with and without a source, for nu = (2, 2)
and (1, 1), for max_levels = 3, for a second call and for run() afterwards.
Residuals (r0 and the deciding one): within 2e-13 relative of the math.fsum
residuals of the serial fields.
Convergence is a condition on the reference: serial_mg reaches rtol = 1e-6
within 10 cycles from the random field, and no residual of its series lies
within 1% of the threshold; with lag 0 the engine then decides at the same
cycle, with lag 1 and 3 that many cycles later."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import free_port
from mg_worker import SEED, reference
from native_util import ROOT, ensure_host_build

WORKER = os.path.join(ROOT, "tests", "mg_worker.py")
NY, NX = 255, 767
CYCLES = 3
RTOL = 1e-6
CAP = 12
RUN_AFTER = 5
BAD = [dict(max_cycles=0), dict(max_cycles=5, check_every=2), dict(max_cycles=-2), dict(max_cycles=2, check_every=-1),
       dict(max_cycles=2, lag=-1), dict(max_cycles=2, lag=9), dict(tol=-1.0, max_cycles=2), dict(rtol=-1e-3, max_cycles=2),
       dict(rtol=float("nan"), max_cycles=2), dict(tol=float("inf"), max_cycles=2), dict(max_cycles=2, norm="l1"),
       dict(max_cycles=2, nu=(0, 0)), dict(max_cycles=2, nu=(-1, 2)), dict(max_cycles=2, nu=(2, -1)),
       dict(max_cycles=2, omega=0.0), dict(max_cycles=2, omega=1.5), dict(max_cycles=2, omega=float("nan")),
       dict(max_cycles=2, max_levels=1), dict(max_cycles=2, max_levels=-1), dict(max_cycles=2, coarse_iters=-1)]


def launch_cpu(cfg, np_=1, transport="rccl"):
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
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{") or ln.startswith("[")][-1])


def same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                                      np.ascontiguousarray(b).view(np.int64)))


def close(got, want):
    return abs(got - want) <= 2e-13 * abs(want)


def sweeps_from(field, source, k):
    """k NumPy Jacobi sweeps from `field` inside the engine's Dirichlet ring."""
    from gpu_mpi_tests_amd import engine

    u = engine.initial_field(NY, NX, "random", SEED)
    u[1:-1, 1:-1] = field
    s = None if source is None else engine.source_field(NY, NX, source, SEED)
    for _ in range(k):
        un = u.copy()
        un[1:-1, 1:-1] = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1]))
        if s is not None:
            un[1:-1, 1:-1] += s
        u = un
    return u[1:-1, 1:-1]


def deciding_cycle(series):
    """The first cycle whose L2 residual meets RTOL, with every value of the series clear of the threshold."""
    thr = RTOL * series[0][0]
    c = next(i for i, (r, _) in enumerate(series) if r <= thr)
    assert all(abs(r - thr) > 0.01 * thr for r, _ in series), (thr, series)
    return c


def standard_ops(tsteps=1):
    return [
        dict(op="rn"),
        dict(op="mg", tag="c3", kw=dict(max_cycles=CYCLES, lag=1)),
        dict(op="run", k=RUN_AFTER * tsteps, tag="run"),
        dict(op="mg", tag="again", kw=dict(max_cycles=2, check_every=2, lag=0)),
        # an odd number of sweeps a cycle: the parity flips
        dict(op="reset"), dict(op="mg", tag="odd", kw=dict(max_cycles=CYCLES, nu=(1, 1), lag=0)),
        dict(op="run", k=2 * tsteps, tag="run_odd"),
        # three levels: a coarsest level of many cells
        dict(op="reset"), dict(op="mg", tag="l3", kw=dict(max_cycles=2, max_levels=3)),
        # the decision, lag 0, 1 and 3
        dict(op="reset"), dict(op="mg", tag="d0", kw=dict(rtol=RTOL, max_cycles=CAP, lag=0)),
        dict(op="reset"), dict(op="mg", tag="d1", kw=dict(rtol=RTOL, max_cycles=CAP, lag=1)),
        dict(op="reset"), dict(op="mg", tag="d3", kw=dict(rtol=RTOL, max_cycles=CAP, lag=3)),
        # the cap, a tolerance met by the starting field
        dict(op="reset"), dict(op="mg", kw=dict(rtol=1e-30, max_cycles=2, lag=1)),
        dict(op="reset"), dict(op="mg", tag="t0", kw=dict(tol=1e300, max_cycles=4, lag=2)),
    ]


def check_standard(res, fields, dims, source, tsteps=1, umax=None):
    """The results of standard_ops against serial_mg.  With fused passes (tsteps > 1) run() after
    mg() agrees with NumPy sweeps within 1e-10 max|u0|, the bound of the CG and Chebyshev tests."""
    from gpu_mpi_tests_amd import engine

    table = engine.mg_levels(NY, NX, dims)
    nlev = len(table)
    ref_f, ser = reference(NY, NX, CAP, source, (2, 2), nlev)
    rn, c3, _, again, _, odd, _, _, l3, _, d0, _, d1, _, d3, _, cap, _, t0 = res[1:]

    def hierarchy(r, levels, shape):
        rho = engine.cheby_rho(*shape)
        assert r["levels"] == levels and (r["coarse_ny"], r["coarse_nx"]) == tuple(shape), r
        assert r["coarse_rho"] == rho and r["coarse_iters"] == engine.mg_coarse_iters(rho), (r, rho)

    # three cycles
    r = c3["res"]
    assert c3["same"] and r["iters"] == CYCLES and r["checks"] == CYCLES + 1 and not r["converged"] and not r["failed"], r
    hierarchy(r, nlev, table[-1])
    assert rn["same"] and close(rn["rn"][0], ser[0][0]) and close(rn["rn"][1], ser[0][1]), (rn, ser[0])
    assert close(r["r0"], ser[0][0]) and close(r["residual"], ser[CYCLES][0]), (r, ser)
    assert close(r["residual_max"], ser[CYCLES][1]), (r, ser)
    assert same_bits(fields["c3"], ref_f[CYCLES])
    # run() keeps sweeping from it; a second call starts from that field
    swept = sweeps_from(ref_f[CYCLES], source, RUN_AFTER * tsteps)
    if tsteps == 1:
        assert same_bits(fields["run"], swept)
    else:
        assert float(np.abs(fields["run"] - swept).max()) <= 1e-10 * umax
    f2, ser2 = engine.serial_mg(NY, NX, 2, init="random", seed=SEED, source=source, max_levels=nlev,
                                start=fields["run"])
    r = again["res"]
    assert again["same"] and r["iters"] == 2 and r["checks"] == 2, r
    assert close(r["r0"], ser2[0][0]) and close(r["residual"], ser2[2][0]), (r, ser2)
    assert same_bits(fields["again"], f2)
    # nu = (1, 1)
    fo, sero = reference(NY, NX, CYCLES, source, (1, 1), nlev)
    r = odd["res"]
    assert odd["same"] and r["iters"] == CYCLES and close(r["residual"], sero[CYCLES][0]), (r, sero)
    assert same_bits(fields["odd"], fo[CYCLES])
    swept = sweeps_from(fo[CYCLES], source, 2 * tsteps)
    if tsteps == 1:
        assert same_bits(fields["run_odd"], swept)
    else:
        assert float(np.abs(fields["run_odd"] - swept).max()) <= 1e-10 * umax
    # max_levels = 3
    f3, ser3 = reference(NY, NX, 2, source, (2, 2), 3)
    r = l3["res"]
    hierarchy(r, 3, engine.mg_levels(NY, NX, dims, 3)[-1])
    assert (r["coarse_ny"], r["coarse_nx"]) == (63, 191) and r["coarse_iters"] > 20, r
    assert l3["same"] and close(r["residual"], ser3[2][0]), (r, ser3)
    assert same_bits(fields["l3"], f3[2])
    # the decision: a condition on the reference first
    c = deciding_cycle(ser)
    assert 1 <= c <= 10, (c, ser)
    for lag, d in ((0, d0), (1, d1), (3, d3)):
        r = d["res"]
        iters = min(c + lag, CAP)
        assert d["same"] and r["converged"] == 1 and r["residual_iters"] == c and r["iters"] == iters, (lag, r, c)
        assert r["checks"] == iters + 1 and close(r["residual"], ser[c][0]) and close(r["r0"], ser[0][0]), (lag, r)
        assert same_bits(fields[f"d{lag}"], ref_f[iters]), lag
    # the cap; a tolerance met at check 0 (lag 2: two more cycles have run)
    r = cap["res"]
    assert cap["same"] and not r["converged"] and r["iters"] == 2 and r["checks"] == 3 and r["residual_iters"] == 2, r
    r = t0["res"]
    assert t0["same"] and r["converged"] == 1 and r["residual_iters"] == 0 and r["iters"] == 2 and r["checks"] == 3, r
    assert same_bits(fields["t0"], ref_f[2])


GRIDS = [(1, None, "rccl"), (2, (1, 2), "rccl"), (2, (2, 1), "ipc"), (4, (2, 2), "rccl"), (6, (2, 3), "ipc")]


@pytest.mark.parametrize("source", [None, "random"])
@pytest.mark.parametrize("np_,dims,transport", GRIDS, ids=lambda v: None if isinstance(v, int) else str(v))
def test_mg_against_serial(np_, dims, transport, source, tmp_path):
    out = str(tmp_path / "fields.npz")
    res = launch_cpu(dict(ny=NY, nx=NX, dims=dims, source=source, ops=standard_ops(), out=out), np_, transport)
    check_standard(res, dict(np.load(out)), dims or (1, 1), source)


def test_levels_and_coarse_iters():
    from gpu_mpi_tests_amd import engine

    full = [(255, 767), (127, 383), (63, 191), (31, 95), (15, 47), (7, 23), (3, 11), (1, 5)]
    assert engine.mg_levels(NY, NX, (1, 1)) == full and engine.mg_levels(NY, NX, (1, 2)) == full
    for dims in ((2, 1), (2, 2), (2, 3)):
        assert engine.mg_levels(NY, NX, dims) == full[:-1]  # a process row would own no row of 1 x 5
    assert engine.mg_levels(NY, NX, (1, 1), 3) == full[:3]
    assert engine.mg_levels(300, 700, (1, 1)) == [(300, 700)] and engine.mg_levels(255, 766, (1, 1)) == [(255, 766)]
    assert engine.mg_levels(8191, 8191, (1, 1))[-1] == (1, 1) and len(engine.mg_levels(8192, 8192, (1, 1))) == 1
    assert engine.mg_coarse_iters(0.0) == 1 and engine.mg_coarse_iters(engine.cheby_rho(1, 5)) == 3
    # the count follows the bound: sigma^k is the Chebyshev reduction factor's t
    for rho in (0.3, 0.9, 0.999, engine.cheby_rho(63, 191)):
        k = engine.mg_coarse_iters(rho)
        sigma = (1.0 - (1.0 - rho * rho) ** 0.5) / rho
        red = lambda n: 2.0 * sigma ** n / (1.0 + sigma ** (2 * n))  # noqa: E731
        assert red(k) <= 0.1 * (1 + 1e-12) and (k == 1 or red(k - 1) > 0.1 * (1 - 1e-12)), (rho, k)


def test_refusals():
    """Bad options, a periodic axis and problems without a coarse level are refused."""
    from gpu_mpi_tests_amd import engine

    ops = [dict(op="bad", kws=BAD), dict(op="periodic"), dict(op="nocoarse", shape=(300, 700)),
           dict(op="nocoarse", shape=(255, 766))]
    for np_, dims in ((1, None), (2, (1, 2))):
        res = launch_cpu(dict(ny=NY, nx=NX, dims=dims, ops=ops), np_)
        bad, periodic, no1, no2 = res[1:]
        assert bad == [True] * len(BAD), bad
        assert periodic and "periodic" in periodic, periodic
        for msg in (no1, no2):
            assert msg and "no coarse level" in msg and "must be even" in msg, msg
    # a rank without a coarse point: 3 x 767 over two process rows
    res = launch_cpu(dict(ny=NY, nx=NX, dims=(2, 1), ops=[dict(op="nocoarse", shape=(3, 767))]), 2)
    assert res[1] and "no coarse level" in res[1] and "own no coarse point" in res[1], res[1]
    assert engine.mg_levels(3, 767, (2, 1)) == [(3, 767)] and len(engine.mg_levels(3, 767, (1, 1))) == 2
