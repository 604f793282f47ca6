"""Conjugate gradients of the native Jacobi engine on the CPU backend
(JacobiSolver::cg, NativeJacobi.cg, mpi_jacobi2d --cg) against the NumPy
definition engine.serial_cg, on 1, 2 and 4 ranks over the host emulations of
RCCL and IPC (tests/cg_worker.py under torch.distributed.run).

Series: the engine's (residual, residual_max) after every check of the first
120 iterations equals serial_cg's within a relative 1e-9 — between summation
orders (NumPy pairwise, fsum, per-rank partial sums) the series differ by at
most 3e-13, so a deviation above 1e-10 is a bug, not a tolerance to loosen;
nothing is compared where the reference's own residual is below 1e-7 * r0.
Decision: rtol is chosen so that the reference first meets it at a check c with
every checked value up to c at least 2.5% away (cg_worker.pick_rtol: CG's
residual is not monotone), so residual_iters, iters and checks are fixed
numbers, on every rank alike.  Field: interior() is within 1e-10 * max|u0| of
serial_cg(iters), and so are the fields of 1, 2 and 4 ranks of each other.
r0 equals residual_norm() of the starting field (1e-12 relative for L2,
bitwise for max); with lag 0 the true residual is within 1e-10 * r0 of the
recursive one."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cg_worker import SEED, pick_rtol, reference
from conftest import free_port
from native_util import ROOT, ensure_host_build, have_mpi, run_app

WORKER = os.path.join(ROOT, "tests", "cg_worker.py")
SERIES_UPTO = 120
SPECS = [(0, "l2"), (1, "max"), (3, "l2")]  # (lag, norm) of the decision cases
RUN_AFTER = 7
BAD = [dict(rtol=1e-3, max_iters=0), dict(rtol=1e-3, max_iters=25, check_every=10), dict(rtol=1e-3, max_iters=-10),
       dict(rtol=1e-3, max_iters=20, check_every=-1), dict(rtol=1e-3, max_iters=20, lag=-1),
       dict(rtol=1e-3, max_iters=20, lag=9), dict(tol=-1.0, max_iters=20), dict(rtol=-1e-3, max_iters=20),
       dict(rtol=float("nan"), max_iters=20), dict(tol=float("inf"), max_iters=20),
       dict(rtol=1e-3, max_iters=20, norm="l1")]
worst = {"series": 0.0, "field": 0.0, "true": 0.0}  # the largest deviations seen (printed by each test)


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


# ---------------------------------------------------------------- the standard run
def standard_plan(ny, nx, every, lo, init="random", series_every=None, beats=False, specs=SPECS, n_ref=None):
    """The ops of one worker run and what the reference says about them.  One reference run serves the
    series, the picks and the fields (kept at every check); configurations of one shape share it."""
    n = n_ref or max(SERIES_UPTO, (lo + 6) * every)
    while True:
        fields, ser = reference(ny, nx, n, init, None, tuple(range(0, n + 1, every)))
        try:
            picks = [pick_rtol(ser, every, lo + i, norm) for i, (_, norm) in enumerate(specs)]
            if all((c + lag) * every <= n for (lag, _), (c, _) in zip(specs, picks)):
                break
        except AssertionError:
            pass
        n += 10 * every
        assert n <= 400, "no decidable check in 400 iterations"
    ops = [dict(op="rn")]
    if series_every:
        ops.append(dict(op="series", every=series_every, upto=SERIES_UPTO))
    keep = {0}
    for i, ((lag, norm), (c, rtol)) in enumerate(zip(specs, picks)):
        cap = (c + lag + 2) * every
        ops += [dict(op="reset"), dict(op="cg", tag=f"d{i}", kw=dict(rtol=rtol, norm=norm, lag=lag, check_every=every,
                                                                    max_iters=cap))]
        keep.add((c + lag) * every)
        if i == 0:  # sweeps from the solution, then a second solve on the same engine
            ops += [dict(op="run", k=RUN_AFTER, tag="run"), dict(op="rn"),
                    dict(op="cg", tag="again", kw=dict(rtol=0.5, lag=0, check_every=every, max_iters=12 * every))]
    ops += [dict(op="reset"), dict(op="cg", tag="fixed", kw=dict(max_iters=2 * every, check_every=every)),
            dict(op="reset"), dict(op="cg", kw=dict(rtol=1e-30, max_iters=2 * every, check_every=every, lag=1)),
            dict(op="bad", kws=BAD), dict(op="periodic")]
    keep.add(2 * every)
    if beats:
        ops += [dict(op="reset"), dict(op="cg", kw=dict(rtol=1e-4, max_iters=200, check_every=5, lag=0)),
                dict(op="solve", kw=dict(rtol=1e-4, max_sweeps=200, check_every=20))]
    assert max(keep) <= n and all(k % every == 0 for k in keep)
    return dict(ops=ops, picks=picks, fields=fields, series=ser, every=every, series_every=series_every,
                beats=beats, specs=specs, init=init)


def sweeps_from(field, ny, nx, init, k):
    """k NumPy Jacobi sweeps from `field` inside the engine's Dirichlet ring."""
    from gpu_mpi_tests_amd import engine

    u = engine.initial_field(ny, nx, init, SEED)
    u[1:-1, 1:-1] = field
    un = u.copy()
    for _ in range(k):
        un[1:-1, 1:-1] = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1]))
        u, un = un, u
    return u[1:-1, 1:-1].copy()


def rel(a, b):
    return abs(a - b) / abs(b)


def check_standard(plan, results, got_fields, ny, nx):
    ser, every, init = plan["series"], plan["every"], plan["init"]
    info, results = results[0], results[1:]
    umax = info["umax"]
    bound = 1e-10 * umax
    it = iter(zip(plan["ops"], results))
    nxt = lambda kind: next(r for o, r in it if o["op"] == kind)  # noqa: E731
    rn0 = nxt("rn")
    assert rn0["same"]
    for g, w in zip(rn0["rn"], ser[0]):
        assert rel(g, w) <= 1e-11, (rn0, ser[0])
    if plan["series_every"]:
        s = nxt("series")
        assert s["same"]
        for i, (r2, rm, r0) in enumerate(s["series"]):
            k = (i + 1) * plan["series_every"]
            if ser[k][0] < 1e-7 * ser[0][0]:
                break  # the rounding floor of the reference itself
            dev = max(rel(r2, ser[k][0]), rel(rm, ser[k][1]))
            worst["series"] = max(worst["series"], dev)
            assert dev <= 1e-9, (k, r2, rm, ser[k])
            assert rel(r0, rn0["rn"][0]) <= 1e-12
    for i, ((lag, norm), (c, rtol)) in enumerate(zip(plan["specs"], plan["picks"])):
        g = nxt("cg")
        res = g["res"]
        kn = 0 if norm == "l2" else 1
        assert g["same"], g
        assert (res["converged"], res["failed"]) == (1, 0), res
        assert res["residual_iters"] == c * every and res["iters"] == (c + lag) * every, (res, c, lag)
        assert res["checks"] == c + lag + 1, res
        assert rel(res["residual"], ser[c * every][kn]) <= 1e-9 and rel(res["residual_max"], ser[c * every][1]) <= 1e-9
        # r0 is residual_norm() of the starting field: 1e-12 relative for L2, bitwise for max
        assert (rel(res["r0"], rn0["rn"][0]) <= 1e-12) if norm == "l2" else (res["r0"] == rn0["rn"][1]), (res, rn0)
        true = res["true_residual"] if norm == "l2" else res["true_residual_max"]
        assert math.isfinite(res["true_residual"]) and math.isfinite(res["true_residual_max"])
        if lag == 0:
            worst["true"] = max(worst["true"], abs(true - res["residual"]) / res["r0"])
            assert abs(true - res["residual"]) <= 1e-10 * res["r0"], res
        else:  # the later iterate's: it meets the criterion or lies below the deciding one
            assert true <= rtol * res["r0"] or true < res["residual"], res
        err = float(np.abs(got_fields[f"d{i}"] - plan["fields"][res["iters"]]).max())
        worst["field"] = max(worst["field"], err / umax)
        assert err <= bound, (i, err, bound)
        if i == 0:
            # run(k) keeps sweeping from the solution with re-exchanged ghosts
            want = sweeps_from(got_fields["d0"], ny, nx, init, RUN_AFTER)
            assert float(np.abs(got_fields["run"] - want).max()) <= bound
            rn = nxt("rn")
            again = nxt("cg")
            a = again["res"]
            assert again["same"] and a["failed"] == 0 and a["converged"] == 1, a
            assert rel(a["r0"], rn["rn"][0]) <= 1e-12 and a["residual"] <= 0.5 * a["r0"], (a, rn)
            assert abs(a["true_residual"] - a["residual"]) <= 1e-10 * a["r0"], a
            assert np.isfinite(got_fields["again"]).all()
    fixed = nxt("cg")["res"]
    assert (fixed["converged"], fixed["failed"], fixed["iters"], fixed["residual_iters"], fixed["checks"]) == \
        (0, 0, 2 * every, 2 * every, 3), fixed
    assert rel(fixed["residual"], ser[2 * every][0]) <= 1e-9, (fixed, ser[2 * every])
    assert float(np.abs(got_fields["fixed"] - plan["fields"][2 * every]).max()) <= bound
    cap = nxt("cg")["res"]
    assert (cap["converged"], cap["failed"], cap["iters"], cap["residual_iters"], cap["checks"]) == \
        (0, 0, 2 * every, 2 * every, 3), cap
    assert nxt("bad") == [True] * len(BAD)
    assert nxt("periodic") is True
    if plan["beats"]:
        cg = nxt("cg")["res"]
        jac = nxt("solve")["res"]
        assert cg["converged"] == 1 and cg["iters"] <= 200, cg
        assert jac["converged"] == 0 and jac["sweeps"] == 200 and jac["residual"] > 1e-2 * jac["r0"], jac
    print("largest deviations so far:", worst)


_cache = {}


def standard_cpu(name, tmp_path_factory):
    """One worker run per configuration, shared by the tests that look at it."""
    if name not in _cache:
        np_, transport, ny, nx, dims, every, lo, series_every, beats = CONFIGS[name]
        plan = standard_plan(ny, nx, every, lo, series_every=series_every, beats=beats)
        out = str(tmp_path_factory.mktemp("cg") / "fields.npz")
        res = launch_cpu(dict(ny=ny, nx=nx, dims=dims, ops=plan["ops"], out=out), np_, transport)
        _cache[name] = (plan, res, dict(np.load(out)))
    return _cache[name]


# name -> ranks, transport, ny, nx, dims, check_every, first candidate check, series check_every, beats-Jacobi case
CONFIGS = {
    "60x64 1": (1, "rccl", 60, 64, None, 5, 6, 10, True),
    "60x64 1x2 rccl": (2, "rccl", 60, 64, (1, 2), 5, 6, 10, False),
    "60x64 2x1 ipc": (2, "ipc", 60, 64, (2, 1), 5, 6, None, False),
    "60x64 2x2 rccl": (4, "rccl", 60, 64, (2, 2), 5, 6, None, False),
    "60x64 2x2 ipc": (4, "ipc", 60, 64, (2, 2), 5, 6, 10, False),
    "300x700 1": (1, "rccl", 300, 700, None, 10, 3, 20, False),
    "300x700 1x2 ipc": (2, "ipc", 300, 700, (1, 2), 10, 3, None, False),
    "300x700 2x2 rccl": (4, "rccl", 300, 700, (2, 2), 10, 3, 20, False),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_cg_against_serial(name, tmp_path_factory):
    plan, res, fields = standard_cpu(name, tmp_path_factory)
    np_, transport, ny, nx = CONFIGS[name][:4]
    if np_ > 1:
        assert res[0]["transport"] == f"{transport}-host", res[0]
    check_standard(plan, res, fields, ny, nx)


@pytest.mark.parametrize("names", [("60x64 1", "60x64 1x2 rccl", "60x64 2x1 ipc", "60x64 2x2 ipc"),
                                   ("300x700 1", "300x700 1x2 ipc", "300x700 2x2 rccl")])
def test_same_field_on_1_2_4_ranks(names, tmp_path_factory):
    """The solutions of different process grids agree within the bound of the serial comparison."""
    runs = [standard_cpu(n, tmp_path_factory) for n in names]
    umax = runs[0][1][0]["umax"]
    for tag in ("d0", "d1", "d2", "fixed"):
        for _, _, f in runs[1:]:
            assert float(np.abs(f[tag] - runs[0][2][tag]).max()) <= 1e-10 * umax, tag


def test_analytic_init_decision():
    """The analytic field: the residual first rises above r0 and steps upward many times on its way down."""
    ny, nx, every = 60, 64, 5
    plan = standard_plan(ny, nx, every, 20, init="analytic", specs=[(1, "l2")])
    ser = plan["series"]
    assert max(s[0] for s in ser) > 2 * ser[0][0] and sum(b[0] > a[0] for a, b in zip(ser, ser[1:])) >= 8
    (c, rtol), = plan["picks"]
    res = launch_cpu(dict(ny=ny, nx=nx, dims=(1, 2), init="analytic", ops=[
        dict(op="cg", kw=dict(rtol=rtol, lag=1, check_every=every, max_iters=(c + 3) * every))]), 2, "rccl")
    r = res[1]["res"]
    assert res[1]["same"] and (r["converged"], r["residual_iters"], r["iters"], r["checks"]) == \
        (1, c * every, (c + 1) * every, c + 2), (r, c)


@pytest.mark.parametrize("np_,dims", [(1, None), (2, (2, 1))])
def test_sources(np_, dims, tmp_path):
    """source="poly" with the analytic field: already the discrete fixed point,
    so r0 is at rounding level and a tol above it converges at check 0 with
    iters == lag * check_every.  source="random" against serial_cg."""
    every = 5
    res = launch_cpu(dict(ny=60, nx=64, dims=dims, init="analytic", source="poly", ops=[
        dict(op="cg", kw=dict(tol=1e-10, lag=0, check_every=every, max_iters=4 * every)), dict(op="reset"),
        dict(op="cg", kw=dict(tol=1e-10, lag=2, check_every=every, max_iters=4 * every))]), np_, "ipc")
    for g, lag in ((res[1], 0), (res[3], 2)):
        r = g["res"]
        assert g["same"] and r["r0"] < 1e-12 and r["converged"] == 1 and r["residual_iters"] == 0, r
        assert r["iters"] == lag * every and r["checks"] == lag + 1, r
    out = str(tmp_path / "f.npz")
    res = launch_cpu(dict(ny=60, nx=64, dims=dims, source="random", out=out, ops=[
        dict(op="rn"), dict(op="cg", tag="f", kw=dict(max_iters=40, check_every=10, lag=1))]), np_, "ipc")
    fields, ser = reference(60, 64, 40, "random", "random", (40,))
    r = res[2]["res"]
    assert rel(r["r0"], ser[0][0]) <= 1e-11 and rel(r["r0"], res[1]["rn"][0]) <= 1e-12, (r, ser[0])
    assert r["iters"] == 40 and rel(r["residual"], ser[40][0]) <= 1e-9 and rel(r["residual_max"], ser[40][1]) <= 1e-9
    assert float(np.abs(np.load(out)["f"] - fields[40]).max()) <= 1e-10 * res[0]["umax"]


def test_serial_cg_is_cg():
    """The NumPy definition itself: residuals fall below 1e-8 * r0 within 260 iterations at 60 x 64, the field
    then solves u = J(u) to that level, and `keep` returns the fields of the single runs."""
    from gpu_mpi_tests_amd import engine

    f, ser = engine.serial_cg(60, 64, 260, init="random", seed=SEED)
    assert min(s[0] for s in ser) < 1e-8 * ser[0][0]
    d = sweeps_from(f, 60, 64, "random", 1) - f
    assert math.sqrt(float((d * d).sum())) < 1e-7 * ser[0][0]
    kept, ser2 = engine.serial_cg(60, 64, 30, init="random", seed=SEED, keep=(0, 10, 30))
    assert ser2 == ser[:31] and sorted(kept) == [0, 10, 30]
    assert np.array_equal(kept[10], engine.serial_cg(60, 64, 10, init="random", seed=SEED)[0])
    assert np.array_equal(kept[0], engine.initial_field(60, 64, "random", SEED)[1:-1, 1:-1])


# ------------------------------------------------------------------- the app
@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
@pytest.mark.parametrize("np_", [1, 2, 4])
def test_app_cg(np_, tmp_path):
    """mpi_jacobi2d 64 400 --ny=60 --init=random --cg --rtol=R --check --json: the new lines and JSON keys."""
    from gpu_mpi_tests_amd import engine

    _, ser = engine.serial_cg(60, 64, 120, init="random", seed=0)
    c, rtol = pick_rtol(ser, 10, 4)
    js = tmp_path / "out.json"
    p = run_app("mpi_jacobi2d", "64", "400", "--ny=60", "--init=random", "--cg", f"--rtol={rtol!r}", "--check",
                f"--json={js}", np=np_)
    out = p.stdout
    assert "solver    = cg" in out and "converged : yes" in out, out
    m = re.search(r"iters     : (\d+) \(criterion met at (\d+), (\d+) checks, lag 1\)", out)
    assert m, out
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == ((c + 1) * 10, c * 10, c + 2), (out, c)
    assert re.search(r"TIME solve: [0-9.]+ ms", out), out
    shown = float(re.search(r"residual  : ([0-9.e+-]+)", out).group(1))
    assert rel(shown, ser[c * 10][0]) <= 1e-9, (shown, ser[c * 10])
    assert re.search(r"true resid: [0-9.e+-]+", out), out
    assert re.search(r"check\s*: max\|diff\| vs serial cg = [0-9.eE+-]+ \(bound [0-9.eE+-]+\) OK", out), out
    j = json.loads(js.read_text().strip().splitlines()[-1])
    for k in ("solver", "iters", "residual_iters", "checks", "solve_ms", "r0", "residual_max", "true_residual"):
        assert k in j, j
    assert j["solver"] == "cg" and j["converged"] is True and j["iters"] == (c + 1) * 10, j
    assert j["residual_iters"] == c * 10 and j["checks"] == c + 2, j
    assert rel(j["r0"], ser[0][0]) <= 1e-8 and rel(j["residual"], ser[c * 10][0]) <= 1e-8, (j, ser[0])


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
def test_app_cg_cap_fixed_count_and_plain_run():
    """An unreachable --tol exits 4 at the (rounded-up) cap; --cg alone runs n_iter iterations; without --cg the
    app prints none of the new words."""
    p = run_app("mpi_jacobi2d", "64", "25", "--ny=60", "--init=random", "--cg", "--tol=1e-300", "--lag=2", np=2,
                check=False)
    assert p.returncode == 4, p.stdout + p.stderr
    assert "converged : no" in p.stdout and "rounded up to a multiple of 10" in p.stdout, p.stdout
    assert re.search(r"iters     : 30 \(criterion met at 30, 4 checks, lag 2\)", p.stdout), p.stdout
    f = run_app("mpi_jacobi2d", "64", "40", "--ny=60", "--init=random", "--cg", "--check", np=2)
    assert "solver    = cg" in f.stdout and re.search(r"iters     : 40 \(fixed count", f.stdout), f.stdout
    assert re.search(r"ms per iteration", f.stdout) and " OK" in f.stdout, f.stdout
    q = run_app("mpi_jacobi2d", "64", "30", "--ny=60", "--warmup=2", np=2)
    for word in ("solver", "converged", "iters", "TIME solve", "true resid", "cg"):
        assert word not in q.stdout, q.stdout
    bad = run_app("mpi_jacobi2d", "64", "30", "--ny=60", "--periodic", "--cg", np=1, check=False)
    assert bad.returncode != 0 and "periodic" in (bad.stdout + bad.stderr), bad.stdout + bad.stderr


def test_kernel_bench_cg_host():
    """gmt_kernel_bench --only=cg on the CPU backend: one line per kernel, each beside its DAXPY."""
    out = run_app("gmt_kernel_bench", "--only=cg", "--cg-n=64", "--iters=2", "--reps=1").stdout
    for k in ("cg_apply", "cg_update", "cg_dir"):
        assert len(re.findall(rf"^{k}\s+v0\s+64x64 best", out, re.M)) == 1, out
        assert re.search(rf"{k} GB/s / daxpy GB/s = [0-9.]+", out), out
    assert len(re.findall(r"^daxpy\s+v[123]", out, re.M)) == 3, out
