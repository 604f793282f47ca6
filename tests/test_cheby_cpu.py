"""Chebyshev semi-iteration of the native Jacobi engine on the CPU backend
(JacobiSolver::cheby, NativeJacobi.cheby) against the NumPy definition
engine.serial_cheby, on 1, 2 and 4 ranks over the host emulations of RCCL and
IPC (tests/cheby_worker.py under torch.distributed.run).

Field: after n iterations interior() is BITWISE serial_cheby(n, rho=result["rho"])
on every process grid (every rank's share is gathered), for fixed counts, for
the decision cases, for a supplied rho, and for a second call (a serial
restart).  result["rho"] agrees with engine.cheby_rho within 1e-15 relative (two
cos implementations may differ by an ulp); a supplied rho comes back bit for bit.
Residuals (r0, the series, the deciding residual): within 1e-11 * max(1, value)
of the math.fsum residuals of the serial fields, the tolerance
tests/test_solve_cpu.py uses for the same kernel.
Decision: rtol is chosen by cheby_worker.pick_rtol so that the reference first
meets it at a check c with every checked value at least 2.5% away, so
residual_iters, iters, checks and the final field are fixed numbers, on every
rank alike, for lag 0, 1 and 3.  At 300 x 700 the max-norm series is not
monotone at check_every = 10 and L2 ratios reach 0.985: that shape uses the L2
norm and the picker's choice of c.
run(k) after cheby(): bitwise NumPy sweeps from the field for a tsteps = 1
engine (from an even and an odd iteration count), within 1e-10 * max|u0| (the
bound tests/test_cg_gpu.py uses) for fused passes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cheby_worker import SEED, pick_rtol, reference
from conftest import free_port
from native_util import ROOT, ensure_host_build

WORKER = os.path.join(ROOT, "tests", "cheby_worker.py")
N_FIXED = 120
SPECS = [(0, "l2"), (1, "max"), (3, "l2")]     # (lag, norm) of the decision cases
SPECS_L2 = [(0, "l2"), (1, "l2"), (3, "l2")]   # 300 x 700 and larger
RUN_AFTER = 7
ODD = 21
RHO_GIVEN = 0.9
BAD = [dict(rtol=1e-3, max_iters=0), dict(rtol=1e-3, max_iters=25, check_every=10), dict(rtol=1e-3, max_iters=-10),
       dict(rtol=1e-3, max_iters=20, check_every=-1), dict(rtol=1e-3, max_iters=20, lag=-1),
       dict(rtol=1e-3, max_iters=20, lag=9), dict(tol=-1.0, max_iters=20), dict(rtol=-1e-3, max_iters=20),
       dict(rtol=float("nan"), max_iters=20), dict(tol=float("inf"), max_iters=20),
       dict(rtol=1e-3, max_iters=20, norm="l1"), dict(max_iters=20, rho=1.0), dict(max_iters=20, rho=-0.5),
       dict(max_iters=20, rho=1.5), dict(max_iters=20, rho=float("nan")), dict(max_iters=20, rho=float("inf"))]
worst = {"series": 0.0, "r0": 0.0, "deciding": 0.0}  # the largest residual deviations seen, over max(1, value)


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


def dev(got, want):
    return abs(got - want) / max(1.0, abs(want))


def same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                                      np.ascontiguousarray(b).view(np.int64)))


def standard_plan(ny, nx, every, lo, init="random", series=False, specs=SPECS):
    """The ops of one worker run and what the reference says about them.  One reference run (the closed-form
    rho) serves the series, the picks and the fields; configurations of one shape share it."""
    from gpu_mpi_tests_amd import engine

    rho = engine.cheby_rho(ny, nx)
    n = N_FIXED
    while True:
        _, ser = reference(ny, nx, n, every, rho, init)
        try:
            picks = [pick_rtol(ser, every, lo + i, norm) for i, (_, norm) in enumerate(specs)]
            if all((c + lag) * every <= n for (lag, _), (c, _) in zip(specs, picks)):
                break
        except AssertionError:
            pass
        n += 10 * every
        assert n <= 400, "no decidable check in 400 iterations"
    ops = [dict(op="rn")]
    if series:
        ops.append(dict(op="series", every=every, upto=N_FIXED))
    for i, ((lag, norm), (c, rtol)) in enumerate(zip(specs, picks)):
        ops += [dict(op="reset"), dict(op="cheby", tag=f"d{i}", kw=dict(rtol=rtol, norm=norm, lag=lag, check_every=every,
                                                                       max_iters=(c + lag + 2) * every))]
    ops += [
        # a fixed count (even), then sweeps from it
        dict(op="reset"), dict(op="cheby", tag="fixed", kw=dict(max_iters=N_FIXED, check_every=every)),
        dict(op="run", k=RUN_AFTER, tag="run_even"),
        # an odd count, then sweeps from it
        dict(op="reset"), dict(op="cheby", tag="odd", kw=dict(max_iters=ODD, check_every=ODD, lag=0)),
        dict(op="run", k=RUN_AFTER, tag="run_odd"),
        # a second call restarts the recurrence
        dict(op="reset"), dict(op="cheby", kw=dict(max_iters=2 * every, check_every=every)),
        dict(op="cheby", tag="again", kw=dict(max_iters=2 * every, check_every=every)),
        # the cap, a tolerance met by the starting field, a supplied rho
        dict(op="reset"), dict(op="cheby", kw=dict(rtol=1e-30, max_iters=2 * every, check_every=every, lag=1)),
        dict(op="reset"), dict(op="cheby", kw=dict(tol=1e300, max_iters=4 * every, check_every=every, lag=2)),
        dict(op="reset"), dict(op="cheby", tag="rho", kw=dict(max_iters=2 * every, check_every=every, rho=RHO_GIVEN)),
        dict(op="bad", kws=BAD), dict(op="periodic")]
    return dict(ops=ops, picks=picks, n=n, rho=rho, every=every, series=series, specs=specs, init=init)


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


def check_standard(plan, results, got, ny, nx):
    every, init, n = plan["every"], plan["init"], plan["n"]
    info, results = results[0], results[1:]
    umax = info["umax"]
    it = iter(zip(plan["ops"], results))
    nxt = lambda kind: next(r for o, r in it if o["op"] == kind)  # noqa: E731
    rn0 = nxt("rn")
    assert rn0["same"]
    # the rho the engine used: the closed form within an ulp or so; the references take it as an argument
    first = next(r for o, r in zip(plan["ops"], results) if o["op"] == "cheby")
    rho = first["res"]["rho"]
    assert abs(rho - plan["rho"]) <= 1e-15 * plan["rho"], (rho, plan["rho"])
    fields, ser = reference(ny, nx, n, every, rho, init)
    for g, w in zip(rn0["rn"], ser[0]):
        worst["r0"] = max(worst["r0"], dev(g, w))
        assert dev(g, w) <= 1e-11, (rn0, ser[0])
    if plan["series"]:
        s = nxt("series")
        assert s["same"]
        for i, (r2, rm, r0) in enumerate(s["series"]):
            k = (i + 1) * every
            d = max(dev(r2, ser[k][0]), dev(rm, ser[k][1]))
            worst["series"] = max(worst["series"], d)
            assert d <= 1e-11, (k, r2, rm, ser[k])
            assert r0 == rn0["rn"][0]
    for i, ((lag, norm), (c, rtol)) in enumerate(zip(plan["specs"], plan["picks"])):
        g = nxt("cheby")
        res = g["res"]
        kn = 0 if norm == "l2" else 1
        assert g["same"], g
        assert res["rho"] == rho
        assert (res["converged"], res["failed"]) == (1, 0), res
        assert res["residual_iters"] == c * every and res["iters"] == (c + lag) * every, (res, c, lag)
        assert res["checks"] == c + lag + 1, res
        d = max(dev(res["residual"], ser[c * every][kn]), dev(res["residual_max"], ser[c * every][1]))
        worst["deciding"] = max(worst["deciding"], d)
        assert d <= 1e-11, (res, ser[c * every])
        assert res["r0"] == rn0["rn"][kn], (res, rn0)  # the residual of the starting field
        assert same_bits(got[f"d{i}"], fields[res["iters"]]), i
    bound = 1e-10 * umax

    def check_run(tag, start):
        want = sweeps_from(got[start], ny, nx, init, RUN_AFTER)
        if info["tsteps"] == 1:
            assert same_bits(got[tag], want), tag
        else:
            assert float(np.abs(got[tag] - want).max()) <= bound, tag

    fixed = nxt("cheby")["res"]
    assert (fixed["converged"], fixed["failed"], fixed["iters"], fixed["residual_iters"], fixed["checks"]) == \
        (0, 0, N_FIXED, N_FIXED, N_FIXED // every + 1), fixed
    assert dev(fixed["residual"], ser[N_FIXED][0]) <= 1e-11 and dev(fixed["residual_max"], ser[N_FIXED][1]) <= 1e-11
    assert same_bits(got["fixed"], fields[N_FIXED])
    check_run("run_even", "fixed")
    odd = nxt("cheby")["res"]
    assert (odd["iters"], odd["checks"], odd["converged"]) == (ODD, 2, 0), odd
    assert same_bits(got["odd"], reference(ny, nx, ODD, ODD, rho, init)[0][ODD])
    check_run("run_odd", "odd")
    nxt("cheby")
    again = nxt("cheby")["res"]
    assert again["iters"] == 2 * every and again["failed"] == 0, again
    assert same_bits(got["again"], reference(ny, nx, 4 * every, every, rho, init, None, 2 * every)[0][4 * every])
    cap = nxt("cheby")["res"]
    assert (cap["converged"], cap["failed"], cap["iters"], cap["residual_iters"], cap["checks"]) == \
        (0, 0, 2 * every, 2 * every, 3), cap
    met = nxt("cheby")["res"]
    assert (met["converged"], met["failed"], met["iters"], met["residual_iters"], met["checks"]) == \
        (1, 0, 2 * every, 0, 3), met
    assert met["residual"] == met["r0"] == rn0["rn"][0], (met, rn0)
    given = nxt("cheby")["res"]
    assert given["rho"] == RHO_GIVEN, given  # bit for bit
    assert same_bits(got["rho"], reference(ny, nx, 2 * every, every, RHO_GIVEN, init)[0][2 * every])
    assert nxt("bad") == [True] * len(BAD)
    assert nxt("periodic") is True
    print("largest residual deviations so far:", worst)


_cache = {}


def standard_cpu(name, tmp_path_factory):
    """One worker run per configuration."""
    if name not in _cache:
        np_, transport, ny, nx, dims, kind, lo, series, specs = CONFIGS[name]
        plan = standard_plan(ny, nx, 10, lo, series=series, specs=specs)
        out = str(tmp_path_factory.mktemp("cheby") / "fields.npz")
        res = launch_cpu(dict(kind, ny=ny, nx=nx, dims=dims, ops=plan["ops"], out=out), np_, transport)
        _cache[name] = (plan, res, dict(np.load(out)))
    return _cache[name]


# name -> ranks, transport, ny, nx, dims, engine kind, first candidate check, series too, (lag, norm) specs
CONFIGS = {
    "60x64 1": (1, "rccl", 60, 64, None, {}, 3, True, SPECS),
    "60x64 1x2 rccl": (2, "rccl", 60, 64, (1, 2), {}, 3, False, SPECS),
    "60x64 2x1 ipc": (2, "ipc", 60, 64, (2, 1), {}, 3, True, SPECS),
    "60x64 2x2 rccl": (4, "rccl", 60, 64, (2, 2), {}, 3, False, SPECS),
    "300x700 1": (1, "rccl", 300, 700, None, {}, 3, True, SPECS_L2),
    "300x700 1x2 rccl fused": (2, "rccl", 300, 700, (1, 2), dict(tsteps=20, graph=True), 3, False, SPECS_L2),
    "400x900 2x1 ipc inline halo": (2, "ipc", 400, 900, (2, 1), dict(tsteps=20, push=True), 3, False, SPECS_L2),
    "300x700 2x2 ipc overlap": (4, "ipc", 300, 700, (2, 2), dict(overlap=True), 3, False, SPECS_L2),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_cheby_against_serial(name, tmp_path_factory):
    plan, res, fields = standard_cpu(name, tmp_path_factory)
    np_, transport, ny, nx = CONFIGS[name][:4]
    if np_ > 1:
        assert res[0]["transport"] == f"{transport}-host", res[0]
    check_standard(plan, res, fields, ny, nx)


def test_analytic_init():
    """The analytic initial field on a 1 x 2 grid: fixed count bitwise, and a decision."""
    from gpu_mpi_tests_amd import engine

    ny, nx, every = 60, 64, 10
    rho = engine.cheby_rho(ny, nx)
    _, ser = reference(ny, nx, N_FIXED, every, rho, "analytic")
    c, rtol = pick_rtol(ser, every, 3)
    res = launch_cpu(dict(ny=ny, nx=nx, dims=(1, 2), init="analytic", ops=[
        dict(op="cheby", kw=dict(rtol=rtol, lag=1, check_every=every, max_iters=(c + 3) * every))]), 2, "rccl")
    r = res[1]["res"]
    assert res[1]["same"] and (r["converged"], r["residual_iters"], r["iters"], r["checks"]) == \
        (1, c * every, (c + 1) * every, c + 2), (r, c)


@pytest.mark.parametrize("np_,dims,init,source", [(1, None, "analytic", "poly"), (2, (2, 1), "random", "poly"),
                                                  (1, None, "random", "random"), (4, (2, 2), "analytic", "random")])
def test_sources(np_, dims, init, source, tmp_path):
    """The poly and random sources (the kernel's f instantiation): field bitwise, r0 and the residual by fsum."""
    out = str(tmp_path / "f.npz")
    res = launch_cpu(dict(ny=60, nx=64, dims=dims, init=init, source=source, out=out, ops=[
        dict(op="cheby", tag="f", kw=dict(max_iters=40, check_every=10, lag=1))]), np_, "ipc")
    r = res[1]["res"]
    fields, ser = reference(60, 64, 40, 10, r["rho"], init, source)
    assert res[1]["same"] and r["iters"] == 40 and r["failed"] == 0, r
    assert same_bits(np.load(out)["f"], fields[40])
    assert dev(r["r0"], ser[0][0]) <= 1e-11 and dev(r["residual"], ser[40][0]) <= 1e-11, (r, ser[0], ser[40])
    assert dev(r["residual_max"], ser[40][1]) <= 1e-11
    worst["deciding"] = max(worst["deciding"], dev(r["residual"], ser[40][0]))
    print("largest residual deviations so far:", worst)


def test_converges_faster_than_sweeps():
    """60 x 64 with a random source: 200 Chebyshev iterations leave a residual at least 100x smaller than 200
    plain sweeps from the same field (NumPy: 6.3e-5 of r0 against 3.4e-2)."""
    res = launch_cpu(dict(ny=60, nx=64, source="random", ops=[
        dict(op="cheby", kw=dict(max_iters=200, check_every=200, lag=0)), dict(op="reset"),
        dict(op="run", k=200), dict(op="rn")]))
    ch, sw = res[1]["res"], res[4]["rn"][0]
    print("cheby", ch["residual"] / ch["r0"], "sweeps", sw / ch["r0"])
    assert ch["iters"] == 200 and 100.0 * ch["residual"] <= sw, (ch, sw)


def test_serial_cheby_and_weights():
    """The NumPy definition itself: weights in the documented order, keep / resid_every / restart_every,
    iteration 1 is one plain sweep, and an under-estimated rho stagnates where the exact one converges."""
    from gpu_mpi_tests_amd import engine

    rho = engine.cheby_rho(60, 64)
    assert 0.0 < rho < 1.0 and rho == engine.cheby_rho(64, 60)
    w = engine.cheby_weights(rho, 50)
    assert w[0] == 1.0 and w[1] == 1.0 / (1.0 - 0.5 * (rho * rho)) and w[2] == 1.0 / (1.0 - 0.25 * (rho * rho) * w[1])
    assert all(1.0 <= a < 2.0 for a in w) and all(b <= a for a, b in zip(w[1:], w[2:]))
    one, _ = engine.serial_cheby(60, 64, 1, rho, init="random", seed=SEED)
    assert np.array_equal(one, engine.serial_jacobi(60, 64, 1, init="random", seed=SEED))
    kept, ser = engine.serial_cheby(60, 64, 30, rho, init="random", seed=SEED, keep=(0, 10, 30), resid_every=10)
    assert sorted(kept) == [0, 10, 30] and sorted(ser) == [0, 10, 20, 30]
    assert np.array_equal(kept[10], engine.serial_cheby(60, 64, 10, rho, init="random", seed=SEED)[0])
    again, _ = engine.serial_cheby(60, 64, 20, rho, init="random", seed=SEED, restart_every=10)
    assert not np.array_equal(again, engine.serial_cheby(60, 64, 20, rho, init="random", seed=SEED)[0])
    _, exact = engine.serial_cheby(60, 64, 200, rho, init="random", seed=SEED, source="random", resid_every=200)
    _, under = engine.serial_cheby(60, 64, 200, 0.98 * rho, init="random", seed=SEED, source="random",
                                   resid_every=200)
    assert exact[200][0] < 2e-4 * exact[0][0] and under[200][0] > 1e-3 * under[0][0], (exact, under)
