"""Red-black Gauss-Seidel smoothing of the multigrid cycle
(NativeJacobi.mg(smoother="rb")) on the CPU backend: tests/mg_rb_worker.py under
torch.distributed.run on the process grids 1x1, 1x2, 2x1, 2x2 and 3x2.

Field: after 2 cycles interior() is BITWISE engine.serial_mg(smoother="rb") —
every smoothing sweep reference.mg_smooth_rb(h=2, par=0) over the whole level —
on every grid, for fuse 0, 2, 3 and 4, nu (1, 1), (2, 1) and (0, 2), engines of
tsteps 1 and 4, with and without a source, nested (63 x 127) and
coarsen="any" (64 x 100).  The block split gives the larger share first, so on
1x2, 2x1 and 2x2 every rank of 63 x 127 starts on an even offset (32 rows, 64
columns); on 3x2 the shares are 21 rows and the second process row starts on
row 21, 64 x 100 gives it 22 + 21 + 21: ranks whose first cell is black, which
the test asserts are there.  r0 and the last residual are within 2e-13 relative of the
math.fsum residuals of the serial fields (the bound of tests/test_mg_cpu.py).

Convergence is a condition between two runs of the same engine: from the
analytic field at rtol = 1e-6, smoother="rb" with nu = (1, 1) stops in no more
cycles than smoother="jacobi" with nu = (2, 2), on 255 x 255 (nested) and on
256 x 256 (coarsen="any"), and both counts are serial_mg's."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import free_port
from mg_worker import SEED
from native_util import ROOT, ensure_host_build
from test_mg_cpu import close, same_bits

WORKER = os.path.join(ROOT, "tests", "mg_rb_worker.py")
CYCLES = 2
RTOL = 1e-6
CAP = 12
GRIDS = [(1, None), (2, (1, 2)), (2, (2, 1)), (4, (2, 2)), (6, (3, 2))]
FUSES = (0, 2, 3, 4)
NUS = ((1, 1), (2, 1), (0, 2))
LATTICES = ((63, 127, "nested"), (64, 100, "any"))


def launch_cpu(cfg, np_=1, transport="rccl"):
    ensure_host_build()
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    if np_ == 1:
        cmd = [sys.executable, WORKER, json.dumps(cfg)]
    else:
        env["GMT_TRANSPORT"] = transport
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(np_),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), WORKER, json.dumps(cfg)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("[")][-1])


@functools.lru_cache(maxsize=None)
def reference(ny, nx, cycles, source, nu, max_levels, coarsen, smoother="rb", init="random", omega=None):
    """engine.serial_mg once per argument set, never modified: (field after `cycles`, residual series)."""
    from gpu_mpi_tests_amd import engine

    return engine.serial_mg(ny, nx, cycles, init=init, seed=SEED, source=source, nu=nu, max_levels=max_levels,
                            coarsen=coarsen, smoother=smoother, omega=omega)


def engine_entries(fuses=FUSES, nus=NUS, tsteps_all=(1, 4), sources=(None, "random"), lattices=LATTICES):
    """The engines of one launch and, per mg op, what it ran: tag -> (ny, nx, coarsen, source, nu, fuse, tsteps)."""
    engines, what = [], {}
    for ny, nx, coarsen in lattices:
        for tsteps in tsteps_all:
            for source in sources:
                ops = []
                for fuse in fuses:
                    for nu in nus:
                        tag = f"{ny}_{tsteps}_{source}_{fuse}_{nu[0]}{nu[1]}"
                        ops.append(dict(op="mg", tag=tag, kw=dict(max_cycles=CYCLES, nu=nu, fuse=fuse, coarsen=coarsen,
                                                                   smoother="rb")))
                        what[tag] = (ny, nx, coarsen, source, nu, fuse, tsteps)
                engines.append(dict(ny=ny, nx=nx, tsteps=tsteps, source=source, ops=ops))
    return engines, what


def check_against_serial(res, fields, engines, what, dims):
    from gpu_mpi_tests_amd import engine

    for ec, rs in zip(engines, res):
        for op, r in zip(ec["ops"], rs["ops"]):
            tag = op["tag"]
            ny, nx, coarsen, source, nu, fuse, tsteps = what[tag]
            nlev = len(engine.mg_levels(ny, nx, dims, 0, coarsen))
            want, ser = reference(ny, nx, CYCLES, source, nu, nlev, coarsen)
            got = r["res"]
            assert r["same"] and got["iters"] == CYCLES and got["levels"] == nlev and not got["failed"], (tag, got)
            assert got["smoother"] == "rb" and got["omega"] == 1.0 and got["fuse"] == fuse, (tag, got)
            depths = engine.mg_fuse_depths(ny, nx, dims, fuse, tsteps, 0, coarsen)
            assert (got["fuse_fine"], got["fuse_levels"]) == (depths[0], sum(d >= 2 for d in depths)), (tag, got, depths)
            if not same_bits(fields[tag], want):
                bad = np.argwhere(fields[tag].view(np.int64) != want.view(np.int64))
                raise AssertionError((tag, dims, "cells (row, column) that differ", len(bad), bad[:8].tolist()))
            assert close(got["r0"], ser[0][0]) and close(got["residual"], ser[CYCLES][0]), (tag, got, ser)
            assert close(got["residual_max"], ser[CYCLES][1]), (tag, got, ser)


@pytest.mark.parametrize("np_,dims", GRIDS, ids=lambda v: None if isinstance(v, int) else str(v))
def test_rb_cycle_is_serial_mg(np_, dims, tmp_path):
    out = str(tmp_path / "fields.npz")
    engines, what = engine_entries()
    res = launch_cpu(dict(dims=dims, engines=engines, out=out), np_, "ipc" if dims == (2, 1) else "rccl")
    check_against_serial(res, dict(np.load(out)), engines, what, dims or (1, 1))
    if dims == (3, 2):  # ranks whose first cell is black: par = 1 on the fine level
        for ec, rs in zip(engines, res):
            assert any((oy + ox) % 2 for oy, ox in rs["offsets"]), (ec["ny"], ec["nx"], rs["offsets"])


def deciding_cycle(series):
    """The first cycle whose L2 residual meets RTOL, with every value of the series clear of the threshold."""
    thr = RTOL * series[0][0]
    c = next(i for i, (r, _) in enumerate(series) if r <= thr)
    assert all(abs(r - thr) > 0.01 * thr for r, _ in series), (thr, series)
    return c


@pytest.mark.parametrize("ny,nx,coarsen", [(255, 255, "nested"), (256, 256, "any")])
def test_rb_v11_needs_no_more_cycles_than_jacobi_v22(ny, nx, coarsen):
    """The issue's NumPy probe gives 7 cycles against 9 on both lattices."""
    kw = dict(rtol=RTOL, max_cycles=CAP, lag=0, coarsen=coarsen)
    ops = [dict(op="mg", kw=dict(kw, smoother="rb", nu=(1, 1))), dict(op="mg", kw=dict(kw, smoother="jacobi", nu=(2, 2))),
           dict(op="mg", kw=dict(kw, smoother="rb", nu=(1, 1), fuse=2))]
    res = launch_cpu(dict(engines=[dict(ny=ny, nx=nx, init="analytic", ops=ops)]))[0]["ops"]
    rb, jac, rbf = (r["res"] for r in res)
    for r in (rb, jac, rbf):
        assert r["converged"] == 1 and not r["failed"], r
    print("cycles to rtol 1e-6:", (ny, nx, coarsen), "rb V(1,1)", rb["iters"], "jacobi V(2,2)", jac["iters"])
    assert rb["iters"] <= jac["iters"], (rb, jac)
    assert rbf["iters"] == rb["iters"] and rbf["residual"] == rb["residual"], (rb, rbf)
    # the counts are the definition's
    _, ser_rb = reference(ny, nx, CAP, None, (1, 1), 0, coarsen, "rb", "analytic")
    _, ser_j = reference(ny, nx, CAP, None, (2, 2), 0, coarsen, "jacobi", "analytic")
    assert rb["iters"] == deciding_cycle(ser_rb) and jac["iters"] == deciding_cycle(ser_j), (rb, jac, ser_rb, ser_j)


def test_defaults_and_refusals(tmp_path):
    from gpu_mpi_tests_amd import engine

    ny, nx = 63, 127
    out = str(tmp_path / "fields.npz")
    bad = [dict(max_cycles=2, smoother="gs"), dict(max_cycles=2, smoother=1), dict(max_cycles=2, smoother=None),
           dict(max_cycles=2, smoother="rb", omega=0.0), dict(max_cycles=2, smoother="rb", omega=1.5)]
    ops = [dict(op="mg", tag="plain", kw=dict(max_cycles=CYCLES)),
           dict(op="mg", tag="jac", kw=dict(max_cycles=CYCLES, smoother="jacobi")),
           dict(op="mg", tag="rb", kw=dict(max_cycles=CYCLES, smoother="rb")),
           dict(op="mg", tag="rb08", kw=dict(max_cycles=CYCLES, smoother="rb", omega=0.8, fuse=3)),
           dict(op="bad", kws=bad), dict(op="capi", smoother=2), dict(op="capi", smoother=-1),
           dict(op="capi", smoother=1), dict(op="capi", smoother=0)]
    for np_, dims in ((1, None), (2, (1, 2))):
        res = launch_cpu(dict(dims=dims, engines=[dict(ny=ny, nx=nx, ops=ops)], out=out), np_)[0]["ops"]
        fields = dict(np.load(out))
        plain, jac, rb, rb08 = (r["res"] for r in res[:4])
        assert (plain["smoother"], plain["omega"]) == ("jacobi", 0.8) and (jac["smoother"], jac["omega"]) == ("jacobi", 0.8)
        assert (rb["smoother"], rb["omega"]) == ("rb", 1.0) and (rb08["smoother"], rb08["omega"]) == ("rb", 0.8)
        assert res[4] == [True] * len(bad), res[4]
        assert res[5:] == [1, 1, 0, 0], res[5:]  # the C ABI: smoother outside {0, 1} is code 1
        # mg() without smoother is today's serial_mg, called as before
        want, _ = engine.serial_mg(ny, nx, CYCLES, init="random", seed=SEED)
        assert same_bits(fields["plain"], want) and same_bits(fields["jac"], want)
        assert same_bits(fields["rb"], reference(ny, nx, CYCLES, None, (2, 2), 0, "nested")[0])
        assert same_bits(fields["rb08"], reference(ny, nx, CYCLES, None, (2, 2), 0, "nested", "rb", "random", 0.8)[0])
        assert not same_bits(fields["rb"], want)
    with pytest.raises(ValueError):
        engine.serial_mg(ny, nx, 1, smoother="gs")
