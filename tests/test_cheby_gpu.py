"""Chebyshev semi-iteration of the native Jacobi engine on the GPU: the assertions
of tests/test_cheby_cpu.py (field bitwise engine.serial_cheby on every process
grid, rho, residual series by fsum, decision for lag 0, 1 and 3, fixed count of
120 iterations, the cap, a tolerance met at check 0, a supplied rho, argument
errors, the periodic refusal, run() after cheby() from an even and an odd count,
a second cheby()) through the engine kinds whose buffers and transport cheby()
borrows — a plain engine at 300 x 700 (across the 512-column workgroup seam), a
tsteps = 20 engine replaying hipGraphs (run() before and after cheby() still
replays), an inline-halo engine at 2 ranks, a 2 x 2 grid with overlap.  Ranks
share cuda:0 over IPC.  Every child runs under `timeout`; once a child has
failed nothing further runs on the GPU from this file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cheby_worker import reference
from conftest import free_port
from gpu_mpi_tests_amd import _native
from test_cheby_cpu import SPECS_L2, check_standard, same_bits, standard_plan, sweeps_from, worst

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "cheby_worker.py")
_failed = []


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _launch(cfg, np_):
    if _failed:
        pytest.fail(f"not run: an earlier child failed ({_failed[0]})")
    if np_ == 1:
        cmd = ["timeout", "-k", "10", "150", sys.executable, WORKER, json.dumps(cfg)]
    else:
        cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               "--nproc-per-node", str(np_), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
               WORKER, json.dumps(cfg)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd=ROOT,
                       env=dict(os.environ, OMP_NUM_THREADS="1", GMT_TRANSPORT="ipc", GMT_TEST_DEVICE="cuda"))
    if p.returncode != 0:
        _failed.append(f"rc={p.returncode}")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("[")][-1])


def graph_ops(tsteps):
    """run() replays before and after a cheby() that starts from a swept field."""
    return [dict(op="reset"), dict(op="run", k=2 * tsteps, tag="pre"), dict(op="rn"),
            dict(op="cheby", tag="mid", kw=dict(max_iters=20, check_every=10, lag=0)),
            dict(op="run", k=2 * tsteps, tag="post")]


@pytest.mark.parametrize("name,np_,cfg,series", [
    ("one rank plain", 1, dict(ny=300, nx=700, transport="local"), True),
    ("1x2 fused passes from graphs", 2, dict(ny=300, nx=700, dims=(1, 2), tsteps=20, graph=True), True),
    ("2x1 inline halo", 2, dict(ny=400, nx=900, dims=(2, 1), tsteps=20, push=True), False),
    ("2x2 overlap", 4, dict(ny=300, nx=700, dims=(2, 2), overlap=True), False),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_cheby_against_serial(name, np_, cfg, series, tmp_path):
    from gpu_mpi_tests_amd import engine

    ny, nx = cfg["ny"], cfg["nx"]
    plan = standard_plan(ny, nx, 10, 3, series=series, specs=SPECS_L2)
    ops = plan["ops"] + (graph_ops(cfg["tsteps"]) if cfg.get("graph") else [])
    out = str(tmp_path / "fields.npz")
    res = _launch(dict(cfg, ops=ops, out=out), np_)
    fields = dict(np.load(out))
    check_standard(plan, res, fields, ny, nx)
    print("largest residual deviations on the GPU so far:", worst)
    info = res[0]
    if cfg.get("push"):
        assert info["push"], info
    if cfg.get("graph"):
        assert info["graph_fused"], info
        k = 2 * cfg["tsteps"]
        _, _, rn, mid, _ = res[1 + len(plan["ops"]):]
        assert np.array_equal(fields["pre"], engine.serial_jacobi(ny, nx, k, init="random", seed=11))  # replayed passes
        m = mid["res"]
        assert mid["same"] and m["iters"] == 20 and m["failed"] == 0 and m["r0"] == rn["rn"][0], (m, rn)
        # 20 iterations from the swept field: the serial step applied to it
        u = engine.initial_field(ny, nx, "random", 11)
        v = u.copy()
        u[1:-1, 1:-1] = fields["pre"]
        for i, w in enumerate(engine.cheby_weights(m["rho"], 20)):
            o = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1]))
            if i == 0:
                v[1:-1, 1:-1] = o
            else:
                pv = v[1:-1, 1:-1]
                t = o - pv
                v[1:-1, 1:-1] = pv + w * t
            u, v = v, u
        assert same_bits(fields["mid"], u[1:-1, 1:-1])
        want = sweeps_from(fields["mid"], ny, nx, "random", k)
        assert float(np.abs(fields["post"] - want).max()) <= 1e-10 * info["umax"]


@pytest.mark.parametrize("np_,dims,init,source", [(1, None, "analytic", "poly"), (2, (1, 2), "random", "random")])
def test_sources(np_, dims, init, source, tmp_path):
    """The kernel's f instantiation through the engine, at 300 x 700: field bitwise, residuals by fsum."""
    out = str(tmp_path / "f.npz")
    res = _launch(dict(ny=300, nx=700, dims=dims, init=init, source=source, out=out, ops=[
        dict(op="cheby", tag="f", kw=dict(max_iters=40, check_every=10, lag=1))]), np_)
    r = res[1]["res"]
    fields, ser = reference(300, 700, 40, 10, r["rho"], init, source)
    assert res[1]["same"] and r["iters"] == 40 and r["failed"] == 0, r
    assert same_bits(np.load(out)["f"], fields[40])
    for got, want in ((r["r0"], ser[0][0]), (r["residual"], ser[40][0]), (r["residual_max"], ser[40][1])):
        print("residual deviation:", abs(got - want) / max(1.0, abs(want)))
        assert abs(got - want) <= 1e-11 * max(1.0, abs(want)), (r, ser[0], ser[40])
