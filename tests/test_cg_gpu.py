"""Conjugate gradients of the native Jacobi engine on the GPU: the assertions of
tests/test_cg_cpu.py (series, decision, field, r0, true residual, fixed count,
cap, argument errors, the periodic refusal, run() after cg(), a second cg())
against engine.serial_cg, through the engine kinds whose buffers and transport
cg() borrows — a plain engine, a tsteps = 20 engine replaying hipGraphs (run()
before and after cg() still replays), an inline-halo engine at 2 ranks, a 2 x 2
grid.  Ranks share cuda:0 over IPC.  Every child runs under `timeout`; once a
child has failed nothing further runs on the GPU from this file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import free_port
from gpu_mpi_tests_amd import _native
from test_cg_cpu import check_standard, rel, standard_plan, sweeps_from, worst

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "cg_worker.py")
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
    """run() replays before and after a cg() that starts from a swept field."""
    return [dict(op="reset"), dict(op="run", k=2 * tsteps, tag="pre"), dict(op="rn"),
            dict(op="cg", tag="mid", kw=dict(max_iters=20, check_every=10, lag=0)),
            dict(op="run", k=2 * tsteps, tag="post")]


@pytest.mark.parametrize("name,np_,cfg,every,lo,series_every", [
    ("one rank plain", 1, dict(ny=300, nx=700, transport="local"), 10, 3, 20),
    ("1x2 fused passes from graphs", 2, dict(ny=300, nx=700, dims=(1, 2), tsteps=20, graph=True), 10, 3, 20),
    ("2x1 inline halo", 2, dict(ny=400, nx=900, dims=(2, 1), tsteps=20, push=True), 10, 2, None),
    ("2x2 overlap", 4, dict(ny=300, nx=700, dims=(2, 2), overlap=True), 10, 3, None),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_cg_against_serial(name, np_, cfg, every, lo, series_every, tmp_path):
    from gpu_mpi_tests_amd import engine

    ny, nx = cfg["ny"], cfg["nx"]
    # the 300 x 700 configurations share one reference run; the larger shape gets a shorter one
    n_ref = None if ny * nx <= 300 * 700 else (lo + 6) * every
    plan = standard_plan(ny, nx, every, lo, series_every=series_every, n_ref=n_ref)
    ops = plan["ops"] + (graph_ops(cfg["tsteps"]) if cfg.get("graph") else [])
    out = str(tmp_path / "fields.npz")
    res = _launch(dict(cfg, ops=ops, out=out), np_)
    fields = dict(np.load(out))
    check_standard(plan, res, fields, ny, nx)
    print("largest deviations on the GPU so far:", worst)
    info = res[0]
    if cfg.get("push"):
        assert info["push"], info
    if cfg.get("graph"):
        assert info["graph_fused"], info
        k = 2 * cfg["tsteps"]
        _, _, rn, mid, _ = res[1 + len(plan["ops"]):]
        assert np.array_equal(fields["pre"], engine.serial_jacobi(ny, nx, k, init="random", seed=11))  # replayed passes
        m = mid["res"]
        assert mid["same"] and m["iters"] == 20 and m["failed"] == 0 and m["residual"] < m["r0"], m
        assert rel(m["r0"], rn["rn"][0]) <= 1e-12 and abs(m["true_residual"] - m["residual"]) <= 1e-10 * m["r0"], (m, rn)
        want = sweeps_from(fields["mid"], ny, nx, "random", k)
        assert float(np.abs(fields["post"] - want).max()) <= 1e-10 * info["umax"]
