"""residual_norm and solve-to-tolerance of the native Jacobi engine on the GPU:
the assertions of tests/test_solve_cpu.py (read-only, repeatable residual
equal to NumPy's; the deciding check, sweeps, checks and the final field of a
solve fixed by a tolerance the NumPy reference first meets at a chosen check;
the same result on every rank) through the pass kinds the solve drives —
serial exchange, band-first, inline halo, hipGraph replay.  check_every is a
multiple of tsteps everywhere, so the captured graphs replay between checks.
Ranks share cuda:0 over IPC.  Once a child has failed nothing further runs on
the GPU from this file."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import free_port
from gpu_mpi_tests_amd import _native
from test_solve_cpu import check_case, check_residual_norm, solve_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "solve_worker.py")
SPECS = [(4, 1, "l2"), (5, 3, "max")]
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
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def _check(r, cfg, specs, cases, every):
    ny, nx, periodic = cfg["ny"], cfg["nx"], bool(cfg.get("periodic", False))
    check_residual_norm(r, ny, nx, periodic, cfg["pre"][0])
    for (c, _, _), case, got in zip(specs, cases, r["cases"]):
        check_case(case, got, ny, nx, periodic, every, c)


@pytest.mark.parametrize("name,np_,cfg,every,specs", [
    ("one rank, local", 1, dict(ny=300, nx=700, tsteps=12, transport="local"), 12, SPECS),
    ("one rank, periodic, inline halo from graphs", 1,
     dict(ny=300, nx=700, tsteps=20, periodic=True, push=True, graph=True, transport="local"), 20, SPECS),
    ("2x1 periodic inline halo", 2, dict(ny=400, nx=900, tsteps=20, dims=(2, 1), periodic=True, push=True), 20, SPECS),
    ("2x1 periodic inline halo, lag 0", 2, dict(ny=400, nx=900, tsteps=20, dims=(2, 1), periodic=True, push=True),
     20, [(4, 0, "l2")]),
    ("1x2 Dirichlet serial exchange from graphs", 2, dict(ny=300, nx=1200, tsteps=12, dims=(1, 2), graph=True), 12,
     SPECS),
    ("2x2 band-first", 4, dict(ny=600, nx=1100, tsteps=20, dims=(2, 2), overlap=True), 20, SPECS),
], ids=lambda v: v.replace(" ", "_").replace(",", "") if isinstance(v, str) else None)
def test_solve_and_residual_norm(name, np_, cfg, every, specs):
    periodic = bool(cfg.get("periodic", False))
    cases = solve_cases(cfg["ny"], cfg["nx"], periodic, every, specs)
    cfg = dict(cfg, pre=(cfg["tsteps"] + 3, 9), cases=cases)
    r = _launch(cfg, np_)
    _check(r, cfg, specs, cases, every)
    if cfg.get("push"):
        assert r["push"], r
    if cfg.get("push") and cfg.get("graph"):
        assert r["graph_fused"], r
