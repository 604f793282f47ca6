"""Multigrid on any lattice size on the GPU: the assertions of
tests/test_mg_any_cpu.py (field bitwise engine.serial_mg(coarsen="any") on every
process grid, level table, coarse iteration count and rho, residuals by fsum,
nu = (1, 1), max_levels = 3, decision for lag 0, 1 and 3, the cap, run() after
mg(), a second mg()) at 256 x 766 — y general once, x general on every level —
through the engine kinds whose buffers and transport mg() borrows: a plain
engine at one rank (ghost depth 1: the residual has its own buffer for the
2-wide ring), a tsteps = 20 engine at 1 x 2 replaying hipGraphs, an inline-halo
engine at 2 x 1, a 2 x 2 grid with overlap; and at 254 x 766, both axes general
on every level, on one rank.  Ranks share cuda:0 over IPC.  Every child runs
under `timeout`; once a child has failed nothing further runs on the GPU from
this file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import free_port
from gpu_mpi_tests_amd import _native
from test_mg_any_cpu import NX, NY, NY2, any_ops, check_short_any, check_standard_any, short_ops
from test_mg_cpu import standard_ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mg_worker.py")
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


@pytest.mark.parametrize("name,np_,cfg", [
    ("one rank plain", 1, dict(transport="local")),
    ("1x2 fused passes from graphs", 2, dict(dims=(1, 2), tsteps=20, graph=True)),
    ("2x1 inline halo", 2, dict(dims=(2, 1), tsteps=20, push=True)),
    ("2x2 overlap", 4, dict(dims=(2, 2), overlap=True)),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_mg_any_against_serial(name, np_, cfg, tmp_path):
    tsteps = cfg.get("tsteps", 1)
    out = str(tmp_path / "fields.npz")
    res = _launch(dict(cfg, ny=NY, nx=NX, ops=any_ops(standard_ops(tsteps)), out=out), np_)
    info = res[0]
    check_standard_any(res, dict(np.load(out)), NY, NX, cfg.get("dims") or (1, 1), None, tsteps, info["umax"])
    if cfg.get("push"):
        assert info["push"], info
    if cfg.get("graph"):
        assert info["graph_fused"], info


def test_mg_any_both_axes_general(tmp_path):
    out = str(tmp_path / "fields.npz")
    res = _launch(dict(transport="local", ny=NY2, nx=NX, ops=short_ops(), out=out), 1)
    check_short_any(res, dict(np.load(out)), NY2, NX, (1, 1))
