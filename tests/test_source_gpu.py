"""The Poisson source term of the native Jacobi engine on the GPU
(JacobiConfig::source): the assertions of tests/test_source_cpu.py through the
pass kinds a source block drives — serial exchange, band-first, inline halo,
hipGraph replay — each followed by the add of the block field (gmt_add2d).
Single source sweeps are bitwise the float64 NumPy sweeps (graphs included);
fused blocks are bitwise independent of the decomposition and within the
derived rounding bound of long double single sweeps (tests/source_cases.py).
Ranks share cuda:0 over IPC.  Once a child has failed nothing further runs on
the GPU from this file."""
import json
import os
import subprocess
import sys

import pytest
import torch

import source_cases as sc
from conftest import free_port
from gpu_mpi_tests_amd import _native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "source_worker.py")
_failed = []


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _launch(jobs, np_=1):
    if _failed:
        pytest.fail(f"not run: an earlier child failed ({_failed[0]})")
    if np_ == 1:
        cmd = ["timeout", "-k", "10", "150", sys.executable, WORKER, json.dumps(jobs)]
    else:
        cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               "--nproc-per-node", str(np_), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
               WORKER, json.dumps(jobs)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd=ROOT,
                       env=dict(os.environ, OMP_NUM_THREADS="1", GMT_TRANSPORT="ipc", GMT_TEST_DEVICE="cuda"))
    if p.returncode != 0:
        _failed.append(f"rc={p.returncode}")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("[")][-1])


def test_single_sweep_source_path(tmp_path):
    """C: one rank, 40 x 70, 7 sweeps, Dirichlet and periodic, overlap on (core and frame) and off, eager and from graphs."""
    jobs = [dict(sc.SINGLE, periodic=p, overlap=o, graph=g, save=str(tmp_path / f"s{int(p)}{int(o)}{int(g)}"))
            for p in (False, True) for o in (False, True) for g in (False, True)]
    res = _launch(jobs)
    for job, r in zip(jobs, res):
        assert r["graph"] == job["graph"], r  # the single-sweep graphs captured the source pointer
        assert r["source_plan"] == dict(blocks=0, src_every=0, tail=7), r
        sc.check_single(job, job["save"])


@pytest.mark.parametrize("name,np_,cfg", sc.FUSED,
                         ids=lambda v: v.replace(" ", "_").replace(",", "") if isinstance(v, str) else None)
def test_fused_source_path(name, np_, cfg, tmp_path):
    """D: every configuration with src_every = tsteps and 2 * tsteps, two blocks and three single sweeps."""
    prefix, base = str(tmp_path / "f"), str(tmp_path / "b")
    res = _launch(sc.fused_jobs(cfg, prefix), np_)
    _launch(sc.baseline_jobs(cfg, base))
    sc.check_fused(cfg, res, prefix, base, gpu=True)


def test_fixed_point(tmp_path):
    """E: x^3 + y^2 with the poly source, Dirichlet."""
    job = dict(ny=sc.N_CONV, nx=sc.N_CONV, tsteps=4, src_every=20, kind="run", sweeps=60, init="analytic",
               source="poly", resid0=True, transport="local", save=str(tmp_path / "p"))
    (r,) = _launch([job])
    sc.check_fixed_point(r, job["save"], 60, 20)


@pytest.mark.parametrize("np_,cfg,every", [
    (1, dict(ny=300, nx=700, tsteps=20, periodic=True, push=True, graph=True, transport="local"), 20),
    (2, dict(ny=300, nx=1200, tsteps=12, dims=(1, 2), graph=True), 24),
])
def test_residual_and_solve(np_, cfg, every, tmp_path):
    """F: residual_norm includes s and is read-only; the deciding check of a solve is the reference series'."""
    specs = [(4, 1, "l2"), (3, 0, "max")]
    jobs = [dict(cfg, kind="resid", src_every=every, pre=(every + 3, 9), save=str(tmp_path / "r"))]
    jobs += [sc.solve_job(cfg, every, c, lag, norm, str(tmp_path / f"s{i}")) for i, (c, lag, norm) in enumerate(specs)]
    res = _launch(jobs, np_)
    sc.check_resid(jobs[0], res[0], jobs[0]["save"])
    for job, got, (c, lag, norm) in zip(jobs[1:], res[1:], specs):
        sc.check_solve(job, got, every, c, lag, norm)


def test_solve_converges(tmp_path):
    """64 x 64 Dirichlet, tblock 4, blocks of 20: solve to 1e-9 in the max norm, then compare with the converged NumPy iteration."""
    job = sc.converge_job(str(tmp_path / "c"), transport="local", graph=True)
    (got,) = _launch([job])
    sc.check_converged(job, got)
