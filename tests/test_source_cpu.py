"""The Poisson source term on the CPU backend: gmt_add2d and the fill modes 6
and 7 bitwise against NumPy; the engine's single source sweeps bitwise against
the float64 NumPy sweeps; its fused blocks (Laplace passes + one add of the
block field, JacobiConfig::source) bitwise independent of the decomposition
and within a derived rounding bound of long double single sweeps
(tests/source_cases.py); the fixed point of the poly source; residual_norm and
solve with a source; mpi_jacobi2d --source."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import source_cases as sc
from conftest import free_port
from native_util import ROOT, ensure_host_build, have_mpi, run_app

WORKER = os.path.join(ROOT, "tests", "source_worker.py")
HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def _worker(jobs, np_=1, transport="rccl"):
    ensure_host_build()
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    if np_ == 1:
        cmd = [sys.executable, WORKER, json.dumps(jobs)]
    else:
        env["GMT_TRANSPORT"] = transport
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(np_),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), WORKER, json.dumps(jobs)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("[")][-1])


def test_host_add2d_and_fills():
    """A and B on the CPU backend, in a child process (the library shares its SONAME with the GPU one)."""
    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "source_cases.py"), HOST_LIB], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["ok"] and r["cases"] == len(sc.ADD_CASES)
    assert r["refused"] == [1] * (len(sc.ADD_REFUSED) + 2), r  # hipErrorInvalidValue's value, as on the GPU
    assert r["big"] in (True, None), r  # None: the allocation failed


def test_reference_ops_add2d():
    """ops.add2d on CPU tensors (the PyTorch reference path) runs the same cases."""
    import torch

    from gpu_mpi_tests_amd import ops

    def add(g, gs, u, us):
        ops.add2d(torch.from_numpy(g)[gs], torch.from_numpy(u)[us])
        return g, u

    assert sc.run_add_cases(add) == len(sc.ADD_CASES)
    with pytest.raises(ValueError):
        ops.add2d(torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 5, dtype=torch.float64))


def test_source_model_is_the_engines():
    """engine.source_field is the fill model of the engine's lattice; serial_jacobi without a source is unchanged."""
    from gpu_mpi_tests_amd import engine

    h = 1.0 / 71
    assert sc.same_bits(engine.source_field(40, 70, "poly"), sc.fill_model(7, 70, 40, 0.0, h, 0.0, h))
    assert sc.same_bits(engine.source_field(40, 70, "random", seed=4, source_amp=0.25),
                        sc.fill_model(6, 70, 40, 0.0, 5.0, 0.0, 0.25))
    assert sc.same_bits(engine.serial_jacobi(9, 11, 3), engine.serial_jacobi(9, 11, 3, source=None))
    with pytest.raises(ValueError):
        engine.source_field(4, 4, "cubic")


def test_single_sweep_source_path(tmp_path):
    """C: one rank, 40 x 70, 7 sweeps, Dirichlet and periodic, overlap on (core and frame) and off."""
    jobs = [dict(sc.SINGLE, periodic=p, overlap=o, save=str(tmp_path / f"s{int(p)}{int(o)}"))
            for p in (False, True) for o in (False, True)]
    res = _worker(jobs)
    for job, r in zip(jobs, res):
        assert r["source_plan"] == dict(blocks=0, src_every=0, tail=7) and r["setup"]["sweeps"] == 0, r
        sc.check_single(job, job["save"])


def test_single_sweep_source_path_two_ranks(tmp_path):
    """The core-and-frame path with a real neighbour, and the built-in random source."""
    from gpu_mpi_tests_amd import engine

    jobs = [dict(sc.SINGLE, dims=(2, 1), overlap=True, transport="auto", save=str(tmp_path / "a")),
            dict(sc.SINGLE, dims=(1, 2), overlap=True, transport="auto", source="random", source_amp=0.125,
                 save=str(tmp_path / "b"))]
    _worker(jobs, 2, "ipc")
    sc.check_single(jobs[0], jobs[0]["save"])
    want = engine.serial_jacobi(40, 70, 7, init="random", seed=sc.SEED, source="random", source_amp=0.125)
    assert sc.same_bits(np.load(jobs[1]["save"] + ".npy"), want)


@pytest.mark.parametrize("name,np_,cfg", sc.FUSED,
                         ids=lambda v: v.replace(" ", "_").replace(",", "") if isinstance(v, str) else None)
def test_fused_source_path(name, np_, cfg, tmp_path):
    """D on the host emulations (ipc where the halo is inline, rccl otherwise)."""
    prefix, base = str(tmp_path / "f"), str(tmp_path / "b")
    res = _worker(sc.fused_jobs(cfg, prefix), np_, "ipc" if cfg.get("push") else "rccl")
    _worker(sc.baseline_jobs(cfg, base))
    sc.check_fused(cfg, res, prefix, base, gpu=False)


def test_fixed_point(tmp_path):
    """E: x^3 + y^2 with the poly source."""
    job = dict(ny=sc.N_CONV, nx=sc.N_CONV, tsteps=4, src_every=20, kind="run", sweeps=60, init="analytic",
               source="poly", resid0=True, transport="local", save=str(tmp_path / "p"))
    (r,) = _worker([job])
    sc.check_fixed_point(r, job["save"], 60, 20)


@pytest.mark.parametrize("np_,transport,cfg,every", [
    (1, "rccl", dict(ny=60, nx=64, tsteps=1, transport="local"), 12),
    (1, "rccl", dict(ny=60, nx=64, tsteps=20, periodic=True, transport="local"), 20),
    (2, "ipc", dict(ny=300, nx=700, tsteps=12, dims=(1, 2), periodic=True, overlap=True), 24),
    (4, "rccl", dict(ny=60, nx=64, tsteps=4, dims=(2, 2)), 16),
])
def test_residual_and_solve(np_, transport, cfg, every, tmp_path):
    """F: residual_norm includes s and is read-only; the deciding check of a solve is the reference series'."""
    specs = [(4, 1, "l2"), (3, 0, "max")]
    ts = cfg["tsteps"]
    jobs = [dict(cfg, kind="resid", src_every=every if ts > 1 else 0, pre=(every + 3, 9), save=str(tmp_path / "r"))]
    jobs += [sc.solve_job(cfg, every, c, lag, norm, str(tmp_path / f"s{i}")) for i, (c, lag, norm) in enumerate(specs)]
    if ts == 1:
        for j in jobs:
            j["src_every"] = 0
    res = _worker(jobs, np_, transport)
    sc.check_resid(jobs[0], res[0], jobs[0]["save"])
    for job, got, (c, lag, norm) in zip(jobs[1:], res[1:], specs):
        sc.check_solve(job, got, every, c, lag, norm)


def test_solve_converges(tmp_path):
    """64 x 64 Dirichlet, tblock 4, blocks of 20: solve to 1e-9 in the max norm, then compare with the converged NumPy iteration."""
    job = sc.converge_job(str(tmp_path / "c"), transport="local")
    (got,) = _worker([job])
    sc.check_converged(job, got)


BAD_ARGS = """
import sys
sys.path.insert(0, sys.argv[1])
from gpu_mpi_tests_amd import engine
from gpu_mpi_tests_amd.parallel import dist as gd
env = gd.init(device="cpu")
bad = 0
for kw in (dict(source="cubic"), dict(source="random", source_amp=-1.0), dict(source="random", source_amp=float("nan")),
           dict(source="poly", tblock=12, src_every=18), dict(source="poly", src_every=-1)):
    try:
        engine.NativeJacobi(32, 32, env, **kw)
    except ValueError:
        bad += 1
e = engine.NativeJacobi(32, 32, env, source="poly")
try:
    e.set_source([[0.0] * 32] * 32)
except engine.EngineError:
    bad += 1
print("refused", bad)
"""


def test_bad_source_arguments():
    """Every bad option is a ValueError before anything is built; set_source needs an ndarray engine."""
    ensure_host_build()
    p = subprocess.run([sys.executable, "-c", BAD_ARGS, ROOT], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0 and "refused 6" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


@pytest.mark.skipif(not have_mpi(), reason="no mpirun")
@pytest.mark.parametrize("np_", [1, 2, 4])
def test_app_source(np_, tmp_path):
    """G: mpi_jacobi2d --source on the CPU backend, --check against its serial run with the same source."""
    js = tmp_path / "out.json"
    p = run_app("mpi_jacobi2d", "64", "30", "--ny=60", "--warmup=5", "--source=poly", "--check", f"--json={js}", np=np_)
    assert re.search(r"source    = poly every 1 sweeps \(set-up 0 sweeps, [0-9.]+ ms, [0-9.]+ MiB\)", p.stdout), p.stdout
    assert re.search(r"check\s*: max\|diff\| vs serial = [0-9.eE+-]+ OK", p.stdout), p.stdout
    m = re.search(r"source err: max\|u - u0\| = ([0-9.eE+-]+)", p.stdout)
    assert m and float(m.group(1)) < 1e-12, p.stdout
    j = json.loads(js.read_text().strip().splitlines()[-1])
    assert j["source"] == "poly" and j["src_every"] == 1 and "source_setup_ms" in j, j
    q = run_app("mpi_jacobi2d", "64", "90", "--ny=60", "--warmup=13", "--tblock", "--source=random:0.01",
                "--src-every=40", "--check", f"--json={js}", np=np_)
    assert re.search(r"source    = random:0\.01 every 40 sweeps \(set-up 40 sweeps, [0-9.]+ ms, [0-9.]+ MiB\)", q.stdout), \
        q.stdout
    assert re.search(r"check\s*: max\|diff\| vs serial = [0-9.eE+-]+ OK", q.stdout), q.stdout
    assert "source err" not in q.stdout, q.stdout
    j = json.loads(js.read_text().strip().splitlines()[-1])
    assert j["source"] == "random" and j["src_every"] == 40 and j["source_setup_ms"] >= 0, j
    # the zero-source run computes something else: the check sees the term
    z = run_app("mpi_jacobi2d", "64", "90", "--ny=60", "--warmup=13", "--tblock", np=np_)
    assert "source" not in z.stdout, z.stdout
    assert re.search(r"residual  : ([0-9.e+-]+)", z.stdout).group(1) != re.search(r"residual  : ([0-9.e+-]+)",
                                                                                 q.stdout).group(1)
