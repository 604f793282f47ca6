"""Geometric multigrid of the native Jacobi engine on the GPU: the assertions of
tests/test_mg_cpu.py (field bitwise engine.serial_mg on every process grid,
level table, coarse iteration count and rho, residuals by fsum, nu = (1, 1),
max_levels = 3, decision for lag 0, 1 and 3, the cap, a tolerance met at check
0, run() after mg(), a second mg()) through the engine kinds whose buffers and
transport mg() borrows — a plain engine at one rank, a tsteps = 20 engine at
1 x 2 replaying hipGraphs (run() before and after mg() still replays), an
inline-halo engine at 2 x 1, a 2 x 2 grid with overlap — all at 255 x 767 (the
fine level crosses the 512-column workgroup seam).  Ranks share cuda:0 over
IPC.  Every child runs under `timeout`; once a child has failed nothing further
runs on the GPU from this file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import free_port
from gpu_mpi_tests_amd import _native
from mg_worker import SEED
from test_mg_cpu import NX, NY, check_standard, close, same_bits, standard_ops, sweeps_from

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


def graph_ops(tsteps):
    """run() replays before and after an mg() that starts from a swept field."""
    return [dict(op="reset"), dict(op="run", k=2 * tsteps, tag="pre"), dict(op="rn"),
            dict(op="mg", tag="mid", kw=dict(max_cycles=3, lag=0)), dict(op="run", k=2 * tsteps, tag="post")]


@pytest.mark.parametrize("name,np_,cfg", [
    ("one rank plain", 1, dict(transport="local")),
    ("1x2 fused passes from graphs", 2, dict(dims=(1, 2), tsteps=20, graph=True)),
    ("2x1 inline halo", 2, dict(dims=(2, 1), tsteps=20, push=True)),
    ("2x2 overlap", 4, dict(dims=(2, 2), overlap=True)),
    ("1x2 with a source", 2, dict(dims=(1, 2), source="random")),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_mg_against_serial(name, np_, cfg, tmp_path):
    from gpu_mpi_tests_amd import engine

    tsteps = cfg.get("tsteps", 1)
    std = standard_ops(tsteps)
    ops = std + (graph_ops(tsteps) if cfg.get("graph") else [])
    out = str(tmp_path / "fields.npz")
    res = _launch(dict(cfg, ny=NY, nx=NX, ops=ops, out=out), np_)
    fields = dict(np.load(out))
    info = res[0]
    check_standard(res[:1 + len(std)], fields, cfg.get("dims") or (1, 1), cfg.get("source"), tsteps, info["umax"])
    if cfg.get("push"):
        assert info["push"], info
    if cfg.get("graph"):
        assert info["graph_fused"], info
        k = 2 * tsteps
        _, _, rn, mid, _ = res[1 + len(std):]
        assert np.array_equal(fields["pre"], engine.serial_jacobi(NY, NX, k, init="random", seed=SEED))  # replayed passes
        want, ser = engine.serial_mg(NY, NX, 3, init="random", seed=SEED, start=fields["pre"])
        m = mid["res"]
        assert mid["same"] and m["iters"] == 3 and m["failed"] == 0 and m["r0"] == rn["rn"][0], (m, rn)
        assert close(m["r0"], ser[0][0]) and close(m["residual"], ser[3][0]), (m, ser)
        assert same_bits(fields["mid"], want)
        swept = sweeps_from(fields["mid"], None, k)
        assert float(np.abs(fields["post"] - swept).max()) <= 1e-10 * info["umax"]
