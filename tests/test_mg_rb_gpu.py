"""Red-black Gauss-Seidel smoothing of the multigrid cycle
(NativeJacobi.mg(smoother="rb")) on the GPU: the assertions of
tests/test_mg_rb_cpu.py — after the cycles interior() is bitwise
engine.serial_mg(smoother="rb"), r0 and the residual within 2e-13 relative of
the serial fields' — on one rank and on two ranks that share cuda:0 over IPC
(1 x 2 and 2 x 1), at 63 x 127 (nested) and 64 x 100 (coarsen="any"), for fuse
0, 2 and 4, with and without a source, on engines of tsteps 1 and 4 (on two
ranks the fine level fuses only with the deeper ghost ring).  One child process
per process grid (tests/mg_rb_worker.py builds its engines one after another),
each under `timeout`; once a child has failed nothing further runs on the GPU
from this file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import free_port
from gpu_mpi_tests_amd import _native
from test_mg_rb_cpu import check_against_serial, engine_entries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mg_rb_worker.py")
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


@pytest.mark.parametrize("np_,dims", [(1, None), (2, (1, 2)), (2, (2, 1))],
                         ids=lambda v: None if isinstance(v, int) else str(v))
def test_rb_cycle_is_serial_mg(np_, dims, tmp_path):
    out = str(tmp_path / "fields.npz")
    engines, what = engine_entries(fuses=(0, 2, 4), nus=((1, 1), (2, 1)))
    cfg = dict(dims=dims, engines=engines, out=out)
    if np_ == 1:
        cfg["transport"] = "local"
    res = _launch(cfg, np_)
    check_against_serial(res, dict(np.load(out)), engines, what, dims or (1, 1))
