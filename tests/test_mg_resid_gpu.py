"""The fused residual + restriction of the multigrid cycle
(NativeJacobi.mg(fuse_resid=True)) on the GPU: the assertions of
tests/test_mg_resid_cpu.py at 255 x 511 after 4 cycles with fuse = 2 and the
red-black smoother — interior() is bitwise engine.serial_mg and bitwise the
same engine's fuse_resid = False field, r0 and the residuals are that call's
bit for bit, resid_levels is engine.mg_resid_levels' — on one rank and on two
ranks that share cuda:0 over IPC with tsteps = 2 (the fine level fuses too).
Every child runs under `timeout`; once a child has failed nothing further runs
on the GPU from this file."""
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
from test_mg_cpu import same_bits
from test_mg_resid_cpu import RESULT_KEYS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mg_worker.py")
NY, NX, CYCLES = 255, 511, 4
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
    ("one rank", 1, dict(transport="local")),
    ("1x2 over IPC", 2, dict(dims=(1, 2), tsteps=2)),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_fused_transfer_is_the_two_kernels(name, np_, cfg, tmp_path):
    from gpu_mpi_tests_amd import engine

    dims = cfg.get("dims") or (1, 1)
    tsteps = cfg.get("tsteps", 1)
    kw = dict(max_cycles=CYCLES, fuse=2, smoother="rb")
    ops = [dict(op="reset"), dict(op="mg", tag="plain", kw=dict(kw, fuse_resid=False)),
           dict(op="reset"), dict(op="mg", tag="fused", kw=dict(kw, fuse_resid=True)),
           dict(op="run", k=2 * tsteps, tag="run")]
    out = str(tmp_path / "fields.npz")
    res = _launch(dict(cfg, ny=NY, nx=NX, ops=ops, out=out), np_)
    fields = dict(np.load(out))
    plain, fused = res[2], res[4]
    assert plain["same"] and fused["same"]
    for k in RESULT_KEYS:
        assert plain["res"][k] == fused["res"][k], (k, plain["res"], fused["res"])
    levels = engine.mg_resid_levels(NY, NX, dims, tsteps)
    nlev = len(engine.mg_levels(NY, NX, dims))
    assert levels == list(range(nlev - 1)), levels  # every restricting level, the fine one included
    assert fused["res"]["fuse_resid"] is True and fused["res"]["resid_levels"] == levels, fused["res"]
    assert plain["res"]["fuse_resid"] is False and plain["res"]["resid_levels"] == [], plain["res"]
    assert same_bits(fields["plain"], fields["fused"])
    want, _ = engine.serial_mg(NY, NX, CYCLES, init="random", seed=SEED, max_levels=nlev, smoother="rb")
    assert same_bits(fields["fused"], want)
    assert not same_bits(fields["run"], fields["fused"]) and np.isfinite(fields["run"]).all()
