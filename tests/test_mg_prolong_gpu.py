"""The interpolation fused into the first post-smoothing pass of the multigrid
cycle (NativeJacobi.mg(fuse_prolong=True)) on the GPU: the assertions of
tests/test_mg_prolong_cpu.py at 255 x 511 after 4 cycles — interior() is bitwise
engine.serial_mg and bitwise the same engine's fuse_prolong = False field, r0
and the residuals are that call's bit for bit, prolong_levels is
engine.mg_prolong_levels' — on one rank and on two ranks that share cuda:0 over
IPC, with tsteps = 2, fuse = 2, red-black, and with tsteps = 4, fuse = 4,
red-black, nu = (1, 2), so that a 4-deep chunk runs on the fine level; each
with the fused residual off and on, and run(k) after the fused call is bitwise
run(k) after the plain one.  Every child runs under `timeout`; once a
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


@pytest.mark.parametrize("tsteps,fuse,nu", [(2, 2, (2, 2)), (4, 4, (1, 2))])
@pytest.mark.parametrize("name,np_,cfg", [
    ("one rank", 1, dict(transport="local")),
    ("1x2 over IPC", 2, dict(dims=(1, 2))),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_fused_prolong_is_the_two_kernels(name, np_, cfg, tsteps, fuse, nu, tmp_path):
    from gpu_mpi_tests_amd import engine

    dims = cfg.get("dims") or (1, 1)
    kw = dict(max_cycles=CYCLES, fuse=fuse, smoother="rb", nu=nu)
    ops = []
    for fr in (False, True):
        ops += [dict(op="reset"), dict(op="mg", tag=f"plain{int(fr)}", kw=dict(kw, fuse_resid=fr, fuse_prolong=False)),
                dict(op="reset"), dict(op="mg", tag=f"fused{int(fr)}", kw=dict(kw, fuse_resid=fr, fuse_prolong=True))]
    # run(k) after the fused call (the last one above) and after a plain one
    ops += [dict(op="run", k=2 * tsteps, tag="run"), dict(op="reset"),
            dict(op="mg", tag="plain_again", kw=dict(kw, fuse_resid=True, fuse_prolong=False)),
            dict(op="run", k=2 * tsteps, tag="run_plain")]
    out = str(tmp_path / "fields.npz")
    res = _launch(dict(cfg, ny=NY, nx=NX, tsteps=tsteps, ops=ops, out=out), np_)
    fields = dict(np.load(out))
    levels = engine.mg_prolong_levels(NY, NX, dims, tsteps, fuse, nu[1], "rb")
    nlev = len(engine.mg_levels(NY, NX, dims))
    assert levels and levels[0] == 0, levels
    if tsteps == 4:
        assert engine.mg_fuse_depths(NY, NX, dims, fuse, tsteps)[0] == 4  # c = 4 on the fine level
    want, _ = engine.serial_mg(NY, NX, CYCLES, init="random", seed=SEED, nu=nu, max_levels=nlev, smoother="rb")
    for i in (0, 1):
        plain, fused = res[2 + 4 * i], res[4 + 4 * i]
        assert plain["same"] and fused["same"]
        for k in RESULT_KEYS:
            assert plain["res"][k] == fused["res"][k], (k, plain["res"], fused["res"])
        assert fused["res"]["fuse_prolong"] is True and fused["res"]["prolong_levels"] == levels, fused["res"]
        assert plain["res"]["fuse_prolong"] is False and plain["res"]["prolong_levels"] == [], plain["res"]
        assert plain["res"]["resid_levels"] == fused["res"]["resid_levels"]
        assert same_bits(fields[f"plain{i}"], fields[f"fused{i}"]), i
        assert same_bits(fields[f"fused{i}"], want), i
    assert not same_bits(fields["run"], fields["fused1"]) and np.isfinite(fields["run"]).all()
    # the fused path leaves the engine as the pair does: run(k) continues to the same bits
    assert same_bits(fields["plain_again"], fields["plain1"]) and same_bits(fields["run"], fields["run_plain"])
