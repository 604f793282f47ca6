"""The shared hand-off group option of inline-halo passes (gmt_tb_opts.shared
with push, NativeJacobi(shared=), mpi_jacobi2d --shared) on the CPU backend:
it has no group kernels, answers 0 for both queries, and accepts and ignores
the option.

Each case runs in a fresh interpreter: the HIP and host libraries share the
libgmt.so SONAME, so one process may only ever bind one backend."""
import json
import os
import re
import subprocess
import sys

import pytest

from native_util import ROOT, ensure_host_build, have_mpi, run_app

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")

CODE = r"""
import json, sys
sys.path.insert(0, {root!r})
import numpy as np
from gpu_mpi_tests_amd import engine, ops
from gpu_mpi_tests_amd.parallel import dist as gd
out = dict(supported=[int(ops.tb_push_shared_supported(k, nw)) for k in (12, 16, 20) for nw in (2, 4)],
           paths=[ops.jacobi5tb_shared_path(20, [(24, 2000, 20, 300)], 15, shared=sh, push_w=pw)
                  for sh in (0, 1, 2, 4) for pw in (0, 20)])
env = gd.init(device="cpu")
ny, nx, steps, k = 300, 1000, 43, 20
e = engine.NativeJacobi(ny, nx, env, periodic=True, overlap=False, graph=False, tblock=k, push=True, shared=4,
                        transport="local", init="random", seed=5)
out["push"] = e.push_active
out["shared_strips"] = e.tb_launch(k)["shared_strips"]
e.run(steps); e.synchronize()
got = e.interior()
e.close()
want = engine.serial_jacobi(ny, nx, steps, True, init="random", seed=5)
out["equal"] = bool(np.array_equal(got, want))
try:
    engine.NativeJacobi(ny, nx, env, periodic=True, tblock=k, push=True, shared=3, transport="local")
    out["bad_shared"] = "accepted"
except ValueError as ex:
    out["bad_shared"] = "ValueError"
print(json.dumps(out))
"""


def test_cpu_backend_ignores_shared_for_push_passes():
    ensure_host_build()
    p = subprocess.run([sys.executable, "-c", CODE.format(root=ROOT)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", GMT_LIB=HOST_LIB))
    assert p.returncode == 0, p.stdout + p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["supported"] == [0] * 6, r
    assert r["paths"] == [0] * 8, r
    assert r["push"] is True and r["shared_strips"] == 0, r
    assert r["equal"], r
    assert r["bad_shared"] == "ValueError", r


@pytest.mark.skipif(not have_mpi(), reason="mpirun not available")
def test_mpi_jacobi2d_shared_push_check_on_the_host_build():
    out = run_app("mpi_jacobi2d", "--ny=300", "--nx=2000", "0", "45", "--tblock", "--tsteps=20", "--periodic",
                  "--dims=1x2", "--transport=ipc", "--shared=4", "--push", "--check", "--warmup=2", np=2).stdout
    assert re.search(r"check     : max\|diff\| vs serial = (\S+) OK", out), out
    assert "(inline halo)" in out, out
    # the CPU backend has no group kernels: the option is accepted and ignored
    assert re.search(r"shared    = 4 \(rank 0: 0 strips", out), out


@pytest.mark.skipif(not have_mpi(), reason="mpirun not available")
def test_mpi_jacobi2d_rejects_a_bad_shared_value():
    p = run_app("mpi_jacobi2d", "64", "2", "--shared=3", np=1, check=False)
    assert p.returncode != 0 and "--shared=3" in p.stdout, p.stdout + p.stderr
