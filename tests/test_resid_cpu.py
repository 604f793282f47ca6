"""The read-only Jacobi residual (gmt_jacobi5_resid) of the CPU backend
against the NumPy fp64 reference with math.fsum: the definition checks of
tests/test_resid_gpu.py (every width, segment-seam height, alignment, with
and without f; spikes, NaN, an empty region, 2000 x 4000) without the path
assertions, sum to 1e-12.  In a child process: build/lib-host/libgmt.so
shares its SONAME with the GPU library."""
import json
import os
import subprocess
import sys

from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def test_host_residual_matches_numpy():
    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "resid_cases.py"), HOST_LIB], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["ok"] and r["widths"] == 20
    assert r["path"] == [0, 0]  # GMT_PATH_NONE, no segments: the CPU backend has no kernel to pick


def test_reference_ops_residual():
    """ops.jacobi5_resid on CPU tensors (the PyTorch reference path) against the same NumPy reference."""
    import torch

    import resid_cases as rc
    from gpu_mpi_tests_amd import ops

    for with_f in (False, True):
        case = rc.make_case(129, 17, "walk", with_f)
        U, F = rc.views(case)
        got = ops.jacobi5_resid(torch.from_numpy(U), case["region"], None if F is None else torch.from_numpy(F),
                                rc.C0, rc.C1 if with_f else 0.0)
        rc.check(case, (float(got[0]), float(got[1])), 1e-12, with_f)
