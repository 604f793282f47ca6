"""The Chebyshev step (gmt_cheby_step) of the CPU backend against the NumPy model
of tests/cheby_cases.py: every width, height, alignment variant and weight, with
and without f, empty regions and every refusal — the checks of
tests/test_cheby_kernels_gpu.py without the path assertions.  In a child
process: build/lib-host/libgmt.so shares its SONAME with the GPU library."""
import json
import os
import subprocess
import sys

import pytest

from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def test_host_cheby_step_matches_numpy():
    import cheby_cases as hc

    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cheby_cases.py"), HOST_LIB],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["ok"] and r["cases"] == len(hc.NXS) * (len(hc.ALIGN) + len(hc.ALIGN_F)) * 7 * len(hc.WEIGHTS)
    assert r["codes"] == [1] * hc.N_REFUSALS  # hipErrorInvalidValue's number: the GPU test asserts the same list
    assert r["paths"] == [[0, 0]]             # GMT_PATH_NONE: the CPU backend has no kernel to pick


def test_reference_ops_cheby_step():
    """ops.cheby_step on CPU tensors (the PyTorch reference path) against the NumPy model;
    the wrapper refuses u and v that share storage."""
    import torch

    import cheby_cases as hc
    from gpu_mpi_tests_amd import ops

    for with_f in (False, True):
        for w in hc.WEIGHTS:
            u, v, f, region = hc.fields(129, 17, "fast", with_f)
            want = hc.reference(region, u, v, f, w)
            x0, nx, y0, ny = region
            tv = torch.from_numpy(v.a)
            assert ops.cheby_step(torch.from_numpy(u.a), tv, w, region,
                                  None if f is None else torch.from_numpy(f.a)) is tv
            assert hc.same_bits(v.a[y0:y0 + ny, x0:x0 + nx], want)
    u, v, _, region = hc.fields(9, 5, "fast", False)
    tu = torch.from_numpy(u.a)
    with pytest.raises(ValueError, match="share storage"):
        ops.cheby_step(tu, tu, 1.0, region)
    with pytest.raises(ValueError, match="share storage"):
        ops.cheby_step(tu, tu[1:, 2:], 1.0, (1, 3, 1, 2))
