"""gmt_mg_smooth_k of the CPU backend against the NumPy model of
tests/mg_fuse_cases.py: every k, width, height, mask and alignment variant, the
identities, empty regions and every refusal — the checks of
tests/test_mg_fuse_kernels_gpu.py without the path assertions.  In a child
process: build/lib-host/libgmt.so shares its SONAME with the GPU library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def test_host_mg_smooth_k_matches_numpy():
    import mg_fuse_cases as fc

    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mg_fuse_cases.py"), HOST_LIB],
                       capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    want = [sum(11 * fc.n_fast(k) for k in fc.KS), len(fc.KS) * fc.n_scalar(), len(fc.KS) * fc.N_ALL_MASKS]
    assert r["ok"] and r["cases"] == want, (r["cases"], want)
    assert r["codes"] == [1] * fc.N_REFUSALS  # hipErrorInvalidValue's number: the GPU test asserts the same list
    assert r["path"] == [0, 0]                # GMT_PATH_NONE: the CPU backend has no kernel to pick
    assert r["geom"] == [[124, 496], [124, 496], [120, 480]]  # the gfx950 kernel's, so the widths are the same


def test_model_cell_by_cell():
    """reference.mg_smooth_k against the definition written out cell by cell: U_j on the box B_j, every
    other cell kept, for every mask."""
    import mg_fuse_cases as fc
    from gpu_mpi_tests_amd.ops import reference as ref

    nx, ny = 4, 3
    for k in fc.KS:
        for mask in range(16):
            for with_f in (False, True):
                u, _, f, (x0, _, y0, _) = fc.fields(k, nx, ny, mask, "fast", with_f)
                want = fc.reference(k, (x0, nx, y0, ny), mask, u, f, 0.8)
                hw, he, hs, hn = (bool(mask & b) for b in (1, 2, 4, 8))
                U = {(y, x): u.a[y, x] for y in range(u.a.shape[0]) for x in range(u.a.shape[1])}
                for j in range(1, k + 1):
                    g = k - j
                    xs = range(x0 - (g if hw else 0), x0 + nx + (g if he else 0))
                    ys = range(y0 - (g if hs else 0), y0 + ny + (g if hn else 0))
                    new = dict(U)
                    for y in ys:
                        for x in xs:
                            o = fc.C0 * ((U[y, x - 1] + U[y, x + 1]) + (U[y - 1, x] + U[y + 1, x]))
                            if f is not None:
                                o = o + fc.C1 * f.a[y, x]
                            t = o - U[y, x]
                            new[y, x] = U[y, x] + 0.8 * t
                    U = new
                got = np.array([[U[y, x] for x in range(x0, x0 + nx)] for y in range(y0, y0 + ny)])
                assert fc.same_bits(got, want), (k, mask, with_f)
    with pytest.raises(ValueError):
        ref.mg_smooth_k(u.a, u.a.copy(), 0.8, x0, nx, y0, ny, 5)
    with pytest.raises(ValueError):
        ref.mg_smooth_k(u.a, u.a.copy(), 0.8, x0, nx, y0, ny, 2, 16)


def test_reference_ops_mg_smooth_k():
    """ops.mg_smooth_k on CPU tensors (ops/reference.py) against the model; shared storage is refused."""
    import torch

    import mg_fuse_cases as fc
    from gpu_mpi_tests_amd import ops

    for k in fc.KS:
        for mask in (0, 15, 6):
            for with_f in (False, True):
                u, o, f, region = fc.fields(k, 37, 9, mask, "fast", with_f)
                want = fc.reference(k, region, mask, u, f, 0.8)
                x0, nx, y0, ny = region
                to = torch.from_numpy(o.a)
                assert ops.mg_smooth_k(torch.from_numpy(u.a), to, 0.8, region, k, mask,
                                       None if f is None else torch.from_numpy(f.a)) is to
                assert fc.same_bits(o.a[y0:y0 + ny, x0:x0 + nx], want)
                o.a[y0:y0 + ny, x0:x0 + nx] = fc.SENTINEL
                assert (o.store == fc.SENTINEL).all()
    tu = torch.from_numpy(u.a)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_smooth_k(tu, tu, 0.8, region, 2)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_smooth_k(tu, tu[1:, 2:], 0.8, region, 2)
