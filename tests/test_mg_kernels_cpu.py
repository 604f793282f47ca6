"""The multigrid kernels (gmt_mg_smooth, gmt_mg_restrict, gmt_mg_prolong_add) of
the CPU backend against the NumPy model of tests/mg_cases.py: every width,
height, alignment variant and parity, the identities, empty regions and every
refusal — the checks of tests/test_mg_kernels_gpu.py without the path
assertions.  In a child process: build/lib-host/libgmt.so shares its SONAME
with the GPU library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def test_host_mg_kernels_match_numpy():
    import mg_cases as mc

    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mg_cases.py"), HOST_LIB],
                       capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["ok"] and r["cases"] == [mc.N_SMOOTH, mc.N_RESTRICT, mc.N_PROLONG], r["cases"]
    assert r["codes"] == [1] * mc.N_REFUSALS  # hipErrorInvalidValue's number: the GPU test asserts the same list
    assert r["paths"] == [[0, 0], 0, 0]       # GMT_PATH_NONE: the CPU backend has no kernel to pick


def test_transfer_model_cell_by_cell():
    """The vectorised models of mg_cases against the definition written out cell by cell."""
    import mg_cases as mc

    for px, py in mc.PARITIES:
        nx, ny = 7, 6
        d, _, region, _, (mx, my) = mc.restrict_fields(nx, ny, px, py, "fast")
        x0, _, y0, _ = region
        D = d.a
        got = mc.restrict_reference(d, region, px, py, mx, my)
        assert (mx, my) == (len(range(px, nx, 2)), len(range(py, ny, 2)))
        for J in range(my):
            for I in range(mx):
                x, y = x0 + px + 2 * I, y0 + py + 2 * J
                h = [(D[r, x - 1] + D[r, x + 1]) + 2 * D[r, x] for r in (y - 1, y, y + 1)]
                assert got[J, I] == mc.CS * ((h[0] + h[2]) + 2 * h[1])
        e, u, region, (cx0, cy0) = mc.prolong_fields(nx, ny, px, py, "fast")
        x0, _, y0, _ = region
        E, U = e.a, u.a
        got = mc.prolong_reference(e, u, region, px, py, (cx0, cy0))
        for j in range(ny):
            for i in range(nx):
                # coarse index of region-relative fine index t: (t - p)/2, a half-integer between two points
                fx, fy = (i - px) / 2 + cx0, (j - py) / 2 + cy0
                xs = [int(fx)] if fx == int(fx) else [int(np.floor(fx)), int(np.floor(fx)) + 1]
                ys = [int(fy)] if fy == int(fy) else [int(np.floor(fy)), int(np.floor(fy)) + 1]
                v = [[E[y, x] for x in xs] for y in ys]
                if len(xs) == 1 and len(ys) == 1:
                    t = v[0][0]
                elif len(ys) == 1:
                    t = 0.5 * (v[0][0] + v[0][1])
                elif len(xs) == 1:
                    t = 0.5 * (v[0][0] + v[1][0])
                else:
                    t = 0.25 * ((v[0][0] + v[0][1]) + (v[1][0] + v[1][1]))
                assert got[j, i] == U[y0 + j, x0 + i] + t, (px, py, i, j)


def test_reference_ops_mg():
    """ops.mg_* on CPU tensors (ops/reference.py) against the model; the wrappers refuse shared storage."""
    import torch

    import mg_cases as mc
    from gpu_mpi_tests_amd import ops

    for with_f in (False, True):
        for om in mc.OMEGAS:
            u, o, f, region = mc.smooth_fields(129, 17, "fast", with_f)
            want = mc.smooth_reference(region, u, f, om)
            x0, nx, y0, ny = region
            to = torch.from_numpy(o.a)
            assert ops.mg_smooth(torch.from_numpy(u.a), to, om, region,
                                 None if f is None else torch.from_numpy(f.a)) is to
            assert mc.same_bits(o.a[y0:y0 + ny, x0:x0 + nx], want)
    for px, py in mc.PARITIES:
        for nx, ny in ((130, 9), (129, 4), (1, 1), (2, 3)):
            d, s, region, (cx0, cy0), (mx, my) = mc.restrict_fields(nx, ny, px, py, "fast")
            want = mc.restrict_reference(d, region, px, py, mx, my)
            ts = torch.from_numpy(s.a)
            assert ops.mg_restrict(torch.from_numpy(d.a), ts, region, (px, py), (cx0, cy0)) is ts
            assert mc.same_bits(s.a[cy0:cy0 + my, cx0:cx0 + mx], want)
            e, u, region, coarse = mc.prolong_fields(nx, ny, px, py, "fast")
            x0, _, y0, _ = region
            want = mc.prolong_reference(e, u, region, px, py, coarse)
            tu = torch.from_numpy(u.a)
            assert ops.mg_prolong_add(torch.from_numpy(e.a), tu, region, (px, py), coarse) is tu
            assert mc.same_bits(u.a[y0:y0 + ny, x0:x0 + nx], want), (px, py, nx, ny)
    u, _, _, region = mc.smooth_fields(9, 5, "fast", False)
    tu = torch.from_numpy(u.a)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_smooth(tu, tu, 0.8, region)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_smooth(tu, tu[1:, 2:], 0.8, (1, 3, 1, 2))
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_prolong_add(tu, tu, (1, 3, 1, 2), (1, 1), (1, 1))
