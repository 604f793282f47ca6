"""gmt_mg_resid_restrict of the CPU backend against the NumPy model of
tests/mg_resid_cases.py: every mask, parity, width, height and alignment
variant, the identities against the two existing calls, empty regions and
every refusal — the checks of tests/test_mg_resid_kernels_gpu.py without the
path assertions.  In a child process: build/lib-host/libgmt.so shares its
SONAME with the GPU library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def test_host_mg_resid_restrict_matches_numpy():
    import mg_resid_cases as rc

    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mg_resid_cases.py"), HOST_LIB],
                       capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    want = [rc.N_ALL_MASKS, 9 * 2 * rc.N_SWEEP, rc.N_HEIGHTS * 2 * rc.N_SWEEP, rc.N_SCALAR, 2 * 2 * 2 * 4 * 2]
    assert r["ok"] and r["cases"] == want, (r["cases"], want)
    assert r["codes"] == [1] * rc.N_REFUSALS  # hipErrorInvalidValue's number: the GPU test asserts the same list
    assert r["path"] == [0, 0]                # GMT_PATH_NONE: the CPU backend has no kernel to pick
    assert r["geom"] == [124, 496]            # the gfx950 kernel's, so the widths are the same


def test_model_cell_by_cell():
    """reference.mg_resid_restrict against the definition written out cell by cell: d on the grown box, +0.0 on
    the rest of the ring, then the full weighting, for every mask and parity."""
    import mg_resid_cases as rc
    from gpu_mpi_tests_amd.ops import reference as ref

    nx, ny = 5, 4
    for mask in range(16):
        for par in rc.PARITIES:
            for with_f in (False, True):
                u, _, f, region, coarse = rc.fields(nx, ny, mask, par, "fast", with_f)
                x0, _, y0, _ = region
                want = rc.reference(region, par, mask, coarse, u, f)
                hw, he, hs, hn = (bool(mask & b) for b in (1, 2, 4, 8))
                U = u.a
                D = {}
                for y in range(y0 - 1, y0 + ny + 1):
                    for x in range(x0 - 1, x0 + nx + 1):
                        inx = x0 - hw <= x < x0 + nx + he
                        iny = y0 - hs <= y < y0 + ny + hn
                        if inx and iny:
                            o = rc.C0 * ((U[y, x - 1] + U[y, x + 1]) + (U[y - 1, x] + U[y + 1, x]))
                            if f is not None:
                                o = o + rc.C1 * f.a[y, x]
                            D[y, x] = o - U[y, x]
                        else:
                            D[y, x] = 0.0
                H = lambda r, x: (D[r, x - 1] + D[r, x + 1]) + 2.0 * D[r, x]  # noqa: E731
                got = np.array([[rc.CS * ((H(y - 1, x) + H(y + 1, x)) + 2.0 * H(y, x))
                                 for x in range(x0 + par[0], x0 + nx, 2)] for y in range(y0 + par[1], y0 + ny, 2)])
                assert rc.same_bits(got.reshape(want.shape), want), (mask, par, with_f)
    with pytest.raises(ValueError):
        ref.mg_resid_restrict(u.a, np.zeros((9, 9)), 0.25, x0, nx, y0, ny, 1, 1, 16)
    with pytest.raises(ValueError):
        ref.mg_resid_restrict(u.a, np.zeros((9, 9)), 0.25, x0, nx, y0, ny, 2, 1, 0)


def test_reference_ops_mg_resid_restrict():
    """ops.mg_resid_restrict on CPU tensors (ops/reference.py) against the model; shared storage is refused."""
    import torch

    import mg_resid_cases as rc
    from gpu_mpi_tests_amd import ops

    for mask in (0, 15, 6):
        for par in rc.PARITIES:
            for with_f in (False, True):
                u, s, f, region, coarse = rc.fields(37, 9, mask, par, "fast", with_f)
                want = rc.reference(region, par, mask, coarse, u, f)
                cx0, cy0, mx, my = coarse
                ts = torch.from_numpy(s.a)
                assert ops.mg_resid_restrict(torch.from_numpy(u.a), ts, region, par, (cx0, cy0), mask,
                                             None if f is None else torch.from_numpy(f.a)) is ts
                assert rc.same_bits(s.a[cy0:cy0 + my, cx0:cx0 + mx], want)
                s.a[cy0:cy0 + my, cx0:cx0 + mx] = rc.SENTINEL
                assert (s.store == rc.SENTINEL).all()
    tu = torch.from_numpy(u.a)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_resid_restrict(tu, tu, region, par, (cx0, cy0))
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_resid_restrict(tu, ts, region, par, (cx0, cy0), 0, ts[1:, 2:])
