"""gmt_mg_smooth_rb of the CPU backend against the NumPy model of
tests/mg_rb_cases.py: every h, width, height, mask, colour phase and alignment
variant, the identities, empty regions and every refusal — the checks of
tests/test_mg_rb_kernels_gpu.py without the path assertions.  In a child
process: build/lib-host/libgmt.so shares its SONAME with the GPU library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def test_host_mg_smooth_rb_matches_numpy():
    import mg_rb_cases as rc

    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mg_rb_cases.py"), HOST_LIB],
                       capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    want = [sum(11 * rc.n_fast(h) for h in rc.HS), len(rc.HS) * rc.n_scalar(), len(rc.HS) * rc.N_ALL_MASKS]
    assert r["ok"] and r["cases"] == want, (r["cases"], want)
    assert r["codes"] == [1] * rc.N_REFUSALS  # hipErrorInvalidValue's number: the GPU test asserts the same list
    assert r["path"] == [0, 0]                # GMT_PATH_NONE: the CPU backend has no kernel to pick
    assert r["geom"] == [[128, 512], [124, 496], [124, 496], [120, 480]]  # gmt_mg_smooth_k_geom(h)


def test_model_cell_by_cell():
    """reference.mg_smooth_rb against the definition written out cell by cell: U_j on the due cells of the box
    B_j, every other cell kept, for every mask and both colour phases."""
    import mg_rb_cases as rc
    from gpu_mpi_tests_amd.ops import reference as ref

    nx, ny = 4, 3
    for h in rc.HS:
        for mask in range(16):
            for par in (0, 1):
                for with_f in (False, True):
                    u, _, f, (x0, _, y0, _) = rc.fields(h, nx, ny, mask, "fast", with_f)
                    want = rc.reference(h, par, (x0, nx, y0, ny), mask, u, f, 0.8)
                    hw, he, hs, hn = (bool(mask & b) for b in (1, 2, 4, 8))
                    U = {(y, x): u.a[y, x] for y in range(u.a.shape[0]) for x in range(u.a.shape[1])}
                    for j in range(1, h + 1):
                        g = h - j
                        xs = range(x0 - (g if hw else 0), x0 + nx + (g if he else 0))
                        ys = range(y0 - (g if hs else 0), y0 + ny + (g if hn else 0))
                        new = dict(U)
                        for y in ys:
                            for x in xs:
                                if ((x - x0) + (y - y0) + par + (j - 1)) % 2:  # Python's %: the mathematical mod
                                    continue
                                o = rc.C0 * ((U[y, x - 1] + U[y, x + 1]) + (U[y - 1, x] + U[y + 1, x]))
                                if f is not None:
                                    o = o + rc.C1 * f.a[y, x]
                                t = o - U[y, x]
                                new[y, x] = U[y, x] + 0.8 * t
                        U = new
                    got = np.array([[U[y, x] for x in range(x0, x0 + nx)] for y in range(y0, y0 + ny)])
                    assert rc.same_bits(got, want), (h, mask, par, with_f)
    for bad in (dict(h=5, par=0), dict(h=0, par=0), dict(h=2, par=2), dict(h=2, par=-1), dict(h=2, par=0, halo_mask=16)):
        with pytest.raises(ValueError):
            ref.mg_smooth_rb(u.a, u.a.copy(), 0.8, x0, nx, y0, ny, **bad)


def test_a_sweep_is_gauss_seidel():
    """With omega = 1 the black half-sweep reads the red cells just written: one h = 2 call is the sweep that
    updates red cells from u and black cells from the updated red ones."""
    import mg_rb_cases as rc

    u, _, _, region = rc.fields(2, 9, 7, 0, "fast", False)
    x0, nx, y0, ny = region
    got = rc.reference(2, 0, region, 0, u, None, 1.0)
    a = u.a.copy()
    for colour in (0, 1):
        for y in range(y0, y0 + ny):
            for x in range(x0, x0 + nx):
                if ((x - x0) + (y - y0)) % 2 == colour:  # in place: the other colour's cells are not read-modified
                    o = rc.C0 * ((a[y, x - 1] + a[y, x + 1]) + (a[y - 1, x] + a[y + 1, x]))
                    a[y, x] = a[y, x] + 1.0 * (o - a[y, x])
    assert rc.same_bits(got, a[y0:y0 + ny, x0:x0 + nx])


def test_reference_ops_mg_smooth_rb():
    """ops.mg_smooth_rb on CPU tensors (ops/reference.py) against the model; shared storage is refused."""
    import torch

    import mg_rb_cases as rc
    from gpu_mpi_tests_amd import ops

    for h in rc.HS:
        for mask in (0, 15, 6):
            for par in (0, 1):
                for with_f in (False, True):
                    u, o, f, region = rc.fields(h, 37, 9, mask, "fast", with_f)
                    want = rc.reference(h, par, region, mask, u, f, 1.0)
                    x0, nx, y0, ny = region
                    to = torch.from_numpy(o.a)
                    assert ops.mg_smooth_rb(torch.from_numpy(u.a), to, 1.0, region, h, par, mask,
                                            None if f is None else torch.from_numpy(f.a)) is to
                    assert rc.same_bits(o.a[y0:y0 + ny, x0:x0 + nx], want)
                    o.a[y0:y0 + ny, x0:x0 + nx] = rc.SENTINEL
                    assert (o.store == rc.SENTINEL).all()
    tu = torch.from_numpy(u.a)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_smooth_rb(tu, tu, 1.0, region, 2, 0)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_smooth_rb(tu, tu[1:, 2:], 1.0, region, 2, 0)
