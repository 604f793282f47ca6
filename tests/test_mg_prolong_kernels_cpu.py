"""gmt_mg_prolong_smooth of the CPU backend against the NumPy model of
tests/mg_prolong_cases.py: every mask, mode, parity, width, height and
alignment variant, the identity against the two existing calls, empty regions
and every refusal — the checks of tests/test_mg_prolong_kernels_gpu.py without
the path assertions.  In a child process: build/lib-host/libgmt.so shares its
SONAME with the GPU library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def test_host_mg_prolong_smooth_matches_numpy():
    import mg_prolong_cases as pc

    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mg_prolong_cases.py"), HOST_LIB],
                       capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    want = [4 * pc.N_ALL_MASKS, 4 * pc.N_WIDTHS * 2 * pc.N_SWEEP, sum(pc.n_heights(h) for h in pc.HS),
            4 * pc.N_SCALAR, pc.N_IDENTITIES, 4 * 3 * 3 * 2]
    assert r["ok"] and r["cases"] == want, (r["cases"], want)
    assert r["codes"] == [1] * pc.N_REFUSALS  # hipErrorInvalidValue's number: the GPU test asserts the same list
    assert r["path"] == [0, 0]                # GMT_PATH_NONE: the CPU backend has no kernel to pick
    assert r["geom"] == [[128, 512], [124, 496], [124, 496], [120, 480]]  # the gfx950 kernel's


def _cells(e, u, f, region, par, mask, h, mode, om):
    """The definition cell by cell: u + P e on B0 with the coarse cell of a fine cell from the floor of
    (i - p) / 2, then h sweeps or half-sweeps on the shrinking boxes."""
    import mg_prolong_cases as pc

    x0, nx, y0, ny = region
    gw, ge, gs, gn = (h if mask & b else 0 for b in (1, 2, 4, 8))
    E = e.a
    v = u.a.copy()
    for j in range(-gs, ny + gn):
        for i in range(-gw, nx + ge):
            di, dj = i - par[0], j - par[1]
            I, J = pc.CX0 + di // 2, pc.CY0 + dj // 2
            if di % 2 == 0 and dj % 2 == 0:
                t = E[J, I]
            elif dj % 2 == 0:
                t = 0.5 * (E[J, I] + E[J, I + 1])
            elif di % 2 == 0:
                t = 0.5 * (E[J, I] + E[J + 1, I])
            else:
                t = 0.25 * ((E[J, I] + E[J, I + 1]) + (E[J + 1, I] + E[J + 1, I + 1]))
            v[y0 + j, x0 + i] = v[y0 + j, x0 + i] + t
    for s in range(1, h + 1):
        g = h - s
        bw, be, bs, bn = (g if mask & b else 0 for b in (1, 2, 4, 8))
        n = v.copy()
        for y in range(y0 - bs, y0 + ny + bn):
            for x in range(x0 - bw, x0 + nx + be):
                if mode[0] and ((x - x0) + (y - y0) + mode[1] + (s - 1)) % 2:
                    continue
                o = pc.C0 * ((v[y, x - 1] + v[y, x + 1]) + (v[y - 1, x] + v[y + 1, x]))
                if f is not None:
                    o = o + pc.C1 * f.a[y, x]
                d = o - v[y, x]
                n[y, x] = v[y, x] + om * d
        v = n
    return v[y0:y0 + ny, x0:x0 + nx]


def test_model_cell_by_cell():
    """reference.mg_prolong_smooth (the existing reference functions composed, the interpolation over a moved
    region) against the definition written out cell by cell, for every mask, parity, mode and h."""
    import mg_prolong_cases as pc
    from gpu_mpi_tests_amd.ops import reference as ref

    nx, ny = 6, 5
    for h in pc.HS:
        for mask in range(16):
            for k, par in enumerate(pc.PARITIES):
                mode, with_f = pc.MODES[(mask + k) % 3], bool((mask + k) % 2)
                e, u, _, f, region = pc.fields(h, nx, ny, mask, par, "fast", with_f)
                want = pc.reference(h, mode, region, par, mask, e, u, f, 0.8)
                got = _cells(e, u, f, region, par, mask, h, mode, 0.8)
                assert pc.same_bits(got, want), (h, mask, par, mode, with_f)
    x0, _, y0, _ = region
    for bad in (dict(h=5), dict(h=0), dict(rb=2), dict(par=2), dict(halo_mask=16)):
        kw = dict(dict(h=2, rb=0, par=0, halo_mask=0), **bad)
        with pytest.raises(ValueError):
            ref.mg_prolong_smooth(e.a, u.a, np.zeros(u.a.shape), 0.8, x0, nx, y0, ny, 1, 1, pc.CX0, pc.CY0, **kw)
    with pytest.raises(ValueError):
        ref.mg_prolong_smooth(e.a, u.a, np.zeros(u.a.shape), 0.8, x0, nx, y0, ny, 2, 1, pc.CX0, pc.CY0, 2)


def test_reference_ops_mg_prolong_smooth():
    """ops.mg_prolong_smooth on CPU tensors (ops/reference.py) against the model; shared storage is refused."""
    import torch

    import mg_prolong_cases as pc
    from gpu_mpi_tests_amd import ops

    for h in pc.HS:
        for k, mask in enumerate((0, 15, 6)):
            for m, mode in enumerate(pc.MODES):
                par, with_f = pc.PARITIES[(k + m) % 4], bool((k + m) % 2)
                e, u, o, f, region = pc.fields(h, 37, 9, mask, par, "fast", with_f)
                x0, nx, y0, ny = region
                want = pc.reference(h, mode, region, par, mask, e, u, f, 0.8)
                to = torch.from_numpy(o.a)
                assert ops.mg_prolong_smooth(torch.from_numpy(e.a), torch.from_numpy(u.a), to, 0.8, region, par,
                                             (pc.CX0, pc.CY0), h, mode[0], mode[1], mask,
                                             None if f is None else torch.from_numpy(f.a), pc.C0, pc.C1) is to
                assert pc.same_bits(o.a[y0:y0 + ny, x0:x0 + nx], want)
                o.a[y0:y0 + ny, x0:x0 + nx] = pc.SENTINEL
                assert (o.store == pc.SENTINEL).all()
    te, tu = torch.from_numpy(e.a), torch.from_numpy(u.a)
    for bad in (dict(out=tu), dict(out=te), dict(f=to)):
        kw = dict(dict(out=to, f=None), **bad)
        with pytest.raises(ValueError, match="share storage"):
            ops.mg_prolong_smooth(te, tu, kw["out"], 0.8, region, par, (pc.CX0, pc.CY0), h, f=kw["f"])
