"""The table-driven multigrid transfers (gmt_mg_xfer_plan_create,
gmt_mg_restrict_tab, gmt_mg_prolong_add_tab) of the CPU backend against the
NumPy model of tests/mg_tab_cases.py: every axis pair, region, height and
alignment variant, refused descriptions, empty regions and every refused launch
— the checks of tests/test_mg_tab_kernels_gpu.py without the path assertions.
In a child process: build/lib-host/libgmt.so shares its SONAME with the GPU
library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def test_case_set_covers_what_it_must():
    import mg_tab_cases as tc

    tc.assert_coverage()
    # 100 % of the listed cases: the counts the backends must report
    assert sum(tc.n_cases(xp) for xp in tc.X_AXES) == len(tc.X_AXES) * 6 * len(tc.y_regions())
    assert tc.n_cases(tc.WIDE) == 6 * len(tc.y_regions(tc.WIDE_NYS))


def test_host_tab_kernels_match_numpy():
    import mg_tab_cases as tc

    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mg_tab_cases.py"), HOST_LIB],
                       capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    total = sum(tc.n_cases(xp) for xp in tc.X_AXES + (tc.WIDE,))
    assert r["ok"] and r["cases"] == [total * len(tc.ALIGN_R), total * len(tc.ALIGN_P)], r["cases"]
    assert r["codes"] == [1] * tc.N_REFUSALS  # hipErrorInvalidValue's number: the GPU test asserts the same list
    assert r["paths"] == [0, 0]               # GMT_PATH_NONE: the CPU backend has no kernel to pick


def test_model_cell_by_cell():
    """The vectorised models of mg_tab_cases against the definition written out cell by cell in Python floats."""
    import mg_tab_cases as tc

    for xa, ya in ((tc.share(22, 10, 7, 8), tc.share(22, 10, 0, 5)), (tc.share(15, 7, 5, 5), tc.share(10, 4, 3, 7)),
                   (tc.share(6, 2, 0, 6), tc.share(15, 7, 3, 9))):
        (nx_g, mx_g, fox, nx, cox, mx), (ny_g, my_g, foy, ny, coy, my) = xa, ya
        finex, tapsx = tc.axis_model(nx_g, mx_g)
        finey, tapsy = tc.axis_model(ny_g, my_g)
        d, _, (x0, y0), _, (mx_, my_) = tc.restrict_fields(xa, ya, "fast")
        got = tc.restrict_reference(d, (x0, y0), mx_, my_)
        D = d.a
        for J in range(my):
            for I in range(mx):
                hs = []
                for gj, _ in tapsy[coy + 1 + J]:
                    row = D[y0 + gj - (foy + 1)]
                    v = [w * float(row[x0 + gi - (fox + 1)]) for gi, w in tapsx[cox + 1 + I]]
                    h = (v[0] + v[1]) + v[2]
                    hs.append(h + v[3] if len(v) == 4 else h)
                v = [w * h for (_, w), h in zip(tapsy[coy + 1 + J], hs)]
                s = (v[0] + v[1]) + v[2]
                assert got[J, I] == (s + v[3] if len(v) == 4 else s), (xa, ya, J, I)
        e, u, (x0, y0), (cx0, cy0), (mx_, my_) = tc.prolong_fields(xa, ya, "fast")
        got = tc.prolong_reference(e, u, (x0, y0), (cx0, cy0), mx_, my_)
        E, U = e.a, u.a
        for j in range(ny):
            for i in range(nx):
                (qx, tx), (qy, ty) = finex[fox + 1 + i], finey[foy + 1 + j]
                I, J = cx0 + qx - (cox + 1), cy0 + qy - (coy + 1)
                bot = (1.0 - tx) * float(E[J, I]) + tx * float(E[J, I + 1])
                top = (1.0 - tx) * float(E[J + 1, I]) + tx * float(E[J + 1, I + 1])
                assert got[j, i] == float(U[y0 + j, x0 + i]) + ((1.0 - ty) * bot + ty * top), (xa, ya, j, i)


def test_reference_ops_mg_tab():
    """ops.mg_*_tab on CPU tensors (ops/reference.py) against the model; refused descriptions and shared storage."""
    import torch

    import mg_tab_cases as tc
    from gpu_mpi_tests_amd import ops

    for xa, ya in [(xa, ya) for xp in ((22, 10), (46, 22), (15, 7)) for xa in tc.x_regions(*xp)
                   for ya in tc.y_regions((1, 4, 9))] + tc.case_list(tc.WIDE)[::5]:
        d, s, origin, coarse, (mx_, my_) = tc.restrict_fields(xa, ya, "fast")
        want = tc.restrict_reference(d, origin, mx_, my_)
        ts = torch.from_numpy(s.a)
        assert ops.mg_restrict_tab(torch.from_numpy(d.a), ts, xa, ya, origin, coarse) is ts
        (cx0, cy0), mx, my = coarse, xa[5], ya[5]
        assert tc.same_bits(s.a[cy0:cy0 + my, cx0:cx0 + mx], want), (xa, ya)
        s.a[cy0:cy0 + my, cx0:cx0 + mx] = tc.SENTINEL
        assert (s.store == tc.SENTINEL).all()
        e, u, origin, coarse, (mx_, my_) = tc.prolong_fields(xa, ya, "fast")
        want = tc.prolong_reference(e, u, origin, coarse, mx_, my_)
        tu = torch.from_numpy(u.a)
        assert ops.mg_prolong_add_tab(torch.from_numpy(e.a), tu, xa, ya, origin, coarse) is tu
        (x0, y0), nx, ny = origin, xa[3], ya[3]
        assert tc.same_bits(u.a[y0:y0 + ny, x0:x0 + nx], want), (xa, ya)
    t = torch.zeros(40, 40, dtype=torch.float64)
    for xa, ya in tc.BAD_DESCS:
        with pytest.raises(ValueError):
            ops.mg_restrict_tab(t, torch.zeros(40, 40, dtype=torch.float64), xa, ya, (2, 2), (1, 1))
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_prolong_add_tab(t, t, tc.share(22, 10, 0, 22), tc.share(22, 10, 0, 22), (1, 1), (1, 1))
    assert np.isfinite(t.numpy()).all()
