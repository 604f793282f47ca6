"""gmt_jacobi5_resid on the GPU (csrc/kernels/jacobi5_resid.hip) against a
NumPy fp64 reference with math.fsum (tests/resid_cases.py).

Every cell outside the region's plus-shaped read set is NaN, u is compared
bitwise before and after each call, and a canary follows the declared
workspace.  Widths cover the lane-pair tail and the wave and workgroup column
edges; heights a window shorter than its depth and the segment seams (L = the
rows per segment the path query reports for that width).  x0 = 8 with an even
pitch must take the row walk; an odd x0, an odd pitch or a base off by 8 B
the scalar kernel.

out[0]: |got - ref| <= 1e-11 * max(1, ref), the tolerance of the same sum in
test_kernels_gpu.test_jacobi5.  out[1]: bitwise NumPy's max |d| without f (the
cell has no contractible multiply-add), 1e-14 relative with f."""
import math

import numpy as np
import pytest
import torch

import resid_cases as rc
from gpu_mpi_tests_amd import _native, ops

pytestmark = pytest.mark.gpu
CANARY = 12345.0


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _dev(case):
    """The case's fields on the device, at the same offsets from an aligned base."""
    st = torch.from_numpy(case["store"]).cuda()
    u = st[case["off"]:case["off"] + case["rows"] * case["ld"]].view(case["rows"], case["ld"])
    f = None
    if case["fstore"] is not None:
        f = torch.from_numpy(case["fstore"]).cuda().view(case["rows"], case["ldf"])
    return st, u, f


def call(case):
    L = _native.lib()
    st, u, f = _dev(case)
    before = st.clone()
    x0, nx, y0, ny = case["region"]
    n = int(L.gmt_jacobi5_resid_workspace(nx, ny))
    ws = torch.full((n + 8,), CANARY, dtype=torch.float64, device="cuda")
    out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    _native.check(L.gmt_jacobi5_resid(x0, nx, y0, ny, u.data_ptr(), u.stride(0), f.data_ptr() if f is not None else 0,
                                      f.stride(0) if f is not None else 0, rc.C0, rc.C1 if f is not None else 0.0,
                                      out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "gmt_jacobi5_resid")
    o = out.cpu()
    assert torch.equal(before.view(torch.int64), st.view(torch.int64))  # u is never written
    assert bool((ws[n:] == CANARY).all())                               # nor anything past the workspace
    # the torch-facing wrapper gives the same two numbers
    w = ops.jacobi5_resid(u, case["region"], f, rc.C0, rc.C1 if f is not None else 0.0).cpu()
    assert w.dtype == torch.float64 and w.shape == (2,)
    assert torch.equal(w.view(torch.int64), o.view(torch.int64)) or (math.isnan(float(o[0])) and math.isnan(float(w[0])))
    return float(o[0]), float(o[1])


def path(case):
    _, u, f = _dev(case)
    p, seg = ops.jacobi5_resid_path(u, case["region"], f)
    assert p in (ops.PATH_ROW_WALK, ops.PATH_SCALAR)
    return p == ops.PATH_ROW_WALK, seg


def seg_rows(nx):
    case = rc.make_case(nx, 1)
    walk, seg = path(case)
    assert walk and seg >= 2
    return seg


def test_path_enumerator():
    assert ops.PATH_ROW_WALK == 5 and (ops.PATH_NONE, ops.PATH_SCALAR, ops.PATH_PT) == (0, 1, 2)


@pytest.mark.parametrize("with_f", [False, True])
@pytest.mark.parametrize("nx", rc.NXS)
def test_shapes(nx, with_f):
    rc.run_shapes(call, 1e-11, nx, with_f, seg_rows, path)


@pytest.mark.parametrize("align", ["walk", "odd_x0"])
def test_spike_is_the_reported_max(align):
    L = seg_rows(300)
    rc.run_spikes(call, 300, 2 * L + 1, L, align)


@pytest.mark.parametrize("align", ["walk", "odd_ld"])
def test_nan_gives_inf(align):
    rc.run_nan(call, 130, 2 * seg_rows(130) + 1, align)


def test_empty_region():
    rc.run_empty(call)


def test_two_level_reduction_2000x4000():
    """2000 rows x 4000 columns: more partials than one reduction block
    takes.  1e-10 relative; two calls bitwise equal; equal to the residual of
    gmt_jacobi5 on the same field within the same tolerance."""
    case = rc.make_case(4000, 2000, seed=5)
    walk, seg = path(case)
    assert walk
    x0, nx, y0, ny = case["region"]
    assert ((nx + 511) // 512) * ((ny + seg - 1) // seg) > 1024  # beyond the one-block reduction
    s, m, _ = rc.reference(case)
    got = call(case)
    assert abs(got[0] - s) <= 1e-10 * s and got[1] == m, (got, s, m)
    assert call(case) == got
    _, u, _ = _dev(case)
    un = torch.zeros_like(u)
    r = float(ops.jacobi5(u, un, case["region"], resid=True))
    assert abs(r - s) <= 1e-10 * s and abs(r - got[0]) <= 1e-10 * s, (r, got, s)
