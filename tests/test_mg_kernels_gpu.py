"""gmt_mg_smooth, gmt_mg_restrict and gmt_mg_prolong_add on the GPU
(csrc/kernels/mg.hip) against the NumPy model of tests/mg_cases.py.

Everything outside a kernel's read set is NaN, everything outside its output
region a sentinel that must be bitwise intact afterwards; inputs are compared
bitwise before and after; outputs are bitwise NumPy.  Widths cover the
lane-pair tail and the wave and workgroup column edges; the smoother's heights
a window shorter than its depth and the segment seams (L = the rows per segment
the path query reports); the transfer kernels every (px, py), so the last fine
column both is and is not a coarse point.  Only the all-aligned variant may
take the fast path: the path of every case is asserted."""
import types

import numpy as np
import pytest
import torch

import mg_cases as mc
from gpu_mpi_tests_amd import _native, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _impl():
    return types.SimpleNamespace(lib=_native.lib(), has_paths=True, stream=torch.cuda.current_stream().cuda_stream,
                                 upload=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(),
                                 download=lambda t: t.cpu().numpy(), ptr=lambda t: t.data_ptr())


@pytest.mark.parametrize("with_f", [False, True])
@pytest.mark.parametrize("nx", mc.NXS)
def test_smooth_shapes(nx, with_f):
    mc.run_smooth_shapes(_impl(), nx, with_f)


@pytest.mark.parametrize("nx", mc.NXS)
def test_restrict_shapes(nx):
    mc.run_restrict_shapes(_impl(), nx)


@pytest.mark.parametrize("nx", mc.NXS)
def test_prolong_shapes(nx):
    mc.run_prolong_shapes(_impl(), nx)


def test_identities():
    mc.run_identities(_impl())


def test_empty_regions_and_refusals():
    codes = mc.run_empty_and_refusals(_impl())
    assert codes == [1] * mc.N_REFUSALS, codes  # the CPU backend's codes (tests/test_mg_kernels_cpu.py)


def _t(field):
    st = torch.from_numpy(field.store).cuda()
    return st[field.off:field.off + field.rows * field.ld].view(field.rows, field.ld)


def test_ops_wrappers():
    """ops.mg_* and their path queries give the C ABI's results; shared storage is refused."""
    for with_f in (False, True):
        u, o, f, region = mc.smooth_fields(257, 19, "fast", with_f)
        x0, nx, y0, ny = region
        want = mc.smooth_reference(region, u, f, 0.8)
        tu, to = _t(u), _t(o)
        tf = None if f is None else _t(f)
        assert ops.mg_smooth_path(tu, to, region, tf)[0] == ops.PATH_ROW_WALK
        assert ops.mg_smooth_path(tu[:, 1:], to, region, tf) == (ops.PATH_SCALAR, 0)
        assert ops.mg_smooth(tu, to, 0.8, region, tf) is to
        assert mc.same_bits(to.cpu().numpy()[y0:y0 + ny, x0:x0 + nx], want)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_smooth(tu, tu, 0.8, region)
    for px, py in mc.PARITIES:
        d, s, region, (cx0, cy0), (mx, my) = mc.restrict_fields(257, 9, px, py, "fast")
        want = mc.restrict_reference(d, region, px, py, mx, my)
        td, ts = _t(d), _t(s)
        assert ops.mg_restrict_path(td, ts, region, (cx0, cy0)) == ops.PATH_PT
        assert ops.mg_restrict_path(td, ts, region, (cx0 + 1, cy0)) == ops.PATH_SCALAR
        assert ops.mg_restrict(td, ts, region, (px, py), (cx0, cy0)) is ts
        assert mc.same_bits(ts.cpu().numpy()[cy0:cy0 + my, cx0:cx0 + mx], want)
        e, u, region, coarse = mc.prolong_fields(257, 9, px, py, "fast")
        x0, nx, y0, ny = region
        want = mc.prolong_reference(e, u, region, px, py, coarse)
        te, tu = _t(e), _t(u)
        assert ops.mg_prolong_add_path(te, tu, region) == ops.PATH_PT
        assert ops.mg_prolong_add_path(te, tu[:, 1:], region) == ops.PATH_SCALAR
        assert ops.mg_prolong_add(te, tu, region, (px, py), coarse) is tu
        assert mc.same_bits(tu.cpu().numpy()[y0:y0 + ny, x0:x0 + nx], want)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_prolong_add(tu, tu, region, (1, 1), (1, 1))


def test_rows_4_gib_apart():
    """3 x 5 fine cells in fields whose rows are 2^28 + 2 (and + 6) doubles apart: 32-bit offset
    arithmetic would land elsewhere.  Every kernel on its scalar path (odd first column) and its
    fast path; the small side of a transfer (2 x 3 coarse cells with their ring) has short rows."""
    lds = dict(a=(1 << 28) + 2, b=(1 << 28) + 6)
    ny, nx, W = 3, 5, 12
    rows = ny + 2
    try:
        big = {k: torch.empty((rows - 1) * ld + W, dtype=torch.float64, device="cuda") for k, ld in lds.items()}
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"no room for two 8 GiB allocations: {e}")
    assert all(ny * ld * 8 > 2 ** 32 for ld in lds.values())
    rng = np.random.default_rng(5)
    host = {k: rng.random((rows, W)) - 0.5 for k in lds}  # host copies of the touched part of each row
    for k in lds:
        for j in range(rows):
            big[k][j * lds[k]:j * lds[k] + W] = torch.from_numpy(host[k][j]).cuda()
    t = {k: torch.as_strided(big[k], (rows, W), (lds[k], 1), 0) for k in lds}
    A, B = host["a"], host["b"]
    small = rng.random((4, 8)) - 0.5           # the coarse field of either transfer
    ts = small.copy()

    def rows_equal(what):
        for k, ld in lds.items():
            for j in range(rows):
                assert mc.same_bits(big[k][j * ld:j * ld + W].cpu().numpy(), host[k][j]), (what, k, j)

    for x0, fast in ((3, False), (4, True)):
        region = (x0, nx, 1, ny)
        ys, xs = slice(1, 1 + ny), slice(x0, x0 + nx)
        # smoother: a -> b
        assert ops.mg_smooth_path(t["a"], t["b"], region)[0] == (ops.PATH_ROW_WALK if fast else ops.PATH_SCALAR)
        ops.mg_smooth(t["a"], t["b"], 0.8, region, None, mc.C0, mc.C1)
        o = mc.C0 * ((A[ys, x0 - 1:x0 - 1 + nx] + A[ys, x0 + 1:x0 + 1 + nx]) + (A[0:ny, xs] + A[2:2 + ny, xs]))
        tt = o - A[ys, xs]
        B[ys, xs] = A[ys, xs] + 0.8 * tt
        torch.cuda.synchronize()
        rows_equal(("smooth", x0))
        for px, py in ((1, 1), (0, 0)):
            mx, my = mc.coarse_extent(nx, px), mc.coarse_extent(ny, py)
            # restriction: a -> the small field at (2, 1)
            dev = torch.from_numpy(ts).cuda()
            assert ops.mg_restrict_path(t["a"], dev, region, (2, 1)) == (ops.PATH_PT if fast else ops.PATH_SCALAR)
            ops.mg_restrict(t["a"], dev, region, (px, py), (2, 1), mc.CS)
            cols = x0 + px + 2 * np.arange(mx)
            for J in range(my):
                y = 1 + py + 2 * J
                H = [(A[r, cols - 1] + A[r, cols + 1]) + 2.0 * A[r, cols] for r in (y - 1, y, y + 1)]
                ts[1 + J, 2:2 + mx] = mc.CS * ((H[0] + H[2]) + 2.0 * H[1])
            assert mc.same_bits(dev.cpu().numpy(), ts), ("restrict", x0, px, py)
            # interpolation: the small field (cells at (2, 1), ring around them) -> b
            e = types.SimpleNamespace(a=small)
            u = types.SimpleNamespace(a=B)
            want = mc.prolong_reference(e, u, region, px, py, (2, 1))
            dev = torch.from_numpy(small).cuda()
            assert ops.mg_prolong_add_path(dev, t["b"], region) == (ops.PATH_PT if fast else ops.PATH_SCALAR)
            ops.mg_prolong_add(dev, t["b"], region, (px, py), (2, 1))
            B[ys, xs] = want
            torch.cuda.synchronize()
            rows_equal(("prolong", x0, px, py))
