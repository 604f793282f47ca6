"""gmt_mg_resid_restrict on the GPU (csrc/kernels/mg.hip) against the NumPy
model of tests/mg_resid_cases.py.

Everything outside the read sets of u and f is NaN, sc a sentinel outside its
mx x my cells that must be bitwise intact afterwards; inputs are compared
bitwise before and after; sc is bitwise reference.mg_resid_restrict.  Widths
(from gmt_mg_resid_restrict_geom) cover the lane-pair tail and the seams
between waves and workgroups, where neighbouring waves overlap; heights the
regions shorter than the warm-up and the segment seams (L = the rows per
segment the path query reports).  Only the all-aligned variant may take the
walk: the path of every case is asserted."""
import types

import numpy as np
import pytest
import torch

import mg_resid_cases as rc
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


def test_geometry():
    assert rc.geom(_impl()) == (124, 496) and ops.mg_resid_restrict_geom() == ops.mg_smooth_k_geom(2)


def test_all_masks():
    assert rc.run_all_masks(_impl()) == rc.N_ALL_MASKS


@pytest.mark.parametrize("iw", range(9))
def test_widths(iw):
    impl = _impl()
    assert rc.run_width(impl, rc.widths(impl)[iw]) == 2 * rc.N_SWEEP


@pytest.mark.parametrize("ih", range(rc.N_HEIGHTS))
def test_heights(ih):
    assert rc.run_height(_impl(), ih) == 2 * rc.N_SWEEP


def test_scalar_shapes():
    assert rc.run_scalar_shapes(_impl()) == rc.N_SCALAR


def test_identities():
    assert rc.run_identities(_impl()) == 64


def test_empty_regions_and_refusals():
    codes = rc.run_empty_and_refusals(_impl())
    assert codes == [1] * rc.N_REFUSALS, codes  # the CPU backend's codes (tests/test_mg_resid_kernels_cpu.py)


def _t(field):
    st = torch.from_numpy(field.store).cuda()
    return st[field.off:field.off + field.rows * field.ld].view(field.rows, field.ld)


def test_ops_wrappers():
    """ops.mg_resid_restrict and its queries give the C ABI's results; shared storage is refused."""
    for with_f in (False, True):
        for par in rc.PARITIES:
            u, s, f, region, coarse = rc.fields(257, 19, 15, par, "fast", with_f)
            cx0, cy0, mx, my = coarse
            want = rc.reference(region, par, 15, coarse, u, f)
            tu, ts = _t(u), _t(s)
            tf = None if f is None else _t(f)
            path, seg = ops.mg_resid_restrict_path(tu, ts, region, par, (cx0, cy0), 15, tf)
            assert path == ops.PATH_ROW_WALK and seg == rc.seg_rows(_impl(), 257)
            assert ops.mg_resid_restrict_path(tu[:, 1:], ts, region, par, (cx0, cy0), 15, tf) == (ops.PATH_SCALAR, 0)
            assert ops.mg_resid_restrict(tu, ts, region, par, (cx0, cy0), 15, tf) is ts
            assert rc.same_bits(ts.cpu().numpy()[cy0:cy0 + my, cx0:cx0 + mx], want)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_resid_restrict(tu, tu, region, par, (cx0, cy0))


def test_rows_4_gib_apart():
    """5 x 4 cells of a field whose rows are 2^28 + 2 doubles apart: 32-bit offset arithmetic would land
    elsewhere.  The one-lane-per-coarse-cell kernel (odd first column) and the walk, with halo rows below and
    above (mask S + N), so the far rows are read."""
    ld = (1 << 28) + 2
    ny, nx, W = 4, 5, 12
    rows = ny + 4
    try:
        big = torch.empty((rows - 1) * ld + W, dtype=torch.float64, device="cuda")
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"no room for an allocation of 15 GiB: {e}")
    assert ny * ld * 8 > 2 ** 32
    rng = np.random.default_rng(5)
    host = rng.random((rows, W)) - 0.5  # the host copy of the touched part of each row
    for j in range(rows):
        big[j * ld:j * ld + W] = torch.from_numpy(host[j]).cuda()
    tu = torch.as_strided(big, (rows, W), (ld, 1), 0)
    from gpu_mpi_tests_amd.ops import reference as ref

    for x0, fast in ((3, False), (4, True)):
        region = (x0, nx, 2, ny)
        for par in rc.PARITIES:
            ts = torch.full((4, 8), rc.SENTINEL, dtype=torch.float64, device="cuda")
            want = np.full((4, 8), rc.SENTINEL)
            assert ops.mg_resid_restrict_path(tu, ts, region, par, (2, 1), 12)[0] == \
                (ops.PATH_ROW_WALK if fast else ops.PATH_SCALAR)
            ops.mg_resid_restrict(tu, ts, region, par, (2, 1), 12, None, rc.C0, rc.C1, rc.CS)
            ref.mg_resid_restrict(host, want, rc.CS, x0, nx, 2, ny, par[0], par[1], 12, 2, 1, None, rc.C0, rc.C1)
            assert rc.same_bits(ts.cpu().numpy(), want), (x0, par)
    torch.cuda.synchronize()
    for j in range(rows):
        assert rc.same_bits(big[j * ld:j * ld + W].cpu().numpy(), host[j]), j
