"""gmt_mg_smooth_k on the GPU (csrc/kernels/mg.hip) against the NumPy model of
tests/mg_fuse_cases.py.

Everything outside the read sets of u and f is NaN, everything outside out[R] a
sentinel that must be bitwise intact afterwards; inputs are compared bitwise
before and after; out[R] is bitwise reference.mg_smooth_k.  Widths (from
gmt_mg_smooth_k_geom) cover the lane-pair tail and the seams between waves and
workgroups, where neighbouring waves overlap; heights a region shorter than the
warm-up and the segment seams (L = the rows per segment the path query
reports).  Only the all-aligned variant may take the fused walk: the path of
every case is asserted."""
import types

import numpy as np
import pytest
import torch

import mg_fuse_cases as fc
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
    assert [fc.geom(_impl(), k) for k in fc.KS] == [(124, 496), (124, 496), (120, 480)]
    assert ops.mg_smooth_k_geom(1) == (128, 512) and ops.mg_smooth_k_geom(4) == (120, 480)
    with pytest.raises(ValueError):
        ops.mg_smooth_k_geom(5)


@pytest.mark.parametrize("iw", range(11))
@pytest.mark.parametrize("k", fc.KS)
def test_fast_shapes(k, iw):
    impl = _impl()
    assert fc.run_fast_shapes(impl, k, fc.widths(impl, k)[iw]) > 0


@pytest.mark.parametrize("k", fc.KS)
def test_scalar_shapes(k):
    assert fc.run_scalar_shapes(_impl(), k) == fc.n_scalar()


@pytest.mark.parametrize("k", fc.KS)
def test_all_masks(k):
    assert fc.run_all_masks(_impl(), k) == fc.N_ALL_MASKS


def test_identities():
    fc.run_identities(_impl())


def test_empty_regions_and_refusals():
    codes = fc.run_empty_and_refusals(_impl())
    assert codes == [1] * fc.N_REFUSALS, codes  # the CPU backend's codes (tests/test_mg_fuse_kernels_cpu.py)


def _t(field):
    st = torch.from_numpy(field.store).cuda()
    return st[field.off:field.off + field.rows * field.ld].view(field.rows, field.ld)


def test_ops_wrappers():
    """ops.mg_smooth_k and its queries give the C ABI's results; shared storage is refused."""
    for k in fc.KS:
        for with_f in (False, True):
            u, o, f, region = fc.fields(k, 257, 19, 15, "fast", with_f)
            x0, nx, y0, ny = region
            want = fc.reference(k, region, 15, u, f, 0.8)
            tu, to = _t(u), _t(o)
            tf = None if f is None else _t(f)
            path, seg = ops.mg_smooth_k_path(tu, to, region, k, 15, tf)
            assert path == ops.PATH_ROW_WALK and seg == fc.seg_rows(_impl(), k, nx)
            assert ops.mg_smooth_k_path(tu[:, 1:], to, region, k, 15, tf) == (ops.PATH_SCALAR, 0)
            assert ops.mg_smooth_k(tu, to, 0.8, region, k, 15, tf) is to
            assert fc.same_bits(to.cpu().numpy()[y0:y0 + ny, x0:x0 + nx], want)
    # k = 1 is the single sweep
    u, o, f, region = fc.fields(1, 130, 9, 0, "fast", True)
    x0, nx, y0, ny = region
    tu, to, tf = _t(u), _t(o), _t(f)
    assert ops.mg_smooth_k_path(tu, to, region, 1, 0, tf) == ops.mg_smooth_path(tu, to, region, tf)
    ops.mg_smooth_k(tu, to, 0.8, region, 1, 0, tf)
    assert fc.same_bits(to.cpu().numpy()[y0:y0 + ny, x0:x0 + nx], fc.reference(1, region, 0, u, f, 0.8))
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_smooth_k(tu, tu, 0.8, region, 2)


def test_rows_4_gib_apart():
    """3 x 5 cells in fields whose rows are 2^28 + 2 (and + 6) doubles apart: 32-bit offset arithmetic would
    land elsewhere.  The one-lane-per-cell kernel (odd first column) and the fused walk, k = 2, with halo rows
    below and above (mask S + N), so the far rows are read."""
    lds = dict(a=(1 << 28) + 2, b=(1 << 28) + 6)
    k, ny, nx, W = 2, 3, 5, 12
    rows = ny + 2 * k
    try:
        big = {n: torch.empty((rows - 1) * ld + W, dtype=torch.float64, device="cuda") for n, ld in lds.items()}
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"no room for two allocations of 12 and more GiB: {e}")
    assert all(ny * ld * 8 > 2 ** 32 for ld in lds.values())
    rng = np.random.default_rng(5)
    host = {n: rng.random((rows, W)) - 0.5 for n in lds}  # host copies of the touched part of each row
    for n in lds:
        for j in range(rows):
            big[n][j * lds[n]:j * lds[n] + W] = torch.from_numpy(host[n][j]).cuda()
    t = {n: torch.as_strided(big[n], (rows, W), (lds[n], 1), 0) for n in lds}
    for x0, fast in ((3, False), (4, True)):
        region = (x0, nx, k, ny)
        assert ops.mg_smooth_k_path(t["a"], t["b"], region, k, 12)[0] == (ops.PATH_ROW_WALK if fast else ops.PATH_SCALAR)
        ops.mg_smooth_k(t["a"], t["b"], 0.8, region, k, 12, None, fc.C0, fc.C1)
        from gpu_mpi_tests_amd.ops import reference as ref

        ref.mg_smooth_k(host["a"], host["b"], 0.8, x0, nx, k, ny, k, 12, None, fc.C0, fc.C1)
        torch.cuda.synchronize()
        for n, ld in lds.items():
            for j in range(rows):
                assert fc.same_bits(big[n][j * ld:j * ld + W].cpu().numpy(), host[n][j]), (x0, n, j)
