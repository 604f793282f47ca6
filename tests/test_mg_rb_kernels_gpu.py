"""gmt_mg_smooth_rb on the GPU (csrc/kernels/mg.hip) against the NumPy model of
tests/mg_rb_cases.py.

Everything outside the read sets of u and f is NaN, everything outside out[R] a
sentinel that must be bitwise intact afterwards; inputs are compared bitwise
before and after; out[R] is bitwise reference.mg_smooth_rb.  Widths (from
gmt_mg_smooth_k_geom(h)) cover the lane-pair tail and the seams between waves
and workgroups; heights a region shorter than the warm-up and the segment seams
(L = the rows per segment the path query reports); h = 1..4, both colour phases.
Only the all-aligned variant may take the walk: the path of every case is
asserted."""
import types

import numpy as np
import pytest
import torch

import mg_rb_cases as rc
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


@pytest.mark.parametrize("iw", range(11))
@pytest.mark.parametrize("h", rc.HS)
def test_fast_shapes(h, iw):
    impl = _impl()
    assert rc.run_fast_shapes(impl, h, rc.widths(impl, h)[iw]) > 0


@pytest.mark.parametrize("h", rc.HS)
def test_scalar_shapes(h):
    assert rc.run_scalar_shapes(_impl(), h) == rc.n_scalar()


@pytest.mark.parametrize("h", rc.HS)
def test_all_masks(h):
    assert rc.run_all_masks(_impl(), h) == rc.N_ALL_MASKS


def test_identities():
    rc.run_identities(_impl())


def test_empty_regions_and_refusals():
    codes = rc.run_empty_and_refusals(_impl())
    assert codes == [1] * rc.N_REFUSALS, codes  # the CPU backend's codes (tests/test_mg_rb_kernels_cpu.py)


def _t(field):
    st = torch.from_numpy(field.store).cuda()
    return st[field.off:field.off + field.rows * field.ld].view(field.rows, field.ld)


def test_ops_wrappers():
    """ops.mg_smooth_rb and its path query give the C ABI's results; shared storage is refused."""
    impl = _impl()
    for h in rc.HS:
        for with_f in (False, True):
            for par in (0, 1):
                u, o, f, region = rc.fields(h, 257, 19, 15, "fast", with_f)
                x0, nx, y0, ny = region
                want = rc.reference(h, par, region, 15, u, f, 1.0)
                tu, to = _t(u), _t(o)
                tf = None if f is None else _t(f)
                path, seg = ops.mg_smooth_rb_path(tu, to, region, h, par, 15, tf)
                assert path == ops.PATH_ROW_WALK and seg == rc.seg_rows(impl, h, nx)
                assert ops.mg_smooth_rb_path(tu[:, 1:], to, region, h, par, 15, tf) == (ops.PATH_SCALAR, 0)
                assert ops.mg_smooth_rb(tu, to, 1.0, region, h, par, 15, tf) is to
                assert rc.same_bits(to.cpu().numpy()[y0:y0 + ny, x0:x0 + nx], want)
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_smooth_rb(tu, tu, 1.0, region, 2, 0)
    with pytest.raises(_native.NativeError):  # par outside 0..1: the C ABI's refusal
        ops.mg_smooth_rb(tu, to, 1.0, region, 2, 2)
