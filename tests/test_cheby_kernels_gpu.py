"""gmt_cheby_step on the GPU (csrc/kernels/cheby.hip) against the NumPy model of
tests/cheby_cases.py.

Everything outside u's plus-shaped read set is NaN, everything outside the
region of v and f a sentinel that must be bitwise intact afterwards; u and f
are compared bitwise before and after; v' is bitwise NumPy for the weights 1.0,
1.9 and 0.0 (v' bitwise v).  Widths cover the lane-pair tail and the wave and
workgroup column edges, heights a window shorter than its depth and the segment
seams (L = the rows per segment the path query reports).  Only the all-aligned
variant may take the row walk: the path of every case is asserted."""
import types

import numpy as np
import pytest
import torch

import cheby_cases as hc
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
@pytest.mark.parametrize("nx", hc.NXS)
def test_step_shapes(nx, with_f):
    hc.run_shapes(_impl(), nx, with_f)


def test_empty_regions_and_refusals():
    codes = hc.run_empty_and_refusals(_impl())
    assert codes == [1] * hc.N_REFUSALS, codes  # the CPU backend's codes (tests/test_cheby_kernels_cpu.py)


def _t(field):
    st = torch.from_numpy(field.store).cuda()
    return st[field.off:field.off + field.rows * field.ld].view(field.rows, field.ld)


def test_ops_wrapper():
    """ops.cheby_step and its path query give the C ABI's results; shared storage is refused."""
    for with_f in (False, True):
        u, v, f, region = hc.fields(257, 19, "fast", with_f)
        x0, nx, y0, ny = region
        want = hc.reference(region, u, v, f, 1.9)
        tu, tv = _t(u), _t(v)
        tf = None if f is None else _t(f)
        assert ops.cheby_step_path(tu, tv, region, tf)[0] == ops.PATH_ROW_WALK
        assert ops.cheby_step_path(tu[:, 1:], tv, region, tf) == (ops.PATH_SCALAR, 0)
        assert ops.cheby_step(tu, tv, 1.9, region, tf) is tv
        assert hc.same_bits(tv.cpu().numpy()[y0:y0 + ny, x0:x0 + nx], want)
    with pytest.raises(ValueError, match="share storage"):
        ops.cheby_step(tu, tu, 1.0, region)


def test_rows_4_gib_apart():
    """3 x 5 cells with pitches of 2^28 + 2 (and + 6, + 10) doubles: 32-bit offset
    arithmetic would land elsewhere.  The scalar path (odd first column) and the
    row walk, with and without f."""
    lds = dict(u=(1 << 28) + 2, v=(1 << 28) + 6, f=(1 << 28) + 10)
    ny, nx, W = 3, 5, 12
    rows = ny + 2
    try:
        big = {k: torch.empty((rows - 1) * ld + W, dtype=torch.float64, device="cuda") for k, ld in lds.items()}
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"no room for three 8 GiB allocations: {e}")
    assert all(ny * ld * 8 > 2 ** 32 for ld in lds.values())
    rng = np.random.default_rng(5)
    host = {k: rng.random((rows, W)) - 0.5 for k in lds}  # host copies of the touched part of each row

    def put(k):
        for j in range(rows):
            big[k][j * lds[k]:j * lds[k] + W] = torch.from_numpy(host[k][j]).cuda()

    for k in lds:
        put(k)
    t = {k: torch.as_strided(big[k], (rows, W), (lds[k], 1), 0) for k in lds}
    for x0, path in ((3, ops.PATH_SCALAR), (4, ops.PATH_ROW_WALK)):
        for with_f in (False, True):
            region = (x0, nx, 1, ny)
            tf = t["f"] if with_f else None
            assert ops.cheby_step_path(t["u"], t["v"], region, tf)[0] == path
            ops.cheby_step(t["u"], t["v"], 1.9, region, tf, hc.C0, hc.C1)
            torch.cuda.synchronize()
            U, V = host["u"], host["v"]
            ys, xs = slice(1, 1 + ny), slice(x0, x0 + nx)
            o = hc.C0 * ((U[ys, x0 - 1:x0 - 1 + nx] + U[ys, x0 + 1:x0 + 1 + nx]) + (U[0:ny, xs] + U[2:2 + ny, xs]))
            if with_f:
                o = o + hc.C1 * host["f"][ys, xs]
            pv = V[ys, xs]
            tt = o - pv
            V[ys, xs] = pv + 1.9 * tt
            for k, ld in lds.items():
                for j in range(rows):
                    assert hc.same_bits(big[k][j * ld:j * ld + W].cpu().numpy(), host[k][j]), (x0, with_f, k, j)
