"""gmt_cg_apply / gmt_cg_update / gmt_cg_dir on the GPU (csrc/kernels/cg.hip)
against the NumPy model of tests/cg_cases.py (math.fsum for the sums).

apply: everything outside p's plus-shaped read set is NaN, q's surroundings are
a sentinel, p is compared bitwise before and after, a canary follows the
declared workspace; q is bitwise NumPy in both modes, mode 1 also bitwise the d
of resid_cases.reference.  update / dir: x, r, p bitwise NumPy, every cell
outside the region bitwise untouched, the zero-coefficient denominators (0,
negative, NaN) leave the fields alone.  Widths cover the lane-pair tail and the
wave and workgroup column edges; apply's heights a window shorter than its depth
and the segment seams (L = the rows per segment the path query reports), the
streaming kernels' the rows one block takes.  Only the all-aligned variant may
take the row walk / the pair path: the path of every case is asserted.

Sums: |got - ref| <= 1e-11 * max(1, sum of the terms' magnitudes), the tolerance
test_resid_gpu.py passes for the same kind of sum.  Maxima: bitwise."""
import math
import types

import numpy as np
import pytest
import torch

import cg_cases as cc
from gpu_mpi_tests_amd import _native, ops

pytestmark = pytest.mark.gpu
TOL_SUM = 1e-11


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _impl():
    return types.SimpleNamespace(lib=_native.lib(), has_paths=True, stream=torch.cuda.current_stream().cuda_stream,
                                 upload=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(),
                                 download=lambda t: t.cpu().numpy(), ptr=lambda t: t.data_ptr())


@pytest.mark.parametrize("mode,with_f", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("nx", cc.NXS)
def test_apply_shapes(nx, mode, with_f):
    cc.run_apply_shapes(_impl(), TOL_SUM, nx, mode, with_f)


@pytest.mark.parametrize("nx", cc.NXS)
def test_update_and_dir_shapes(nx):
    cc.run_stream_shapes(_impl(), TOL_SUM, nx)


def test_zero_coefficients_and_nan_cells():
    cc.run_coefs(_impl(), TOL_SUM)


def test_apply_nan_gives_inf():
    impl = _impl()
    cc.run_apply_nan(impl, 130, 2 * cc.seg_rows(impl, 130) + 1)


def test_empty_regions_and_refusals():
    codes = cc.run_empty_and_refusals(_impl())
    assert codes == [1] * len(codes), codes  # the CPU backend's codes (tests/test_cg_kernels_cpu.py)
    from test_cg_kernels_cpu import N_REFUSALS
    assert len(codes) == N_REFUSALS


def _t(field):
    st = torch.from_numpy(field.store).cuda()
    return st, st[field.off:field.off + field.rows * field.ld].view(field.rows, field.ld)


def test_ops_wrappers():
    """ops.cg_apply / cg_update / cg_dir and their path queries give the C ABI's results."""
    for mode, with_f in ((0, False), (1, True)):
        p, q, f, region = cc.apply_fields(257, 19, "fast", with_f)
        x0, nx, y0, ny = region
        want, s, scale, m = cc.apply_reference(mode, region, p, f)
        (_, tp), (sq, tq) = _t(p), _t(q)
        tf = None if f is None else _t(f)[1]
        assert ops.cg_apply_path(tp, tq, region, tf)[0] == ops.PATH_ROW_WALK
        assert ops.cg_apply_path(tp[:, 1:], tq, region, tf) == (ops.PATH_SCALAR, 0)
        out = ops.cg_apply(tp, tq, region, mode, tf, cc.C0, cc.C1 if with_f else 0.0).cpu()
        assert out.dtype == torch.float64 and out.shape == (2,)
        assert cc.same_bits(tq.cpu().numpy()[y0:y0 + ny, x0:x0 + nx], want)
        assert abs(float(out[0]) - s) <= TOL_SUM * max(1.0, scale) and float(out[1]) == m
    F, region = cc.stream_fields("pqxr", cc.UPDATE_ALIGN, 257, 9, "fast")
    x0, nx, y0, ny = region
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    t = {k: _t(v)[1] for k, v in F.items()}
    num, den = 0.7, 1.3
    a = num / den
    wx = F["x"].a[ys, xs] + a * F["p"].a[ys, xs]
    wr = F["r"].a[ys, xs] - a * F["q"].a[ys, xs]
    wp = wr + a * F["p"].a[ys, xs]
    tn, td = (torch.tensor([v], dtype=torch.float64, device="cuda") for v in (num, den))
    assert ops.cg_update_path(t["p"], t["q"], t["x"], t["r"], region) == ops.PATH_PT
    assert ops.cg_update_path(t["p"], t["q"], t["x"][:, 1:], t["r"], region) == ops.PATH_SCALAR
    assert ops.cg_dir_path(t["r"], t["p"], region) == ops.PATH_PT
    assert ops.cg_dir_path(t["r"], t["p"], (x0 + 1, nx - 1, y0, ny)) == ops.PATH_SCALAR
    out = ops.cg_update(tn, td, t["p"], t["q"], t["x"], t["r"], region).cpu()
    assert cc.same_bits(t["x"].cpu().numpy()[ys, xs], wx) and cc.same_bits(t["r"].cpu().numpy()[ys, xs], wr)
    assert abs(float(out[0]) - cc.fsum(wr * wr)) <= TOL_SUM * max(1.0, cc.fsum(wr * wr))
    assert float(out[1]) == float(np.abs(wr).max())
    assert ops.cg_dir(tn, td, t["r"], t["p"], region) is t["p"]
    assert cc.same_bits(t["p"].cpu().numpy()[ys, xs], wp)


def test_two_level_reduction_2000x4000():
    """2000 rows x 4000 columns: more partials than one reduction block takes, in
    apply (both modes) and in update.  1e-10 relative to the sum of the terms'
    magnitudes; two calls bitwise equal."""
    impl = _impl()
    nx, ny = 4000, 2000
    seg = cc.seg_rows(impl, nx)
    assert ((nx + 511) // 512) * ((ny + seg - 1) // seg) > 1024
    assert ((nx + 511) // 512) * ((ny + 3) // 4) > 1024
    for mode in (0, 1):
        p, q, _, region = cc.apply_fields(nx, ny, "fast", False, seed=5)
        want, s, scale, m = cc.apply_reference(mode, region, p, None)
        got = cc.call_apply(impl, mode, region, p, q)
        x0, _, y0, _ = region
        assert cc.same_bits(q.a[y0:y0 + ny, x0:x0 + nx], want)
        assert abs(got[0] - s) <= 1e-10 * scale and got[1] == m, (mode, got, s, scale, m)
        assert cc.call_apply(impl, mode, region, p, q) == got
    F, region = cc.stream_fields("pqxr", cc.UPDATE_ALIGN, nx, ny, "fast", seed=5)
    x0, _, y0, _ = region
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    r0, x0s = F["r"].store.copy(), F["x"].store.copy()
    wr = F["r"].a[ys, xs] - (0.7 / 1.3) * F["q"].a[ys, xs]
    got = cc.call_update(impl, region, 0.7, 1.3, F["p"], F["q"], F["x"], F["r"])
    s = cc.fsum(wr * wr)
    assert cc.same_bits(F["r"].a[ys, xs], wr)
    assert abs(got[0] - s) <= 1e-10 * s and got[1] == float(np.abs(wr).max()), (got, s)
    F["r"].store[:], F["x"].store[:] = r0, x0s
    assert cc.call_update(impl, region, 0.7, 1.3, F["p"], F["q"], F["x"], F["r"]) == got


def test_rows_4_gib_apart():
    """update and dir on 3 x 5 cells with a pitch of 2^28 + 2 doubles (32-bit
    offset arithmetic would land elsewhere), on the scalar path (odd column
    offset) and on the pair path."""
    lds = dict(p=(1 << 28) + 2, q=(1 << 28) + 6, x=(1 << 28) + 10, r=(1 << 28) + 14)
    ny, nx = 3, 5
    try:
        big = {k: torch.empty((ny - 1) * ld + nx + 4, dtype=torch.float64, device="cuda") for k, ld in lds.items()}
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"no room for four 4 GiB allocations: {e}")
    assert all((ny - 1) * ld * 8 > 2 ** 32 for ld in lds.values())
    rng = np.random.default_rng(5)
    rows = {k: [rng.random(nx + 4) - 0.5 for _ in range(ny)] for k in lds}  # host copies of the touched rows
    for k, ld in lds.items():
        for j in range(ny):
            big[k][j * ld:j * ld + nx + 4] = torch.from_numpy(rows[k][j]).cuda()
    tn, td = (torch.tensor([v], dtype=torch.float64, device="cuda") for v in (0.7, 1.3))
    a = 0.7 / 1.3
    for off, w, path in ((1, nx, ops.PATH_SCALAR), (2, nx - 1, ops.PATH_PT)):
        v = {k: torch.as_strided(big[k], (ny, w), (lds[k], 1), off) for k in lds}
        region = (0, w, 0, ny)
        assert ops.cg_update_path(v["p"], v["q"], v["x"], v["r"], region) == path
        assert ops.cg_dir_path(v["r"], v["p"], region) == path
        out = ops.cg_update(tn, td, v["p"], v["q"], v["x"], v["r"], region).cpu()
        ops.cg_dir(td, tn, v["r"], v["p"], region)
        torch.cuda.synchronize()
        rr = []
        for j in range(ny):
            s = slice(off, off + w)
            rows["x"][j][s] = rows["x"][j][s] + a * rows["p"][j][s]
            rows["r"][j][s] = rows["r"][j][s] - a * rows["q"][j][s]
            rows["p"][j][s] = rows["r"][j][s] + (1.3 / 0.7) * rows["p"][j][s]
            rr.append(rows["r"][j][s])
            for k, ld in lds.items():
                assert cc.same_bits(big[k][j * ld:j * ld + nx + 4].cpu().numpy(), rows[k][j]), (off, k, j)
        rr = np.concatenate(rr)
        assert abs(float(out[0]) - cc.fsum(rr * rr)) <= TOL_SUM and float(out[1]) == float(np.abs(rr).max())
