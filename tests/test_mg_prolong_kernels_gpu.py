"""gmt_mg_prolong_smooth on the GPU (csrc/kernels/mg.hip) against the NumPy
model of tests/mg_prolong_cases.py.

Everything outside the read sets of u, f and e is NaN (e holds exactly the
coarse cells the rule names for B0), out a sentinel outside the region that
must be bitwise intact afterwards; inputs are compared bitwise before and
after; out[R] is bitwise reference.mg_prolong_smooth.  h = 1..4, Jacobi and
red-black with either colour phase, all four (px, py), without and with f.
Widths (from gmt_mg_prolong_smooth_geom) cover the lane-pair tail and the seams
between waves and workgroups; heights the regions shorter than the warm-up and
the segment seams (L = the rows per segment the path query reports).  Only the
all-aligned variant may take the walk: the path of every case is asserted."""
import types

import numpy as np
import pytest
import torch

import mg_prolong_cases as pc
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
    for h in pc.HS:
        assert pc.geom(_impl(), h) == ops.mg_prolong_smooth_geom(h) == ops.mg_smooth_k_geom(h)
    with pytest.raises(ValueError):
        ops.mg_prolong_smooth_geom(5)


@pytest.mark.parametrize("h", pc.HS)
def test_all_masks(h):
    assert pc.run_all_masks(_impl(), h) == pc.N_ALL_MASKS


@pytest.mark.parametrize("iw", range(pc.N_WIDTHS))
@pytest.mark.parametrize("h", pc.HS)
def test_widths(h, iw):
    assert pc.run_width(_impl(), h, iw) == 2 * pc.N_SWEEP


@pytest.mark.parametrize("h", pc.HS)
def test_heights(h):
    impl = _impl()
    w, _ = pc.geom(impl, h)
    want = sum(len(pc.prolong_heights(h, pc.seg_rows(impl, h, nx))) for nx in (3, w + 1)) * pc.N_SWEEP
    assert pc.run_heights(impl, h) == want


@pytest.mark.parametrize("h", pc.HS)
def test_scalar_shapes(h):
    assert pc.run_scalar_shapes(_impl(), h) == pc.N_SCALAR


def test_identity_two_existing_calls():
    """Bitwise gmt_mg_prolong_add over B0 (the region start moved, px, py, cx0, cy0 shifted so that every cell
    keeps its coarse column) followed by gmt_mg_smooth_k / gmt_mg_smooth_rb, through the kernels that exist."""
    assert pc.run_identities(_impl()) == pc.N_IDENTITIES


def test_negative_zero_ring():
    assert pc.run_negative_zero_ring(_impl()) == 4 * 3 * 3 * 2


def test_empty_regions_and_refusals():
    codes = pc.run_empty_and_refusals(_impl())
    assert codes == [1] * pc.N_REFUSALS, codes  # the CPU backend's codes (tests/test_mg_prolong_kernels_cpu.py)


def _t(field):
    st = torch.from_numpy(field.store).cuda()
    return st[field.off:field.off + field.rows * field.ld].view(field.rows, field.ld)


def test_ops_wrappers():
    """ops.mg_prolong_smooth and its queries give the C ABI's results; shared storage is refused."""
    for h in pc.HS:
        for m, mode in enumerate(pc.MODES):
            par, with_f = pc.PARITIES[(h + m) % 4], bool(m % 2)
            e, u, o, f, region = pc.fields(h, 257, 19, 15, par, "fast", with_f)
            x0, nx, y0, ny = region
            want = pc.reference(h, mode, region, par, 15, e, u, f, 0.8)
            te, tu, to = _t(e), _t(u), _t(o)
            tf = None if f is None else _t(f)
            args = (region, par, (pc.CX0, pc.CY0), h, mode[0], mode[1], 15, tf)
            assert ops.mg_prolong_smooth_path(te, tu, to, *args) == (ops.PATH_ROW_WALK, pc.seg_rows(_impl(), h, 257))
            assert ops.mg_prolong_smooth_path(te, tu[:, 1:], to, *args) == (ops.PATH_SCALAR, 0)
            assert ops.mg_prolong_smooth(te, tu, to, 0.8, *args, pc.C0, pc.C1) is to
            assert pc.same_bits(to.cpu().numpy()[y0:y0 + ny, x0:x0 + nx], want)
    for bad in (tu, te):
        with pytest.raises(ValueError, match="share storage"):
            ops.mg_prolong_smooth(te, tu, bad, 0.8, region, par, (pc.CX0, pc.CY0), h)


def test_rows_4_gib_apart():
    """5 x 4 cells of a field whose rows are 2^28 + 2 doubles apart: 32-bit offset arithmetic would land
    elsewhere.  The one-lane-per-cell kernel (odd first column) and the walk, with halo rows below and above
    (mask S + N), so the far rows are read."""
    ld = (1 << 28) + 2
    ny, nx, W = 4, 5, 12
    h = 2
    rows = ny + 2 * h
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
    he = rng.random((8, 10)) - 0.5
    te = torch.from_numpy(he).cuda()
    from gpu_mpi_tests_amd.ops import reference as ref

    for x0, fast in ((3, False), (4, True)):
        region = (x0, nx, h, ny)
        for m, par in enumerate(pc.PARITIES):
            rb, cp = pc.MODES[m % 3]
            to = torch.full((rows, W), pc.SENTINEL, dtype=torch.float64, device="cuda")
            want = np.full((rows, W), pc.SENTINEL)
            assert ops.mg_prolong_smooth_path(te, tu, to, region, par, (2, 3), h, rb, cp, 12)[0] == \
                (ops.PATH_ROW_WALK if fast else ops.PATH_SCALAR)
            ops.mg_prolong_smooth(te, tu, to, 0.8, region, par, (2, 3), h, rb, cp, 12, None, pc.C0, pc.C1)
            ref.mg_prolong_smooth(he, host, want, 0.8, x0, nx, h, ny, par[0], par[1], 2, 3, h, rb, cp, 12, None,
                                  pc.C0, pc.C1)
            assert pc.same_bits(to.cpu().numpy(), want), (x0, par)
    torch.cuda.synchronize()
    for j in range(rows):
        assert pc.same_bits(big[j * ld:j * ld + W].cpu().numpy(), host[j]), j
