"""Every dispatch path of the derivative, reduction and single-sweep Jacobi
kernels, on padded views (row pitch != width) where the launchers' choices
differ from those for contiguous tensors.

Each stencil case first asserts the kernel it is about to run
(``ops.stencil5_2d_path``: the launcher's own decision, no launch), then
compares with the long-double reference of tests/kernel_refs.py under the
bound derived there, then asserts that nothing beside the output was written:
outputs are views of a base filled with a sentinel, with a guard row above
and below, and the sentinel must survive in columns nx..ld of every row (the
16-byte store of a last odd column would overwrite column nx).
"""
import pytest
import torch

import kernel_refs as kr
import resid_cases as rc
from gpu_mpi_tests_amd import _native, ops
from gpu_mpi_tests_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.0625
F64 = torch.float64


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()  # must be the native path — fail loudly otherwise


def _view_of(z_cpu, ld, poison=None):
    """The CPU field as a device view of pitch ld (even: 16-B aligned rows);
    the pad columns stay uninitialised unless a poison value is given."""
    rows, nx = z_cpu.shape
    if ld == nx:
        return z_cpu.to(DEV)
    base = torch.empty(rows, ld, dtype=F64, device=DEV)
    if poison is not None:
        base.fill_(poison)
    v = base[:, :nx]
    v.copy_(z_cpu)
    return v


def _out_view(ny, nx, ld):
    base = torch.full((ny + 2, ld), SENTINEL, dtype=F64, device=DEV)
    return base, base[1:-1, :nx]


def _assert_rest_untouched(base, nx):
    assert bool((base[0] == SENTINEL).all()) and bool((base[-1] == SENTINEL).all()), "a guard row was written"
    assert bool((base[1:-1, nx:] == SENTINEL).all()), "columns nx..ld of an output row were written"


def _run_stencil(dim, ny, nx, ld_in, ld_out, path, seg_rows, default_coef=False):
    z, r, bound, coef, scale = kr.stencil_case(dim, ny, nx, default_coef)
    inp = _view_of(z, ld_in)
    base, out = _out_view(ny, nx, ld_out)
    assert ops.stencil5_2d_path(inp, dim, out) == (path, seg_rows)
    ops.stencil5_2d(inp, dim, out=out, scale=scale, coef=coef)
    torch.cuda.synchronize()
    kr.check(out, r, bound, f"stencil5_2d dim {dim} {ny}x{nx} ld {ld_in}->{ld_out}")
    _assert_rest_untouched(base, nx)


# ------------------------------------------------- dim 1, even width: window walk
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("ny,nx", kr.WIN_CASES)
def test_stencil5_dim1_window_walk(ny, nx, padded):
    """stencil5_d1_win: 128 columns per wave, 2048 per group, segments of
    min(256, ny) rows, a ring of 9 rows.  One valid lane; a second group with
    a single valid lane (2050) and its ragged tail (4098, 4100) while the other
    waves exit or clamp their loads; segment lengths on both sides of 256; rows
    per segment 1, 4, 8, 0 (mod 9) and a second segment of 1, 9 and 257 rows."""
    ld_in, ld_out = (nx + 6, nx + 10) if padded else (nx, nx)
    _run_stencil(1, ny, nx, ld_in, ld_out, ops.PATH_D1_WIN, min(256, ny))


# ------------------------------------------------- dim 1, odd width: LDS-DMA pipeline
@pytest.mark.parametrize("ny,nx", kr.DMA_CASES)
def test_stencil5_dim1_dma_odd_width(ny, nx):
    """stencil5_d1_dma<1, true>: segments of min(128, ny) rows, steps padded to
    a multiple of 5, 4 waves of 128 columns per workgroup, an 8-byte store for
    the last column.  Every L mod 5, segment tails of 1 and 5 rows (129, 133),
    the last column as the only column, at lane 0 (129, 513) and at lane 63
    (127, 255, 511), a second workgroup holding one strip (513, 515)."""
    _run_stencil(1, ny, nx, nx + 5, nx + 1, ops.PATH_D1_DMA, min(128, ny))


# ------------------------------------------------- dim 1, odd width, pitches of 2^21 doubles and more
def test_stencil5_dim1_dma_long_input_pitch():
    """The 32-bit buffer offsets bound the segment: 2^31 / (2^21 * 8) - 13 = 115 rows."""
    _run_stencil(1, 150, 131, 1 << 21, 132, ops.PATH_D1_DMA, 115)


def test_stencil5_dim1_dma_long_output_pitch():
    _run_stencil(1, 150, 131, 136, 1 << 21, ops.PATH_D1_DMA, 115)


@pytest.mark.parametrize("ld_in,path,seg_rows", [(12782640, ops.PATH_D1_DMA, 8), (12782642, ops.PATH_PT, 0)])
def test_stencil5_dim1_pitch_boundary(ld_in, path, seg_rows):
    """The longest pitch the DMA pipeline takes (21 rows of it fit 2^31 bytes:
    segments of 8) and the next even one (20 rows: one pair per thread)."""
    _run_stencil(1, 20, 131, ld_in, 132, path, seg_rows)


def test_stencil5_dim1_pitch_too_long_for_dma():
    _run_stencil(1, 9, 131, 1 << 24, 132, ops.PATH_PT, 0)


# ------------------------------------------------- dim 1, odd width, fewer than 8 rows: pairs per thread
@pytest.mark.parametrize("ny,nx", kr.PT1_CASES)
def test_stencil5_dim1_pair_per_thread(ny, nx):
    """stencil5_pt<1> with its odd last column."""
    _run_stencil(1, ny, nx, nx + 5, nx + 1, ops.PATH_PT, 0)


# ------------------------------------------------- dim 0, odd width
@pytest.mark.parametrize("ny,nx", kr.PT0_CASES)
def test_stencil5_dim0_odd_tail(ny, nx):
    """stencil5_pt<0>: the single last column (x + 1 == nx_out) beside the pairs."""
    _run_stencil(0, ny, nx, nx + 4 + 3, nx + 5, ops.PATH_PT, 0)


# ------------------------------------------------- the derivative's own coefficients, one case per path
@pytest.mark.parametrize("dim,ny,nx", kr.DEFAULT_COEF_CASES)
def test_stencil5_default_coefficients(dim, ny, nx):
    path, seg = {(1, 257, 2050): (ops.PATH_D1_WIN, 256), (1, 133, 257): (ops.PATH_D1_DMA, 128),
                 (1, 7, 129): (ops.PATH_PT, 0), (0, 5, 129): (ops.PATH_PT, 0)}[(dim, ny, nx)]
    nx_in = nx + (4 if dim == 0 else 0)
    _run_stencil(dim, ny, nx, nx_in + (nx_in % 2) + 4, nx + (nx % 2) + 2, path, seg, default_coef=True)


# ------------------------------------------------- 1-D
@pytest.mark.parametrize("n,rem_path", [(kr.ONE_D_CASES[0], ops.PATH_PT), (kr.ONE_D_CASES[1], ops.PATH_SCALAR)])
def test_stencil5_1d_remainder(n, rem_path):
    """Rows of 2^16 through stencil5_pt<0>, then the remainder as a one-row
    field: 2 elements on the vector path, 17 (odd pitch) one per lane."""
    z, r, bound, coef, scale = kr.stencil_case(None, 1, n)
    inp = z.to(DEV)
    base = torch.full((n + 8,), SENTINEL, dtype=F64, device=DEV)
    out = base[:n]
    rows, rem = divmod(n, 65536)
    assert ops.stencil5_2d_path(inp[:rows * 65536 + 4].as_strided((rows, 65540), (65536, 1)), 0,
                                out[:rows * 65536].view(rows, 65536)) == (ops.PATH_PT, 0)
    assert ops.stencil5_2d_path(inp[rows * 65536:].view(1, rem + 4), 0,
                                out[rows * 65536:].view(1, rem)) == (rem_path, 0)
    ops.stencil5_1d(inp, out=out, scale=scale, coef=coef)
    torch.cuda.synchronize()
    kr.check(out, r, bound, f"stencil5_1d {n}")
    assert bool((base[n:] == SENTINEL).all())


# ------------------------------------------------- reductions on padded views (odd nx, even ld)
def _reduce_views(ny, nx):
    """a and b on the device with different even pitches; the pad columns hold
    large values that differ between a and b, so a read past nx shows."""
    a, b = kr.reduce_case(ny, nx)
    return a, b, _view_of(a, nx + 1, poison=3.0e6), _view_of(b, nx + 7, poison=-5.0e6)


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("ny,nx", kr.REDUCE_CASES)
def test_sum_axis_padded(ny, nx, keep):
    """keep 1: rowsum_pass1's vector path with the odd last element of a
    chunk (4095: one chunk; 4097, 8193: a chunk of one element); keep 0:
    col_plan's 16-row partials (16, 17, 33 rows)."""
    a, _, da, _ = _reduce_views(ny, nx)
    n_out = nx if keep == 0 else ny
    base = torch.full((n_out + 4,), SENTINEL, dtype=F64, device=DEV)
    out = ops.sum_axis(da, keep, out=base[:n_out])
    torch.cuda.synchronize()
    kr.check(out, *kr.sum_ref(a, 0 if keep == 0 else 1), f"sum_axis keep {keep} {ny}x{nx}")
    assert bool((base[n_out:] == SENTINEL).all())


@pytest.mark.parametrize("ny,nx", kr.REDUCE_CASES)
def test_diff_sq_padded(ny, nx):
    a, b, da, db = _reduce_views(ny, nx)
    kr.check(ops.diff_sq(da, db), *kr.diff_sq_ref(a, b), f"diff_sq {ny}x{nx}")


@pytest.mark.parametrize("ny,nx", kr.REDUCE_CASES)
def test_abs_max_padded(ny, nx):
    """Exact; the largest value sits in the last column of the last row."""
    a, _, da, _ = _reduce_views(ny, nx)
    assert float(ops.abs_max(da)) == float(a.abs().max())
    da[ny - 1, nx - 1] = -2.5
    assert float(ops.abs_max(da)) == 2.5


@pytest.mark.parametrize("ny,nx", kr.REDUCE_CASES)
def test_diff_bits_padded(ny, nx):
    """Equal fields whose pad columns differ compare equal; then one flipped
    low bit in the last column, and (where there is room) a NaN and a -0.0."""
    a, _, da, _ = _reduce_views(ny, nx)
    db = _view_of(a, nx + 7, poison=-5.0e6)
    assert ops.diff_bits(da, db) == (0.0, 0)
    db.view(torch.int64)[ny - 1, nx - 1] ^= 1
    exp_max, n = abs(float(da[ny - 1, nx - 1] - db[ny - 1, nx - 1])), 1
    assert ops.diff_bits(da, db) == (exp_max, n)
    if nx > 2:
        db[0, 0] = float("nan")
        da[ny // 2, 1] = 0.0
        db[ny // 2, 1] = -0.0
        assert ops.diff_bits(da, db) == (float("inf"), 3)


# ------------------------------------------------- single-sweep Jacobi (the check of the timed run)
@pytest.mark.parametrize("ny,nx", kr.JACOBI_CASES)
def test_jacobi5_odd_width_pair_path(ny, nx):
    """jacobi5_pt with an odd last column: even pitches and x0 = 8, with and
    without f and the residual; tolerances of test_kernels_gpu.test_jacobi5."""
    ld = nx + 17  # even
    u_cpu = kr.field((ny + 2, ld), seed=31 * ny + nx)
    f_cpu = kr.field((ny + 2, ld), seed=31 * ny + nx + 1)
    u, f = u_cpu.to(DEV), _view_of(f_cpu, ld + 4)
    for ff, c1, resid in ((None, 0.0, True), (f, -0.01, True), (None, 0.0, False), (f, -0.01, False)):
        un = torch.full_like(u, SENTINEL)
        un_ref = torch.full(u_cpu.shape, SENTINEL, dtype=F64)
        assert ops.jacobi5_path(u, un, (8, nx, 1, ny), f=ff) == ops.PATH_PT
        r = ops.jacobi5(u, un, (8, nx, 1, ny), f=ff, c1=c1, resid=resid)
        r_ref = ref.jacobi5(u_cpu, un_ref, 8, nx, 1, ny, f_cpu if ff is not None else None, 0.25, c1)
        torch.testing.assert_close(un.cpu(), un_ref, rtol=1e-14, atol=1e-14)  # the sentinel around the region too
        if resid:
            print(f"jacobi5 {ny}x{nx}: resid {float(r)!r} ref {float(r_ref)!r}")
            assert abs(float(r) - float(r_ref)) <= 1e-11 * max(1.0, float(r_ref))


def test_jacobi5_path_scalar_for_odd_origin_or_pitch():
    u = torch.zeros(8, 40, dtype=F64, device=DEV)
    assert ops.jacobi5_path(u, u, (3, 31, 2, 4)) == ops.PATH_SCALAR
    assert ops.jacobi5_path(u, u, (4, 31, 2, 4)) == ops.PATH_PT
    v = torch.zeros(8, 41, dtype=F64, device=DEV)
    assert ops.jacobi5_path(v, v, (4, 31, 2, 4)) == ops.PATH_SCALAR
    assert ops.jacobi5_path(u, u, (4, 31, 2, 4), f=v) == ops.PATH_SCALAR


# ------------------------------------------------- the row walk's segment rule (row_walk.hpp)
@pytest.mark.parametrize("ny", [1, 9, 256, 513])
@pytest.mark.parametrize("nx", [rc.NXS[0], rc.NXS[4], rc.NXS[5], rc.NXS[-1]])
def test_row_walk_kernels_agree_on_seg_rows(nx, ny):
    """The residual, CG's apply and the Chebyshev step walk the same segments:
    one rule decides the rows per segment of all three."""
    u = torch.zeros(ny + 2, 8 + nx + 1 + (nx + 1) % 2, dtype=F64, device=DEV)
    v = torch.zeros_like(u)
    region = (8, nx, 1, ny)
    resid = ops.jacobi5_resid_path(u, region)
    assert resid[0] == ops.PATH_ROW_WALK and resid[1] >= 2
    assert ops.cg_apply_path(u, v, region) == resid
    assert ops.cheby_step_path(u, v, region) == resid
    assert ops.jacobi5_resid_path(u, region, f=v) == ops.cg_apply_path(u, v, region, v) == resid
    assert ops.cheby_step_path(u, v, region, v) == resid
