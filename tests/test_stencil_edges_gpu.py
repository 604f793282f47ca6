"""The boundary-band split of the derivative stencil on the GPU:
``ops.stencil5_2d_edges`` (the band kernels of csrc/kernels/stencil5.hip) and
``ops.stencil5_2d_interior`` (the production kernels on the sub-rectangle
between the bands), for every ``sides`` of the band rule in gmt/kernels.h.

Each case fills two outputs with a sentinel, runs the edges into one and the
interior into the other, and asserts that exactly the band cells changed in
the first and exactly their complement in the second (the outputs are views of
a base with a guard row above and below and pad columns, which must keep the
sentinel too).  The union of the two is then compared with the long-double
reference of tests/kernel_refs.py under the bound derived there.

Shapes: extents 1, 2, 3, 4, 5, 8 along the stencil's axis (bands that fill the
output, overlap-free bands with an empty, one-cell and wider interior; odd
extents send dim 0 to the one-cell-per-lane kernel), and across it 1, 3, 63,
64, 65, 257 and the band kernels' block sizes +-1: 256 rows per block in dim 0,
512 columns per block in dim 1.  Layouts: contiguous, padded even pitches (the
16-byte kernels), a view offset by one element and odd pitches (the
one-cell-per-lane kernel).
"""
import pytest
import torch

import kernel_refs as kr
from gpu_mpi_tests_amd import _native, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.0625
F64 = torch.float64
ALONG = [1, 2, 3, 4, 5, 8]
ACROSS = [1, 3, 63, 64, 65, 257, 255, 256, 511, 512, 513]
LAYOUTS = ["contiguous", "padded", "offset1", "oddpitch"]


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()  # must be the native path — fail loudly otherwise


def _even(n):
    return n + (n & 1)


def _pitch(width, layout, pad):
    if layout == "contiguous":
        return width
    if layout == "oddpitch":
        return _even(width) + pad + 1
    return _even(width) + pad  # padded, offset1: even pitches


def _alloc(rows, width, layout, pad, fill=None):
    """(base, view): `rows` x `width` view of a base of the layout's pitch,
    one guard row above and below; offset1 starts the view at element 1."""
    ld = _pitch(width, layout, pad)
    off = 1 if layout == "offset1" else 0
    base = torch.empty(rows + 2, ld + off, dtype=F64, device=DEV)
    if fill is not None:
        base.fill_(fill)
    flat = base.view(-1)
    view = flat[ld + off:].as_strided((rows, width), (ld, 1))
    assert view.stride(0) == ld and view.data_ptr() == flat.data_ptr() + 8 * (ld + off)
    return base, view


def _band_mask(dim, ny, nx, sides):
    n = nx if dim == 0 else ny
    lo_w, hi_w = ops.stencil5_bands(n, sides)
    along = torch.zeros(n, dtype=torch.bool)
    along[:lo_w] = True
    along[n - hi_w:] = True
    assert int(along.sum()) == lo_w + hi_w  # the two bands never overlap
    return (along[None, :] if dim == 0 else along[:, None]).expand(ny, nx)


def _run(dim, ny, nx, layout, default_coef=False):
    z, r, bound, coef, scale = kr.stencil_case(dim, ny, nx, default_coef)
    _, inp = _alloc(z.shape[0], z.shape[1], layout, 6)
    inp.copy_(z)
    for sides in range(4):
        band = _band_mask(dim, ny, nx, sides)
        base_e, out_e = _alloc(ny, nx, layout, 10, SENTINEL)
        base_i, out_i = _alloc(ny, nx, layout, 10, SENTINEL)
        ops.stencil5_2d_edges(inp, dim, out_e, sides=sides, scale=scale, coef=coef)
        ops.stencil5_2d_interior(inp, dim, out_i, sides=sides, scale=scale, coef=coef)
        torch.cuda.synchronize()
        what = f"dim {dim} {ny}x{nx} {layout} sides {sides}"
        got_e, got_i = out_e.cpu(), out_i.cpu()
        assert torch.equal(got_e != SENTINEL, band), f"edges, {what}: not exactly the band cells were written"
        assert torch.equal(got_i != SENTINEL, ~band), f"interior, {what}: not exactly the complement was written"
        # everything of the bases outside the views kept the sentinel
        for base, out in ((base_e, out_e), (base_i, out_i)):
            n_written = int((base != SENTINEL).sum())
            assert n_written == int((out != SENTINEL).sum()), f"{what}: a cell outside the output was written"
        kr.check(torch.where(band, got_e, got_i), r, bound, f"edges + interior, {what}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("across", ACROSS)
@pytest.mark.parametrize("along", ALONG)
@pytest.mark.parametrize("dim", [0, 1])
def test_edges_and_interior_partition_the_output(dim, along, across, layout):
    ny, nx = (across, along) if dim == 0 else (along, across)
    _run(dim, ny, nx, layout)


@pytest.mark.parametrize("layout", ["padded", "offset1"])
@pytest.mark.parametrize("dim,ny,nx", [(0, 257, 8), (1, 8, 513)])
def test_edges_with_the_derivative_coefficients(dim, ny, nx, layout):
    """DERIV5's centre tap is 0 and its taps are antisymmetric: the case the apps run."""
    _run(dim, ny, nx, layout, default_coef=True)


def test_empty_band_or_no_side_launches_nothing():
    """sides == 0 and empty outputs return 0 and leave `out` alone."""
    base, out = _alloc(4, 6, "padded", 10, SENTINEL)
    inp = torch.zeros(4, 10, dtype=F64, device=DEV)
    ops.stencil5_2d_edges(inp, 0, out, sides=0)
    L = _native.lib()
    for dim in (0, 1):
        for nx, ny in ((0, 5), (5, 0)):
            for fn in (L.gmt_stencil5_2d_edges, L.gmt_stencil5_2d_interior):
                assert fn(dim, nx, ny, None, 1.0, inp.data_ptr(), 10, out.data_ptr(), out.stride(0), 3, 0) == 0
    torch.cuda.synchronize()
    assert bool((base == SENTINEL).all())
