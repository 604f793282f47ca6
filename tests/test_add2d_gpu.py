"""gmt_add2d (csrc/kernels/add2d.hip) and the fill modes 6 and 7 on the GPU,
bitwise against NumPy: one rounding per cell, nothing outside the region
touched (sentinels around it, NaN in g), the kernel each case takes, the empty
region, refused arguments, and rows more than 2^32 bytes apart.  The cases
are those of the CPU backend (tests/source_cases.py)."""
import numpy as np
import pytest
import torch

import source_cases as sc
from gpu_mpi_tests_amd import _native, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


@pytest.mark.parametrize("name", list(sc.ADD_CASES), ids=lambda n: n.replace(" ", "_"))
def test_add2d_bitwise(name):
    c = sc.add_case(name)
    g, u = torch.from_numpy(c["g"]).cuda(), torch.from_numpy(c["u"]).cuda()
    gv, uv = g[c["gs"]], u[c["us"]]
    if c["path"] is not None:
        assert ops.add2d_path(gv, uv) == c["path"] == {sc.PATH_PT: ops.PATH_PT, sc.PATH_SCALAR: ops.PATH_SCALAR}[c["path"]]
    assert ops.add2d(gv, uv) is uv
    torch.cuda.synchronize()
    assert sc.same_bits(u.cpu().numpy(), c["want"])  # the region added, everything around it bit-identical
    assert sc.same_bits(g.cpu().numpy(), c["g"])


def test_add2d_on_a_side_stream_and_empty():
    """The launch goes to the caller's current stream; an empty region launches nothing."""
    c = sc.add_case("odd nx")
    g, u = torch.from_numpy(c["g"]).cuda(), torch.from_numpy(c["u"]).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.add2d(g[c["gs"]], u[c["us"]])
    s.synchronize()
    assert sc.same_bits(u.cpu().numpy(), c["want"])
    L = _native.lib()
    for nx, ny in ((0, 5), (5, 0), (0, 0)):
        assert L.gmt_add2d(nx, ny, None, 64, None, 64, None) == 0  # not even the pointers are looked at
    torch.cuda.synchronize()


def test_add2d_refuses_bad_arguments():
    L = _native.lib()
    g = torch.full((8, 64), float("nan"), dtype=torch.float64, device="cuda")
    u = torch.ones(8, 64, dtype=torch.float64, device="cuda")
    codes = [L.gmt_add2d(nx, ny, g.data_ptr(), ldg, u.data_ptr(), ld, None) for ny, nx, ldg, ld in sc.ADD_REFUSED]
    codes.append(L.gmt_add2d(4, 4, None, 64, u.data_ptr(), 64, None))
    codes.append(L.gmt_add2d(4, 4, g.data_ptr(), 64, None, 64, None))
    torch.cuda.synchronize()
    assert codes == [1] * len(codes), codes  # the CPU backend's code (tests/test_source_cpu.py)
    assert bool((u == 1.0).all())
    with pytest.raises(ValueError):
        ops.add2d(g[:, :5], u[:, :6])
    with pytest.raises(TypeError):
        ops.add2d(g.float(), u.float())


def test_add2d_rows_4_gib_apart():
    """5 x 3 cells with a pitch of 2^28 + 2 doubles: 32-bit offset arithmetic would land elsewhere."""
    ld, ldg, ny, nx = sc.BIG_LD, sc.BIG_LDG, sc.BIG_NY, sc.BIG_NX
    try:
        u = torch.empty((ny - 1) * ld + nx + 2, dtype=torch.float64, device="cuda")
        g = torch.empty((ny - 1) * ldg + nx + 2, dtype=torch.float64, device="cuda")
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"no room for two 4 GiB allocations: {e}")
    assert (ny - 1) * ld * 8 > 2 ** 32
    rng = np.random.default_rng(5)
    want = []
    for j in range(ny):  # only the region and the cell on either side of each row are touched
        urow, grow = sc._values(rng, nx + 2), np.full(nx + 2, np.nan)
        grow[1:-1] = sc._values(rng, nx)
        u[j * ld:j * ld + nx + 2] = torch.from_numpy(urow).cuda()
        g[j * ldg:j * ldg + nx + 2] = torch.from_numpy(grow).cuda()
        urow[1:-1] += grow[1:-1]
        want.append(urow)
    gv = torch.as_strided(g, (ny, nx), (ldg, 1), 1)
    uv = torch.as_strided(u, (ny, nx), (ld, 1), 1)
    assert ops.add2d_path(gv, uv) == ops.PATH_SCALAR  # odd column offset; the pair path: the same case, offset 2
    ops.add2d(gv, uv)
    torch.cuda.synchronize()
    for j in range(ny):
        assert sc.same_bits(u[j * ld:j * ld + nx + 2].cpu().numpy(), want[j]), j
    gv = torch.as_strided(g, (ny, nx - 1), (ldg, 1), 2)
    uv = torch.as_strided(u, (ny, nx - 1), (ld, 1), 2)
    assert ops.add2d_path(gv, uv) == ops.PATH_PT
    ops.add2d(gv, uv)
    torch.cuda.synchronize()
    for j in range(ny):
        w = want[j].copy()
        w[2:-1] += g[j * ldg + 2:j * ldg + nx + 1].cpu().numpy()
        assert sc.same_bits(u[j * ld:j * ld + nx + 2].cpu().numpy(), w), j


def test_fill_modes_6_and_7():
    def fill(mode, nx, ny, x0, dx, y0, dy):
        z = torch.full((ny, nx + 3), float("nan"), dtype=torch.float64, device="cuda")
        ops.fill_poly(z[:, :nx], mode, x0, dx, y0, dy)
        torch.cuda.synchronize()
        out = z.cpu().numpy()
        assert np.isnan(out[:, nx:]).all()
        return out[:, :nx].copy()

    sc.check_fills(fill)
