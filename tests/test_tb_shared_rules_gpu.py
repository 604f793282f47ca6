"""Every Dirichlet rule body of the shared hand-off group kernels
(csrc/kernels/jacobi5tb.hpp tb_block: plain, general keep, and the two
exec-masked one-column keeps of Sh<K, NW>, K = 12 / 16 / 20, two- and
four-strip groups, both stages, exact and scaled) at small shapes: bitwise
against the plain fp64 PyTorch reference of k single sweeps on the whole
output array (7.0 wherever nothing may be stored) and against the per-strip
launch.  The shapes come from the kernel's own geometry
(ops.jacobi5tb_shared_geom); tests/tb_shared_model.py lists the cases and
tests/test_tb_shared_model.py asserts, on the CPU, which bodies they reach:

A  one Dirichlet x side, both y sides halos, one segment: the ghost column in
   every lane slot (rect inset 0-3, NL, up to and past the last window that
   holds it), windows overhanging the array's rows, both ghosts in one group;
B  four segments of a Dirichlet field: fixed-row (general) and one-column
   bodies in one launch, rect = dom and inset on W / E;
C  the default segment planner on a 333-row rect: 64-row edge segments and
   interior ones, boundary and interior groups segmented differently;
D  the default dispatch on the engine's core + frame launches, the inset
   core rect one group wide or wider."""
import os

import pytest
import torch

import tb_shared_model as tm
from gpu_mpi_tests_amd import _native, ops
from gpu_mpi_tests_amd.ops import reference as ref
from test_jacobi_tb_gpu import _engine_frame

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _geom(k, strips):
    return ops.jacobi5tb_shared_geom(k, strips)


def _rand(ny, ncol, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(ny, ncol, generator=g, dtype=torch.float64)


def _launch(k, u, rect, dom, mask, shared, **kw):
    un = torch.full_like(u, 7.0)
    ops.jacobi5tb(k, u, un, [rect], dom, mask, shared=shared, **kw)
    torch.cuda.synchronize()
    return un.cpu()


def _check(k, strips, ncol, rect, dom, mask, seed, exact=False, seg_rows=0):
    """Forced group launch (checked by its plan) == reference == per-strip
    launch, on the whole array."""
    h = _rand(dom[3] + 2 * k, ncol, seed)
    u = h.to(DEV)
    p = ops.jacobi5tb_plan(k, [rect], dom, mask, u.stride(0), u.shape[0], shared=1 if strips == 4 else 2,
                           seg_rows=seg_rows)
    assert p["threads"] == 128 * strips, p  # the group launch runs
    got = _launch(k, u, rect, dom, mask, 1 if strips == 4 else 2, exact=exact, seg_rows=seg_rows)
    exp = torch.full(h.shape, 7.0, dtype=torch.float64)
    ref.jacobi5xk(k, h, exp, [rect], dom, mask)
    assert torch.equal(got, exp), (int((got != exp).sum()), float((got - exp).abs().max()))
    assert torch.equal(got, _launch(k, u, rect, dom, mask, -1, exact=exact, seg_rows=seg_rows))


def _id(key):
    return "-".join("x" if v is True else "s" if v is False else (str(v) or "dom") for v in key)


@pytest.mark.parametrize("key", tm.KEYS_A, ids=_id)
def test_one_column_keeps(key):
    c = tm.case_a(key, _geom(key[0], key[1]))
    _check(c.k, c.strips, c.ncol, c.rect, c.dom, c.mask, seed=31 * c.k + 7 * c.d + c.strips, exact=c.exact)


@pytest.mark.parametrize("key", tm.KEYS_B, ids=_id)
def test_mixed_bodies(key):
    c = tm.case_b(key, _geom(key[0], key[1]))
    _check(c.k, c.strips, c.ncol, c.rect, c.dom, c.mask, seed=17 * c.k + c.strips + c.d, exact=c.exact,
           seg_rows=c.seg_rows)


@pytest.mark.parametrize("k", tm.KS)
@pytest.mark.parametrize("strips", tm.STRIPS)
@pytest.mark.parametrize("mask", [0, 12, 5, 10])
def test_default_planner_small(k, strips, mask):
    g = _geom(k, strips)
    nx = (3 if strips == 4 else 4) * g["GOUT"] + 41  # interior groups beside the two boundary groups
    dom = (25, nx, k, 333)
    _check(k, strips, 25 + nx + k + 3, dom, dom, mask, seed=13 * k + mask)


@pytest.mark.skipif("GMT_TB_SHARED" in os.environ, reason="GMT_TB_SHARED overrides the default dispatch (cached per process)")
@pytest.mark.parametrize("k", tm.KS)
@pytest.mark.parametrize("mask", tm.MASKS_D)
@pytest.mark.parametrize("dw", tm.DW_D)
def test_default_dispatch_engine_frame(k, mask, dw):
    """core + frame launches as the engine issues them, the core rect inset
    K on its halo sides and at least one four-strip group wide: the default
    dispatch sends it to the group kernel; core + frame == one full launch ==
    the reference, and nothing outside the interior is written."""
    nx, ny, xo = tm.nx_d(k, dw, _geom(k, 4)), tm.NY_D, 24 + dw % 2
    dom = (xo, nx, k, ny)
    h = _rand(ny + 2 * k, xo + nx + k + 3, seed=73 + k + dw)
    u = h.to(DEV)
    core, frame = _engine_frame(k, xo, nx, k, ny, mask)
    assert ops.jacobi5tb_plan(k, [core], dom, mask, u.stride(0), u.shape[0], shared=0)["threads"] == 512
    full = torch.full_like(u, 7.0)
    ops.jacobi5tb(k, u, full, [dom], dom, mask)
    split = torch.full_like(u, 7.0)
    ops.jacobi5tb(k, u, split, [core], dom, mask)
    ops.jacobi5tb(k, u, split, frame, dom, mask, wg_waves=1)
    torch.cuda.synchronize()
    exp = torch.full(h.shape, 7.0, dtype=torch.float64)
    ref.jacobi5xk(k, h, exp, [dom], dom, mask)
    assert torch.equal(full.cpu(), exp)
    assert torch.equal(split.cpu(), exp)
