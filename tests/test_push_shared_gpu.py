"""Inline halo exchange (gmt_tb_opts.push) in shared hand-off group launches
(gmt_tb_opts.shared = 2 / 4, csrc/kernels/jacobi5tb.hpp Sh<K, NW>) on the GPU.

* kernel level: the first window of group 0 stores the W face, the last
  window of the last (shifted) group the E face, every output wave whose
  segment holds S / N rows that y face; every target receives exactly its
  face and nothing else, the pass's own output stays bitwise equal to k
  single sweeps — for every Dirichlet rule body that can meet the push body;
* the launcher's decision (ops.jacobi5tb_shared_path) is asserted first, so
  a launch that silently fell back to the per-strip kernel proves nothing;
* fallbacks (a rect narrower than a group, a (k, strips) without a push-group
  kernel) run the per-strip push kernel, bitwise;
* engine level: one rank periodic, and ranks sharing the GPU over IPC."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import free_port
from gpu_mpi_tests_amd import _native, ops
from gpu_mpi_tests_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (12, 16, 20)
XO = 24
# halo mask -> pushed directions: every rule body meets the push body
MASK_DIRS = {
    15: ("S", "N", "W", "E", "SW", "SE", "NW", "NE"),
    14: ("S", "N", "E", "SE", "NE"),  # W Dirichlet: its one-column keep meets y-face segments
    13: ("S", "N", "W", "SW", "NW"),  # the same for E
    3: ("W", "E"),                    # fixed rows within reach of the x-face windows
    6: ("E", "S", "SE"),              # a corner rank of a non-periodic 2x2 grid
}


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _supported(k, nw):
    return ops.tb_push_shared_supported(k, nw)


def _face(d, dom, w):
    x0, nx, y0, ny = dom
    xs = slice(x0, x0 + w) if "W" in d else (slice(x0 + nx - w, x0 + nx) if "E" in d else slice(x0, x0 + nx))
    ys = slice(y0, y0 + w) if d.startswith("S") else (slice(y0 + ny - w, y0 + ny) if d.startswith("N")
                                                      else slice(y0, y0 + ny))
    return ys, xs


_CASES = {}


def _case(k, ny, nx, mask):
    """Input field and the reference output of k single sweeps, computed once
    per (k, shape, mask) and shared (never modified) by every test using it."""
    key = (k, ny, nx, mask)
    if key not in _CASES:
        gen = torch.Generator(device="cpu").manual_seed(ny * 7 + nx + k)
        u = torch.rand(ny + 2 * k, XO + nx + k + 5, generator=gen, dtype=torch.float64)
        dom = (XO, nx, k, ny)
        exp = torch.full(u.shape, 7.0, dtype=torch.float64)
        ref.jacobi5xk(k, u, exp, [dom], dom, mask)
        _CASES[key] = (u, exp, dom)
    return _CASES[key]


def _run_and_check(k, ny, nx, mask, w, shared, exact, want_path):
    u_cpu, exp, dom = _case(k, ny, nx, mask)
    dirs = MASK_DIRS[mask]
    path = ops.jacobi5tb_shared_path(k, [dom], mask, shared=shared, push_w=w)
    assert path == want_path, (path, want_path)
    u = u_cpu.to(DEV)
    un = torch.full_like(u, 7.0)
    tg = {d: torch.full_like(u, 3.0) for d in dirs}
    ops.jacobi5tb(k, u, un, [dom], dom, mask, push=tg, push_w=w, shared=shared, exact=exact)
    torch.cuda.synchronize()
    got = un.cpu()
    assert torch.equal(got, exp), (int((got != exp).sum()), float((got - exp).abs().max()))
    for d, t in tg.items():
        want = torch.full(u.shape, 3.0, dtype=torch.float64)
        ys, xs = _face(d, dom, w)
        want[ys, xs] = exp[ys, xs]
        g = t.cpu()
        assert torch.equal(g, want), (d, int((g != want).sum()))


def _widths(k, nw):
    gout = ops.jacobi5tb_shared_geom(k, nw)["GOUT"]
    # one group (W in window 0, E in window NW - 1); two groups that overlap
    # almost entirely; an odd width (the shifted last group has the other
    # parity); a middle group holding no x face
    return {"gout": gout, "gout+6": gout + 6, "gout+7": gout + 7, "2gout+100": 2 * gout + 100}


@pytest.mark.parametrize("mask", sorted(MASK_DIRS, reverse=True))
@pytest.mark.parametrize("ny,w", [(46, 20), (46, 4), (333, 20), (333, 4)])
@pytest.mark.parametrize("width", ["gout", "gout+6", "gout+7", "2gout+100"])
@pytest.mark.parametrize("shared", [2, 4])
@pytest.mark.parametrize("k,exact", [(12, False), (16, False), (20, False), (20, True)])
def test_push_group_faces_kernel(k, exact, shared, width, ny, w, mask):
    if exact:
        # the exact form at K = 20, or at the largest K whose push-group kernel is built
        built = [kk for kk in KS if _supported(kk, shared)]
        if built:
            k = max(built)
    if not _supported(k, shared):
        pytest.skip(f"no push-group kernel for k={k}, {shared} strips (tb_push_shared_supported)")
    if ny < 2 * w + 2:
        pytest.skip("the kernel needs two segments clear of each other's face")
    _run_and_check(k, ny, _widths(k, shared)[width], mask, w, shared, exact, shared)


def test_group_widths():
    """GOUT of the group kernels, from the kernel's own constants."""
    got = {(k, nw): ops.jacobi5tb_shared_geom(k, nw)["GOUT"] for k in KS for nw in (2, 4)}
    assert got == {(12, 2): 472, (16, 2): 464, (20, 2): 448, (12, 4): 952, (16, 4): 936, (20, 4): 920}


@pytest.mark.parametrize("k", KS)
def test_push_narrow_rect_falls_back_to_per_strip(k):
    """A rect narrower than a group: shared=4 is asked for, the per-strip
    push kernel runs, bitwise."""
    nx = ops.jacobi5tb_shared_geom(k, 4)["GOUT"] - 2
    _run_and_check(k, 130, nx, 15, 20, 4, False, 0)


@pytest.mark.parametrize("k,strips", [(18, 4), (4, 2)] + [(k, nw) for k in KS for nw in (2, 4)])
def test_push_unsupported_combination_falls_back(k, strips):
    """A (k, strips) without a push-group kernel (K = 18 and 4 have no group
    kernel at all): path 0, per-strip push, bitwise."""
    if _supported(k, strips):
        pytest.skip("a push-group kernel is built for this combination")
    _run_and_check(k, 130, 1100, 15, 20, strips, False, 0)


def test_push_shared_supported_names_group_shapes_only():
    for k in (1, 4, 10, 14, 18):  # no group kernel, or no push kernel (14)
        assert not ops.tb_push_shared_supported(k, 2) and not ops.tb_push_shared_supported(k, 4)
    for k in KS:
        assert not ops.tb_push_shared_supported(k, 3) and not ops.tb_push_shared_supported(k, 8)


def test_default_push_pass_stays_per_strip():
    """shared unset: a push pass is a per-strip launch, whatever its width."""
    for k in KS:
        dom = (XO, 2100, k, 333)
        assert ops.jacobi5tb_shared_path(k, [dom], 15, push_w=20) == 0
        assert ops.jacobi5tb_shared_path(k, [dom], 15, shared=-1, push_w=20) == 0
        # (the plain pass of the same rect takes its default group launch)
        assert ops.jacobi5tb_shared_path(k, [dom], 15) == 4


@pytest.fixture(scope="module")
def env():
    from gpu_mpi_tests_amd.parallel import dist as gd

    return gd.init(device="cuda")


@pytest.mark.parametrize("ny,nx,steps,k,nw", [(300, 1000, 43, 20, 4), (300, 920, 43, 20, 4), (257, 1031, 29, 12, 2)])
def test_push_group_engine_one_rank_periodic(env, ny, nx, steps, k, nw):
    """The engine's inline halo in group launches on one periodic GPU rank:
    every face lands in the pass's own next input; bitwise equal to the
    serial solve."""
    import numpy as np

    from gpu_mpi_tests_amd import engine

    if not _supported(k, nw):
        pytest.skip(f"no push-group kernel for k={k}, {nw} strips")
    e = engine.NativeJacobi(ny, nx, env, periodic=True, overlap=False, graph=False, tblock=k, push=True, shared=nw,
                            transport="local", init="random", seed=5)
    try:
        assert e.push_active
        assert e.tb_launch(k)["shared_strips"] == nw, e.tb_launch(k)
        e.run(steps)
        e.synchronize()
        got = e.interior()
    finally:
        e.close()
    want = engine.serial_jacobi(ny, nx, steps, True, init="random", seed=5)
    assert np.array_equal(got, want), float(np.abs(got - want).max())


def test_engine_rejects_a_bad_shared_value(env):
    from gpu_mpi_tests_amd import engine

    with pytest.raises(ValueError):
        engine.NativeJacobi(300, 1000, env, periodic=True, tblock=20, push=True, shared=3, transport="local")


@pytest.mark.parametrize("np_,ny,nx,steps,periodic,k,dims,shared", [
    (2, 400, 2000, 45, True, 20, "1x2", 4),
    (4, 600, 1900, 33, False, 20, "2x2", 4),
    (4, 500, 1000, 29, False, 12, "2x2", 2),
])
def test_push_group_engine_ranks_sharing_the_gpu(np_, ny, nx, steps, periodic, k, dims, shared):
    """np_ ranks on cuda:0 over IPC mappings, every pass a push-group launch:
    bitwise equal to the serial solve, residual identical on every rank,
    every rank launching groups of the requested size."""
    if not _supported(k, shared):
        pytest.skip(f"no push-group kernel for k={k}, {shared} strips")
    port = str(free_port())
    cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(np_), "--master-addr", "127.0.0.1", "--master-port", port,
           os.path.join(ROOT, "tests", "engine_push_shared_worker.py"), str(ny), str(nx), str(steps),
           "1" if periodic else "0", str(k), dims, str(shared)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd=ROOT,
                       env=dict(os.environ, OMP_NUM_THREADS="1", GMT_TRANSPORT="ipc", GMT_TEST_DEVICE="cuda"))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["push"] and r["diff"] == 0.0 and r["resid_same"], r
    assert r["shared_strips"] == [shared] * np_, r
