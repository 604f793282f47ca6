"""Cases and NumPy fp64 model of the Chebyshev step (gmt_cheby_step), shared by
tests/test_cheby_kernels_gpu.py (the gfx950 kernels) and
tests/test_cheby_kernels_cpu.py (the CPU backend: this file run as a program in
a child process, because build/lib-host/libgmt.so shares its SONAME with the
GPU library).

Both run the C ABI through the small `impl` of tests/cg_cases.py.  v' is
bitwise NumPy's (no contraction anywhere in the cell).  Everything outside u's
plus-shaped read set is NaN, everything outside the region of v and f a
sentinel that must be bitwise intact afterwards, and u and f must be bitwise
unchanged.  Only the all-aligned variant may take the row walk; the path of
every case is asserted where the backend has one."""
import ctypes
import json
import sys
import types

import numpy as np

import cg_cases as cc
import resid_cases as rc

NXS = rc.NXS
C0, C1 = 0.25, 1.0  # the engine's coefficients
SENTINEL = cc.SENTINEL
WEIGHTS = (1.0, 1.9, 0.0)  # the first iteration's, a typical one, and the identity on v
ALIGN = cc.aligns("uv")
ALIGN_F = cc.aligns("uv", extra="f")
PATH_NONE, PATH_SCALAR, PATH_ROW_WALK = cc.PATH_NONE, cc.PATH_SCALAR, cc.PATH_ROW_WALK
same_bits = cc.same_bits


def fields(nx, ny, align, with_f, seed=0):
    x0, odd, base = (ALIGN_F if with_f else ALIGN)[align]
    y0 = 2
    rows = y0 + ny + 2  # one NaN row beyond the ring on either side
    g = cc._rng("cheby", nx, ny, seed)
    u = cc.Field(rows, x0 + nx + 3, "u" in odd, "u" in base, np.nan)
    U = u.a
    U[y0:y0 + ny, x0:x0 + nx] = g.random((ny, nx)) - 0.5
    U[y0:y0 + ny, x0 - 1] = g.random(ny)
    U[y0:y0 + ny, x0 + nx] = g.random(ny)
    U[y0 - 1, x0:x0 + nx] = g.random(nx)
    U[y0 + ny, x0:x0 + nx] = g.random(nx)
    v = cc.Field(rows, x0 + nx + 1, "v" in odd, "v" in base, SENTINEL)
    v.a[y0:y0 + ny, x0:x0 + nx] = g.random((ny, nx)) - 0.5
    f = None
    if with_f:
        f = cc.Field(rows, x0 + nx, "f" in odd, 0, SENTINEL)
        f.a[y0:y0 + ny, x0:x0 + nx] = g.random((ny, nx)) - 0.5
    return u, v, f, (x0, nx, y0, ny)


def reference(region, u, v, f, w, c0=C0, c1=C1):
    """v' over the region in the operation order of the kernels."""
    x0, nx, y0, ny = region
    U = u.a
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    o = c0 * ((U[ys, x0 - 1:x0 - 1 + nx] + U[ys, x0 + 1:x0 + 1 + nx]) + (U[y0 - 1:y0 - 1 + ny, xs] + U[y0 + 1:y0 + 1 + ny, xs]))
    if f is not None:
        o = o + c1 * f.a[ys, xs]
    pv = v.a[ys, xs]
    t = o - pv
    return pv + w * t


def call(impl, region, u, v, f, w, c0=C0, c1=C1):
    d = cc.Dev(impl, u=u, v=v, f=f)
    x0, nx, y0, ny = region
    code = impl.lib.gmt_cheby_step(x0, nx, y0, ny, d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"), c0, c1, w,
                                   d.ptr("v"), d.ld("v"), impl.stream)
    assert code == 0, code
    d.fetch()


def path(impl, region, u, v, f=None):
    d = cc.Dev(impl, u=u, v=v, f=f)
    seg = ctypes.c_int64(-1)
    p = impl.lib.gmt_cheby_step_path(region[0], region[1], region[3], d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"),
                                     d.ptr("v"), d.ld("v"), ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(p), int(seg.value)


def seg_rows(impl, nx):
    """Rows per segment of the row walk for this width (8 on a backend without kernels)."""
    if not impl.has_paths:
        return 8
    u, v, _, region = fields(nx, 1, "fast", False)
    p, seg = path(impl, region, u, v)
    assert p == PATH_ROW_WALK and seg >= 2, (p, seg)
    return seg


def check(impl, nx, ny, align, with_f, w, seg=None, seed=0):
    what = ("cheby", nx, ny, align, with_f, w)
    u, v, f, region = fields(nx, ny, align, with_f, seed)
    x0, _, y0, _ = region
    if impl.has_paths:
        p, s = path(impl, region, u, v, f)
        fast = align == "fast"
        assert p == (PATH_ROW_WALK if fast else PATH_SCALAR), (what, p)
        assert s == (seg if fast else 0), (what, s, seg)
    ubefore, vbefore = u.store.copy(), v.store.copy()
    fbefore = None if f is None else f.store.copy()
    want = reference(region, u, v, f, w)
    call(impl, region, u, v, f, w)
    assert same_bits(ubefore, u.store), what                      # u is never written
    assert f is None or same_bits(fbefore, f.store), what
    V = v.a
    assert same_bits(V[y0:y0 + ny, x0:x0 + nx], want), what       # bitwise NumPy
    if w == 0.0:                                                  # v + 0*t: bitwise v
        old = vbefore[v.off:v.off + v.rows * v.ld].reshape(v.rows, v.ld)
        assert same_bits(V[y0:y0 + ny, x0:x0 + nx], old[y0:y0 + ny, x0:x0 + nx]), what
    V[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (v.store == SENTINEL).all(), what                      # nothing outside the region is written


def run_shapes(impl, nx, with_f):
    L = seg_rows(impl, nx)
    n = 0
    for align in (ALIGN_F if with_f else ALIGN):
        for ny in rc.ny_list(L):
            for w in WEIGHTS:
                check(impl, nx, ny, align, with_f, w, L)
                n += 1
    return n


def run_empty_and_refusals(impl):
    """An empty region launches nothing and returns 0; the refused calls, with their codes."""
    L = impl.lib
    u, v, f, (x0, nx, y0, ny) = fields(5, 4, "fast", True)
    d = cc.Dev(impl, u=u, v=v, f=f)

    def step(x0=x0, nx=nx, y0=y0, ny=ny, pu=d.ptr("u"), ld=u.ld, pf=d.ptr("f"), ldf=f.ld, pv=d.ptr("v"), ldv=v.ld):
        return L.gmt_cheby_step(x0, nx, y0, ny, pu, ld, pf, ldf, C0, C1, 1.5, pv, ldv, impl.stream)

    for enx, eny in ((0, 4), (5, 0), (0, 0)):
        assert step(nx=enx, ny=eny) == 0
    codes = [step(pu=None), step(pv=None), step(nx=-1), step(ny=-1), step(nx=-1, ny=0), step(x0=0), step(y0=0),
             step(ld=x0 + nx), step(ldv=x0 + nx - 1), step(ldf=x0 + nx - 1)]
    # nothing was written by the empty or the refused calls
    before = v.store.copy()
    d.fetch()
    assert same_bits(v.store, before)
    assert step(pf=None, ldf=0) == 0  # f is optional
    return [int(c) for c in codes]


N_REFUSALS = 10


def host_impl(lib):
    from gpu_mpi_tests_amd import _native

    _native.bind(lib, [n for n in _native._SIGS if n.startswith("gmt_cheby_")])
    return types.SimpleNamespace(lib=lib, stream=None, has_paths=False, upload=lambda a: a.copy(),
                                 download=lambda h: h.copy(), ptr=lambda h: h.ctypes.data)


def main():
    """Every check through the CPU backend; prints one JSON line."""
    impl = host_impl(ctypes.CDLL(sys.argv[1]))
    n = 0
    for nx in NXS:
        for with_f in (False, True):
            n += run_shapes(impl, nx, with_f)
    codes = run_empty_and_refusals(impl)
    u, v, _, region = fields(100, 100, "fast", False)
    print(json.dumps(dict(ok=True, cases=n, codes=codes, paths=[path(impl, region, u, v)])))


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
