"""Cases and NumPy fp64 model of the fused residual + full weighting
(gmt_mg_resid_restrict), shared by tests/test_mg_resid_kernels_gpu.py (the
gfx950 kernels) and tests/test_mg_resid_kernels_cpu.py (the CPU backend: this
file run as a program in a child process, because build/lib-host/libgmt.so
shares its SONAME with the GPU library).  The conventions of
tests/mg_fuse_cases.py: the C ABI through the small `impl` of tests/cg_cases.py;
everything outside the stated read sets of u and f is NaN (u: the region plus 2
cells beyond a set side and 1 beyond a clear side, without the outermost corner
cell where two set sides meet; f: the region plus 1 cell beyond set sides);
sc is a sentinel outside its mx x my cells that must be bitwise intact
afterwards; inputs must be bitwise unchanged; sc is bitwise
ops/reference.py's mg_resid_restrict (cg_apply on the grown box into a zeroed
field, then mg_restrict); only the all-aligned variant may take the walk and
the path of every case is asserted where the backend has one.

Widths come from gmt_mg_resid_restrict_geom (the lane-pair tail, the seams
between waves and workgroups, where neighbouring waves overlap), heights from
the rows per segment L that the path query reports (regions shorter than the
warm-up, and the segment seams)."""
import ctypes
import json
import sys
import types

import numpy as np

import cg_cases as cc
import mg_cases as mc

C0, C1, CS = mc.C0, mc.C1, mc.CS
SENTINEL = cc.SENTINEL
MASKS = (0, 15, 5, 10)
PARITIES = mc.PARITIES
HOST_SEG = 8   # a segment length of the walk: the heights of a backend without kernels
Y0, CY0 = 3, 1  # room for 2 halo rows and one NaN row below them
# name -> (fine x0, coarse cx0, fields with an odd pitch, fields whose base is off by 8 B)
ALIGN = {"fast": (8, 8, (), ()), "odd_x0": (9, 8, (), ()), "odd_cx0": (8, 9, (), ()),
         "u_odd_ld": (8, 8, ("u",), ()), "u_base_8B": (8, 8, (), ("u",)),
         "s_odd_ld": (8, 8, ("s",), ()), "s_base_8B": (8, 8, (), ("s",))}
ALIGN_F = dict(ALIGN, f_odd_ld=(8, 8, ("f",), ()), f_base_8B=(8, 8, (), ("f",)))
PATH_NONE, PATH_SCALAR, PATH_ROW_WALK = cc.PATH_NONE, cc.PATH_SCALAR, cc.PATH_ROW_WALK
same_bits = cc.same_bits


def ref():
    from gpu_mpi_tests_amd.ops import reference

    return reference


def geom(impl):
    wc, bc = ctypes.c_int64(0), ctypes.c_int64(0)
    code = impl.lib.gmt_mg_resid_restrict_geom(ctypes.cast(ctypes.pointer(wc), ctypes.c_void_p),
                                               ctypes.cast(ctypes.pointer(bc), ctypes.c_void_p))
    assert code == 0, code
    return int(wc.value), int(bc.value)


def widths(impl):
    w, b = geom(impl)
    return (1, 2, 3, w - 1, w, w + 1, b - 1, b + 1, 2 * b + 3)


def heights(L):
    return tuple(sorted({1, 2, 3, L - 1, L, L + 1, 2 * L + 1}))


def grow(mask, g):
    """(west, east, south, north) cells beyond the region: g on a set side, 1 on a clear one."""
    return tuple(g if mask & bit else 1 for bit in (1, 2, 4, 8))


def fields(nx, ny, mask, par, align, with_f):
    x0, cx0, odd, base = (ALIGN_F if with_f else ALIGN)[align]
    y0, cy0 = Y0, CY0
    px, py = par
    mx, my = mc.coarse_extent(nx, px), mc.coarse_extent(ny, py)
    gw, ge, gs, gn = grow(mask, 2)
    rows = y0 + ny + 3
    g = cc._rng("mg_resid_restrict", nx, ny, mask, par)
    u = cc.Field(rows, x0 + nx + 3, "u" in odd, "u" in base, np.nan)
    u.a[y0 - gs:y0 + ny + gn, x0 - gw:x0 + nx + ge] = g.random((ny + gs + gn, nx + gw + ge)) - 0.5
    for sx, cx in ((gw, x0 - 2), (ge, x0 + nx + 1)):      # the outermost corner where two set sides meet
        for sy, cy in ((gs, y0 - 2), (gn, y0 + ny + 1)):
            if sx == 2 and sy == 2:
                u.a[cy, cx] = np.nan
    s = cc.Field(cy0 + my + 1, cx0 + mx + 1, "s" in odd, "s" in base, SENTINEL)
    f = None
    if with_f:
        f = cc.Field(rows, x0 + nx + 2, "f" in odd, "f" in base, np.nan)
        fw, fe, fs, fn = (t - 1 for t in (gw, ge, gs, gn))
        f.a[y0 - fs:y0 + ny + fn, x0 - fw:x0 + nx + fe] = g.random((ny + fs + fn, nx + fw + fe)) - 0.5
    return u, s, f, (x0, nx, y0, ny), (cx0, cy0, mx, my)


def reference(region, par, mask, coarse, u, f):
    x0, nx, y0, ny = region
    cx0, cy0, mx, my = coarse
    out = np.full((cy0 + my + 1, cx0 + mx + 1), SENTINEL)
    ref().mg_resid_restrict(u.a, out, CS, x0, nx, y0, ny, par[0], par[1], mask, cx0, cy0, None if f is None else f.a,
                            C0, C1)
    want = out[cy0:cy0 + my, cx0:cx0 + mx].copy()
    out[cy0:cy0 + my, cx0:cx0 + mx] = SENTINEL
    assert (out == SENTINEL).all()  # the model writes the coarse cells only
    return want


def path(impl, region, par, mask, coarse, u, s, f=None):
    d = cc.Dev(impl, u=u, s=s, f=f)
    seg = ctypes.c_int64(-1)
    x0, nx, y0, ny = region
    p = impl.lib.gmt_mg_resid_restrict_path(x0, nx, y0, ny, par[0], par[1], mask, d.ptr("u"), d.ld("u"), d.ptr("f"),
                                            d.ld("f"), d.ptr("s"), coarse[0], coarse[1], d.ld("s"),
                                            ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(p), int(seg.value)


def seg_rows(impl, nx):
    """Fine rows per segment of the walk for this width (HOST_SEG on a backend without kernels)."""
    if not impl.has_paths:
        return HOST_SEG
    u, s, _, region, coarse = fields(nx, 1, 0, (0, 0), "fast", False)
    p, seg = path(impl, region, (0, 0), 0, coarse, u, s)
    assert p == PATH_ROW_WALK and seg >= 4 and seg % 2 == 0, (p, seg)
    return seg


def call(impl, region, par, mask, coarse, u, s, f, c0=C0, c1=C1, cs=CS):
    x0, nx, y0, ny = region
    d = cc.Dev(impl, u=u, s=s, f=f)
    code = impl.lib.gmt_mg_resid_restrict(x0, nx, y0, ny, par[0], par[1], mask, d.ptr("u"), d.ld("u"), d.ptr("f"),
                                          d.ld("f"), c0, c1, cs, d.ptr("s"), coarse[0], coarse[1], d.ld("s"),
                                          impl.stream)
    d.fetch()
    return int(code)


def check(impl, nx, ny, mask, par, align, with_f, seg=None):
    what = ("mg_resid_restrict", nx, ny, mask, par, align, with_f)
    u, s, f, region, coarse = fields(nx, ny, mask, par, align, with_f)
    cx0, cy0, mx, my = coarse
    if impl.has_paths:
        p, sg = path(impl, region, par, mask, coarse, u, s, f)
        fast = align == "fast"
        assert p == (PATH_ROW_WALK if fast else PATH_SCALAR), (what, p)
        assert sg == (seg if fast else 0), (what, sg, seg)
    ubefore = u.store.copy()
    fbefore = None if f is None else f.store.copy()
    want = reference(region, par, mask, coarse, u, f)
    assert want.shape == (my, mx) and not np.isnan(want).any(), what  # the model stays inside the read sets
    assert call(impl, region, par, mask, coarse, u, s, f) == 0, what
    assert same_bits(ubefore, u.store), what                          # u is never written
    assert f is None or same_bits(fbefore, f.store), what
    got = s.a[cy0:cy0 + my, cx0:cx0 + mx]
    if not same_bits(got, want):
        bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
        raise AssertionError((what, "coarse cells (row, column) that differ", len(bad), bad[:8].tolist()))
    s.a[cy0:cy0 + my, cx0:cx0 + mx] = SENTINEL
    assert (s.store == SENTINEL).all(), what                          # nothing but the coarse cells is written


# ------------------------------------------------------------------ the cases
def run_all_masks(impl):
    """All 16 masks x every parity x with and without f on 37 x 11, on the walk and on the scalar kernel."""
    n = 0
    L = seg_rows(impl, 37)
    for mask in range(16):
        for par in PARITIES:
            for with_f in (False, True):
                check(impl, 37, 11, mask, par, "fast", with_f, L)
                check(impl, 37, 11, mask, par, "odd_x0", with_f)
                n += 2
    return n


N_ALL_MASKS = 16 * 4 * 2 * 2


def _sweep(impl, nx, ny, L):
    n = 0
    for mask in MASKS:
        for par in PARITIES:
            for with_f in (False, True):
                check(impl, nx, ny, mask, par, "fast", with_f, L)
                n += 1
    return n


N_SWEEP = len(MASKS) * len(PARITIES) * 2


def run_width(impl, nx):
    """One width of the geometry's list at a height below the warm-up and across a segment seam."""
    L = seg_rows(impl, nx)
    return sum(_sweep(impl, nx, ny, L) for ny in (2, L + 1))


def run_height(impl, ih):
    """One height of the segment's list at the lane-pair tail and across a wave seam."""
    w, _ = geom(impl)
    n = 0
    for nx in (3, w + 1):
        L = seg_rows(impl, nx)
        n += _sweep(impl, nx, heights(L)[ih], L)
    return n


N_HEIGHTS = 7


def scalar_shapes(impl):
    w, _ = geom(impl)
    return ((1, 1), (2, 2), (3, 3), (w + 1, 2), (5, HOST_SEG + 1))


def run_scalar_shapes(impl):
    """The alignment variants that must take the one-lane-per-coarse-cell kernel."""
    n = 0
    for with_f in (False, True):
        for align in (ALIGN_F if with_f else ALIGN):
            if align == "fast":
                continue
            for i, (nx, ny) in enumerate(scalar_shapes(impl)):
                for mask in MASKS:
                    check(impl, nx, ny, mask, PARITIES[(i + mask) % 4], align, with_f)
                    n += 1
    return n


N_SCALAR = (len(ALIGN) - 1 + len(ALIGN_F) - 1) * 5 * len(MASKS)


# ---------------------------------------------------------------- identities
def _two_calls(impl, region, par, coarse, u, f, box):
    """gmt_cg_apply mode 1 over `box` into a zeroed field, then gmt_mg_restrict over the region."""
    x0, nx, y0, ny = region
    cx0, cy0, mx, my = coarse
    d = cc.Field(u.rows, u.ld, False, 0, 0.0)
    s = cc.Field(cy0 + my + 1, cx0 + mx + 1, False, 0, SENTINEL)
    dev = cc.Dev(impl, u=u, d=d, s=s, f=f)
    bx, bnx, by, bny = box
    code, _ = cc._with_ws(impl, (bx, bnx, by, bny), lambda o, w: impl.lib.gmt_cg_apply(
        1, bx, bnx, by, bny, dev.ptr("u"), dev.ld("u"), dev.ptr("f"), dev.ld("f"), C0, C1 if f is not None else 0.0,
        dev.ptr("d"), dev.ld("d"), o, w, impl.stream))
    assert code == 0, code
    code = impl.lib.gmt_mg_restrict(x0, nx, y0, ny, par[0], par[1], dev.ptr("d"), dev.ld("d"), CS, dev.ptr("s"), cx0,
                                    cy0, dev.ld("s"), impl.stream)
    assert code == 0, code
    dev.fetch()
    return s.a[cy0:cy0 + my, cx0:cx0 + mx].copy()


def run_identities(impl):
    """Mask 0 is the two existing calls with d's ring zero; mask 15 the same with the ring of d computed from
    the wider field.  Run through the backend's own kernels."""
    w, _ = geom(impl)
    n = 0
    for align in ("fast", "odd_x0"):
        for with_f in (False, True):
            for nx, ny in ((w + 3, 7), (6, 2 * HOST_SEG + 2)):
                for par in PARITIES:
                    for mask in (0, 15):
                        u, s, f, region, coarse = fields(nx, ny, mask, par, align, with_f)
                        x0, _, y0, _ = region
                        cx0, cy0, mx, my = coarse
                        assert call(impl, region, par, mask, coarse, u, s, f) == 0
                        g = 1 if mask else 0
                        two = _two_calls(impl, region, par, coarse, u, f, (x0 - g, nx + 2 * g, y0 - g, ny + 2 * g))
                        assert same_bits(s.a[cy0:cy0 + my, cx0:cx0 + mx], two), (align, with_f, nx, ny, par, mask)
                        n += 1
    return n


# --------------------------------------------------------- empty and refused
def run_empty_and_refusals(impl):
    """An empty region launches nothing and returns 0; the refused calls, with their codes; sc stays intact."""
    L = impl.lib
    u, s, f, (x0, nx, y0, ny), (cx0, cy0, mx, my) = fields(5, 4, 15, (1, 1), "fast", True)
    d = cc.Dev(impl, u=u, s=s, f=f)

    def rr(x0=x0, nx=nx, y0=y0, ny=ny, px=1, py=1, mask=15, pu=d.ptr("u"), ld=u.ld, pf=d.ptr("f"), ldf=f.ld,
           ps=d.ptr("s"), cx0=cx0, cy0=cy0, ldc=s.ld):
        return L.gmt_mg_resid_restrict(x0, nx, y0, ny, px, py, mask, pu, ld, pf, ldf, C0, C1, CS, ps, cx0, cy0, ldc,
                                       impl.stream)

    for enx, eny in ((0, 4), (5, 0), (0, 0)):
        assert rr(nx=enx, ny=eny) == 0
    assert rr(nx=1, px=1) == 0 and rr(ny=1, py=1) == 0                             # no coarse point on the region
    codes = [rr(pu=None), rr(ps=None), rr(nx=-1), rr(ny=-1), rr(nx=-1, ny=0),       # gmt_cg_apply's
             rr(mask=0, x0=0), rr(mask=0, y0=0), rr(mask=0, ld=x0 + nx), rr(mask=0, ldf=x0 + nx - 1),
             rr(px=2), rr(px=-1), rr(py=2), rr(py=-1), rr(cx0=-1), rr(cy0=-1),      # gmt_mg_restrict's
             rr(ldc=cx0 + mx - 1),
             rr(mask=-1), rr(mask=16),                                              # the mask
             rr(mask=1, x0=1), rr(mask=4, y0=1),                                    # the read set's room
             rr(mask=2, ld=x0 + nx + 1), rr(mask=2, ldf=x0 + nx),                   # its pitches
             rr(ps=d.ptr("u")), rr(ps=d.ptr("u") + 8 * u.ld * 2), rr(ps=d.ptr("f") + 8 * f.ld * 3)]  # shared storage
    before = s.store.copy()
    ub, fb = u.store.copy(), f.store.copy()
    d.fetch()
    assert same_bits(s.store, before) and same_bits(u.store, ub) and same_bits(f.store, fb)
    assert rr(pf=None, ldf=0) == 0                                                  # f is optional
    assert rr(mask=1, x0=2) == 0 and rr(mask=0, x0=1, y0=1) == 0                    # the least room that is enough
    assert rr(mask=2, ld=x0 + nx + 2, ldf=x0 + nx + 1) == 0
    return [int(c) for c in codes]


N_REFUSALS = 25


def host_impl(lib):
    from gpu_mpi_tests_amd import _native

    _native.bind(lib, [n for n in _native._SIGS if n.startswith("gmt_mg_") or n.startswith("gmt_cg_")])
    return types.SimpleNamespace(lib=lib, stream=None, has_paths=False, upload=lambda a: a.copy(),
                                 download=lambda h: h.copy(), ptr=lambda h: h.ctypes.data)


def main():
    """Every check through the CPU backend; prints one JSON line."""
    impl = host_impl(ctypes.CDLL(sys.argv[1]))
    n = [run_all_masks(impl), sum(run_width(impl, nx) for nx in widths(impl)),
         sum(run_height(impl, ih) for ih in range(N_HEIGHTS)), run_scalar_shapes(impl), run_identities(impl)]
    codes = run_empty_and_refusals(impl)
    u, s, _, region, coarse = fields(100, 40, 0, (1, 1), "fast", False)
    print(json.dumps(dict(ok=True, cases=n, codes=codes, path=list(path(impl, region, (1, 1), 0, coarse, u, s)),
                          geom=list(geom(impl)))))


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
