"""Cases and NumPy fp64 model of the multigrid kernels (gmt_mg_smooth,
gmt_mg_restrict, gmt_mg_prolong_add), shared by tests/test_mg_kernels_gpu.py
(the gfx950 kernels) and tests/test_mg_kernels_cpu.py (the CPU backend: this
file run as a program in a child process, because build/lib-host/libgmt.so
shares its SONAME with the GPU library).

Both run the C ABI through the small `impl` of tests/cg_cases.py.  Outputs are
bitwise the model's (no contraction anywhere in a cell).  Everything outside a
kernel's documented read set is NaN, everything outside its output region a
sentinel that must be bitwise intact afterwards, and inputs must be bitwise
unchanged.  Only the all-aligned variant may take the fast path; the path of
every case is asserted where the backend has one.

The transfer kernels have no row segments (one lane per pair of coarse / fine
cells, lanes numbered row by row), so their heights are 1, 2, 3 fine rows and
the rows around which a 256-lane workgroup wraps for the widths used."""
import ctypes
import json
import sys
import types

import numpy as np

import cg_cases as cc
import resid_cases as rc

NXS = rc.NXS
C0, C1 = 0.25, 1.0  # the engine's coefficients
CS = 0.25           # and its restriction scale
SENTINEL = cc.SENTINEL
OMEGAS = (0.8, 1.0, 0.0)  # the default, plain Jacobi, and the identity on u
ALIGN = cc.aligns("uo")
ALIGN_F = cc.aligns("uo", extra="f")
# transfer kernels: name -> (fine x0, coarse cx0, fields with an odd pitch, fields whose base is off by 8 B)
ALIGN_R = {"fast": (8, 8, (), ()), "odd_x0": (9, 8, (), ()), "odd_cx0": (8, 9, (), ()),
           "d_odd_ld": (8, 8, ("d",), ()), "d_base_8B": (8, 8, (), ("d",)),
           "s_odd_ld": (8, 8, ("s",), ()), "s_base_8B": (8, 8, (), ("s",))}
ALIGN_P = {"fast": (8, 3, (), ()), "odd_x0": (9, 3, (), ()),
           "e_odd_ld": (8, 3, ("e",), ()), "e_base_8B": (8, 3, (), ("e",)),
           "u_odd_ld": (8, 3, ("u",), ()), "u_base_8B": (8, 3, (), ("u",))}
PARITIES = ((0, 0), (0, 1), (1, 0), (1, 1))
TRANSFER_NYS = (1, 2, 3, 4, 5, 8, 9)
PATH_NONE, PATH_SCALAR, PATH_PT, PATH_ROW_WALK = cc.PATH_NONE, cc.PATH_SCALAR, cc.PATH_PT, cc.PATH_ROW_WALK
same_bits = cc.same_bits


def coarse_extent(n, p):
    return (n - p + 1) // 2


# ------------------------------------------------------------------ smoother
def smooth_fields(nx, ny, align, with_f, seed=0):
    x0, odd, base = (ALIGN_F if with_f else ALIGN)[align]
    y0 = 2
    rows = y0 + ny + 2  # one NaN row beyond the ring on either side
    g = cc._rng("mg_smooth", nx, ny, seed)
    u = cc.Field(rows, x0 + nx + 3, "u" in odd, "u" in base, np.nan)
    U = u.a
    U[y0:y0 + ny, x0:x0 + nx] = g.random((ny, nx)) - 0.5
    U[y0:y0 + ny, x0 - 1] = g.random(ny)
    U[y0:y0 + ny, x0 + nx] = g.random(ny)
    U[y0 - 1, x0:x0 + nx] = g.random(nx)
    U[y0 + ny, x0:x0 + nx] = g.random(nx)
    o = cc.Field(rows, x0 + nx + 1, "o" in odd, "o" in base, SENTINEL)
    f = None
    if with_f:
        f = cc.Field(rows, x0 + nx, "f" in odd, 0, SENTINEL)
        f.a[y0:y0 + ny, x0:x0 + nx] = g.random((ny, nx)) - 0.5
    return u, o, f, (x0, nx, y0, ny)


def smooth_reference(region, u, f, om, c0=C0, c1=C1):
    x0, nx, y0, ny = region
    U = u.a
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    o = c0 * ((U[ys, x0 - 1:x0 - 1 + nx] + U[ys, x0 + 1:x0 + 1 + nx]) + (U[y0 - 1:y0 - 1 + ny, xs] + U[y0 + 1:y0 + 1 + ny, xs]))
    if f is not None:
        o = o + c1 * f.a[ys, xs]
    c = U[ys, xs]
    t = o - c
    return c + om * t


def smooth_path(impl, region, u, o, f=None):
    d = cc.Dev(impl, u=u, o=o, f=f)
    seg = ctypes.c_int64(-1)
    p = impl.lib.gmt_mg_smooth_path(region[0], region[1], region[3], d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"),
                                    d.ptr("o"), d.ld("o"), ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(p), int(seg.value)


def smooth_seg_rows(impl, nx):
    """Rows per segment of the row walk for this width (8 on a backend without kernels)."""
    if not impl.has_paths:
        return 8
    u, o, _, region = smooth_fields(nx, 1, "fast", False)
    p, seg = smooth_path(impl, region, u, o)
    assert p == PATH_ROW_WALK and seg >= 2, (p, seg)
    return seg


def check_smooth(impl, nx, ny, align, with_f, om, seg=None):
    what = ("mg_smooth", nx, ny, align, with_f, om)
    u, o, f, region = smooth_fields(nx, ny, align, with_f)
    x0, _, y0, _ = region
    if impl.has_paths:
        p, s = smooth_path(impl, region, u, o, f)
        fast = align == "fast"
        assert p == (PATH_ROW_WALK if fast else PATH_SCALAR), (what, p)
        assert s == (seg if fast else 0), (what, s, seg)
    ubefore = u.store.copy()
    fbefore = None if f is None else f.store.copy()
    want = smooth_reference(region, u, f, om)
    d = cc.Dev(impl, u=u, o=o, f=f)
    code = impl.lib.gmt_mg_smooth(x0, nx, y0, ny, d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"), C0, C1, om,
                                  d.ptr("o"), d.ld("o"), impl.stream)
    assert code == 0, (what, code)
    d.fetch()
    assert same_bits(ubefore, u.store), what                      # u is never written
    assert f is None or same_bits(fbefore, f.store), what
    O = o.a
    assert same_bits(O[y0:y0 + ny, x0:x0 + nx], want), what       # bitwise NumPy
    if om == 0.0:                                                 # u + 0*t: bitwise u
        assert same_bits(O[y0:y0 + ny, x0:x0 + nx], u.a[y0:y0 + ny, x0:x0 + nx]), what
    O[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (o.store == SENTINEL).all(), what                      # nothing outside the region is written


def run_smooth_shapes(impl, nx, with_f):
    L = smooth_seg_rows(impl, nx)
    n = 0
    for align in (ALIGN_F if with_f else ALIGN):
        for ny in rc.ny_list(L):
            for om in OMEGAS:
                check_smooth(impl, nx, ny, align, with_f, om, L)
                n += 1
    return n


# --------------------------------------------------------------- restriction
def restrict_fields(nx, ny, px, py, align, const=None):
    x0, cx0, odd, base = ALIGN_R[align]
    y0, cy0 = 2, 1
    mx, my = coarse_extent(nx, px), coarse_extent(ny, py)
    g = cc._rng("mg_restrict", nx, ny, px, py)
    d = cc.Field(y0 + ny + 2, x0 + nx + 3, "d" in odd, "d" in base, np.nan)  # NaN beyond the ring
    d.a[y0 - 1:y0 + ny + 1, x0 - 1:x0 + nx + 1] = g.random((ny + 2, nx + 2)) - 0.5 if const is None else const
    s = cc.Field(cy0 + my + 1, cx0 + mx + 1, "s" in odd, "s" in base, SENTINEL)
    return d, s, (x0, nx, y0, ny), (cx0, cy0), (mx, my)


def restrict_reference(d, region, px, py, mx, my, cs=CS):
    x0, _, y0, _ = region
    D = d.a
    out = np.empty((my, mx))
    xs = x0 + px + 2 * np.arange(mx)
    for J in range(my):
        y = y0 + py + 2 * J
        H = [(D[r, xs - 1] + D[r, xs + 1]) + 2.0 * D[r, xs] for r in (y - 1, y, y + 1)]
        out[J] = cs * ((H[0] + H[2]) + 2.0 * H[1])
    return out


def call_restrict(impl, d, s, region, px, py, coarse, cs=CS):
    dev = cc.Dev(impl, d=d, s=s)
    x0, nx, y0, ny = region
    code = impl.lib.gmt_mg_restrict(x0, nx, y0, ny, px, py, dev.ptr("d"), dev.ld("d"), cs, dev.ptr("s"), coarse[0],
                                    coarse[1], dev.ld("s"), impl.stream)
    assert code == 0, code
    dev.fetch()


def check_restrict(impl, nx, ny, px, py, align):
    what = ("mg_restrict", nx, ny, px, py, align)
    d, s, region, (cx0, cy0), (mx, my) = restrict_fields(nx, ny, px, py, align)
    if impl.has_paths:
        dev = cc.Dev(impl, d=d, s=s)
        p = impl.lib.gmt_mg_restrict_path(region[0], cx0, dev.ptr("d"), dev.ld("d"), dev.ptr("s"), dev.ld("s"))
        assert p == (PATH_PT if align == "fast" else PATH_SCALAR), (what, p)
    before = d.store.copy()
    want = restrict_reference(d, region, px, py, mx, my)
    call_restrict(impl, d, s, region, px, py, (cx0, cy0))
    assert same_bits(before, d.store), what
    S = s.a
    assert same_bits(S[cy0:cy0 + my, cx0:cx0 + mx], want), what
    S[cy0:cy0 + my, cx0:cx0 + mx] = SENTINEL
    assert (s.store == SENTINEL).all(), what


def run_restrict_shapes(impl, nx):
    n = 0
    for align in ALIGN_R:
        for px, py in PARITIES:
            for ny in TRANSFER_NYS:
                check_restrict(impl, nx, ny, px, py, align)
                n += 1
    return n


# ------------------------------------------------------------- interpolation
def prolong_fields(nx, ny, px, py, align, const=None):
    x0, cx0, odd, base = ALIGN_P[align]
    y0, cy0 = 1, 2
    mx, my = coarse_extent(nx, px), coarse_extent(ny, py)
    g = cc._rng("mg_prolong", nx, ny, px, py)
    e = cc.Field(cy0 + my + 2, cx0 + mx + 2, "e" in odd, "e" in base, np.nan)  # NaN beyond the ring
    e.a[cy0 - 1:cy0 + my + 1, cx0 - 1:cx0 + mx + 1] = g.random((my + 2, mx + 2)) - 0.5 if const is None else const
    u = cc.Field(y0 + ny + 1, x0 + nx + 1, "u" in odd, "u" in base, SENTINEL)
    u.a[y0:y0 + ny, x0:x0 + nx] = g.random((ny, nx)) - 0.5
    return e, u, (x0, nx, y0, ny), (cx0, cy0)


def prolong_reference(e, u, region, px, py, coarse):
    x0, nx, y0, ny = region
    cx0, cy0 = coarse
    E, U = e.a, u.a
    want = np.empty((ny, nx))
    di = np.arange(nx) - px
    onx = di % 2 == 0
    I = np.where(onx, di // 2, (di + 1) // 2 - 1) + cx0  # the column a cell sits on, else the one west of it
    for j in range(ny):
        dj = j - py
        ony = dj % 2 == 0
        J = (dj // 2 if ony else (dj + 1) // 2 - 1) + cy0
        if ony:
            t = np.where(onx, E[J, I], 0.5 * (E[J, I] + E[J, I + 1]))
        else:
            t = np.where(onx, 0.5 * (E[J, I] + E[J + 1, I]),
                         0.25 * ((E[J, I] + E[J, I + 1]) + (E[J + 1, I] + E[J + 1, I + 1])))
        want[j] = U[y0 + j, x0:x0 + nx] + t
    return want


def call_prolong(impl, e, u, region, px, py, coarse):
    dev = cc.Dev(impl, e=e, u=u)
    x0, nx, y0, ny = region
    code = impl.lib.gmt_mg_prolong_add(x0, nx, y0, ny, px, py, dev.ptr("e"), coarse[0], coarse[1], dev.ld("e"),
                                       dev.ptr("u"), dev.ld("u"), impl.stream)
    assert code == 0, code
    dev.fetch()


def check_prolong(impl, nx, ny, px, py, align):
    what = ("mg_prolong_add", nx, ny, px, py, align)
    e, u, region, coarse = prolong_fields(nx, ny, px, py, align)
    x0, _, y0, _ = region
    if impl.has_paths:
        dev = cc.Dev(impl, e=e, u=u)
        p = impl.lib.gmt_mg_prolong_add_path(x0, dev.ptr("e"), dev.ld("e"), dev.ptr("u"), dev.ld("u"))
        assert p == (PATH_PT if align == "fast" else PATH_SCALAR), (what, p)
    before = e.store.copy()
    want = prolong_reference(e, u, region, px, py, coarse)
    call_prolong(impl, e, u, region, px, py, coarse)
    assert same_bits(before, e.store), what
    U = u.a
    assert same_bits(U[y0:y0 + ny, x0:x0 + nx], want), what
    U[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (u.store == SENTINEL).all(), what


def run_prolong_shapes(impl, nx):
    n = 0
    for align in ALIGN_P:
        for px, py in PARITIES:
            for ny in TRANSFER_NYS:
                check_prolong(impl, nx, ny, px, py, align)
                n += 1
    return n


# ---------------------------------------------------------------- identities
def run_identities(impl):
    """A constant e = 1 (ring included) adds exactly 1 everywhere; a constant d = 1 restricts to exactly 4*cs."""
    for align_r, align_p in (("fast", "fast"), ("odd_x0", "odd_x0")):
        for px, py in PARITIES:
            for nx, ny in ((130, 9), (257, 4)):
                e, u, region, coarse = prolong_fields(nx, ny, px, py, align_p, const=1.0)
                x0, _, y0, _ = region
                old = u.a[y0:y0 + ny, x0:x0 + nx].copy()
                call_prolong(impl, e, u, region, px, py, coarse)
                assert same_bits(u.a[y0:y0 + ny, x0:x0 + nx], old + 1.0), (nx, ny, px, py)
                for cs in (CS, 0.0625, 0.3):
                    d, s, region, (cx0, cy0), (mx, my) = restrict_fields(nx, ny, px, py, align_r, const=1.0)
                    call_restrict(impl, d, s, region, px, py, (cx0, cy0), cs)
                    # cs*((4 + 4) + 2*4): 16 cs, 4 cs a fine point's share of each coarse point
                    assert same_bits(s.a[cy0:cy0 + my, cx0:cx0 + mx], np.full((my, mx), cs * 16.0)), (nx, ny, px, py)
                    assert cs * 16.0 == 4.0 * (4.0 * cs)


# --------------------------------------------------------- empty and refused
def run_empty_and_refusals(impl):
    """An empty region launches nothing and returns 0; the refused calls, with their codes."""
    L = impl.lib
    u, o, f, (x0, nx, y0, ny) = smooth_fields(5, 4, "fast", True)
    d = cc.Dev(impl, u=u, o=o, f=f)

    def sm(x0=x0, nx=nx, y0=y0, ny=ny, pu=d.ptr("u"), ld=u.ld, pf=d.ptr("f"), ldf=f.ld, po=d.ptr("o"), ldo=o.ld):
        return L.gmt_mg_smooth(x0, nx, y0, ny, pu, ld, pf, ldf, C0, C1, 0.8, po, ldo, impl.stream)

    for enx, eny in ((0, 4), (5, 0), (0, 0)):
        assert sm(nx=enx, ny=eny) == 0
    codes = [sm(pu=None), sm(po=None), sm(nx=-1), sm(ny=-1), sm(nx=-1, ny=0), sm(x0=0), sm(y0=0), sm(ld=x0 + nx),
             sm(ldo=x0 + nx - 1), sm(ldf=x0 + nx - 1)]
    before = o.store.copy()
    d.fetch()
    assert same_bits(o.store, before)
    assert sm(pf=None, ldf=0) == 0  # f is optional

    dd, s, (x0, nx, y0, ny), (cx0, cy0), (mx, my) = restrict_fields(5, 4, 1, 1, "fast")
    d = cc.Dev(impl, d=dd, s=s)

    def rs(x0=x0, nx=nx, y0=y0, ny=ny, px=1, py=1, pd=d.ptr("d"), ldd=dd.ld, ps=d.ptr("s"), cx0=cx0, cy0=cy0, ldc=s.ld):
        return L.gmt_mg_restrict(x0, nx, y0, ny, px, py, pd, ldd, CS, ps, cx0, cy0, ldc, impl.stream)

    for enx, eny in ((0, 4), (5, 0), (0, 0)):
        assert rs(nx=enx, ny=eny) == 0
    assert rs(nx=1, px=1) == 0 and rs(ny=1, py=1) == 0  # a region without a coarse point
    codes += [rs(pd=None), rs(ps=None), rs(nx=-1), rs(ny=-1), rs(x0=0), rs(y0=0), rs(px=2), rs(px=-1), rs(py=2),
              rs(py=-1), rs(cx0=-1), rs(cy0=-1), rs(ldd=x0 + nx), rs(ldc=cx0 + mx - 1)]
    before = s.store.copy()
    d.fetch()
    assert same_bits(s.store, before)

    e, u, (x0, nx, y0, ny), (cx0, cy0) = prolong_fields(5, 4, 1, 1, "fast")
    mx = coarse_extent(nx, 1)
    d = cc.Dev(impl, e=e, u=u)

    def pr(x0=x0, nx=nx, y0=y0, ny=ny, px=1, py=1, pe=d.ptr("e"), cx0=cx0, cy0=cy0, lde=e.ld, pu=d.ptr("u"), ld=u.ld):
        return L.gmt_mg_prolong_add(x0, nx, y0, ny, px, py, pe, cx0, cy0, lde, pu, ld, impl.stream)

    for enx, eny in ((0, 4), (5, 0), (0, 0)):
        assert pr(nx=enx, ny=eny) == 0
    codes += [pr(pe=None), pr(pu=None), pr(nx=-1), pr(ny=-1), pr(x0=0), pr(y0=0), pr(px=2), pr(px=-1), pr(py=2),
              pr(py=-1), pr(cx0=0), pr(cy0=0), pr(lde=cx0 + mx), pr(ld=x0 + nx - 1)]
    before = u.store.copy()
    d.fetch()
    assert same_bits(u.store, before)
    return [int(c) for c in codes]


N_REFUSALS = 10 + 14 + 14
N_SMOOTH = len(NXS) * (len(ALIGN) + len(ALIGN_F)) * 7 * len(OMEGAS)
N_RESTRICT = len(NXS) * len(ALIGN_R) * len(PARITIES) * len(TRANSFER_NYS)
N_PROLONG = len(NXS) * len(ALIGN_P) * len(PARITIES) * len(TRANSFER_NYS)


def host_impl(lib):
    from gpu_mpi_tests_amd import _native

    _native.bind(lib, [n for n in _native._SIGS if n.startswith("gmt_mg_")])
    return types.SimpleNamespace(lib=lib, stream=None, has_paths=False, upload=lambda a: a.copy(),
                                 download=lambda h: h.copy(), ptr=lambda h: h.ctypes.data)


def main():
    """Every check through the CPU backend; prints one JSON line."""
    impl = host_impl(ctypes.CDLL(sys.argv[1]))
    n = [0, 0, 0]
    for nx in NXS:
        for with_f in (False, True):
            n[0] += run_smooth_shapes(impl, nx, with_f)
        n[1] += run_restrict_shapes(impl, nx)
        n[2] += run_prolong_shapes(impl, nx)
    run_identities(impl)
    codes = run_empty_and_refusals(impl)
    u, o, _, region = smooth_fields(100, 100, "fast", False)
    d, s, rregion, coarse, _ = restrict_fields(100, 9, 1, 1, "fast")
    dev = cc.Dev(impl, d=d, s=s)
    paths = [list(smooth_path(impl, region, u, o)),
             int(impl.lib.gmt_mg_restrict_path(rregion[0], coarse[0], dev.ptr("d"), dev.ld("d"), dev.ptr("s"), dev.ld("s"))),
             int(impl.lib.gmt_mg_prolong_add_path(8, dev.ptr("s"), dev.ld("s"), dev.ptr("d"), dev.ld("d")))]
    print(json.dumps(dict(ok=True, cases=n, codes=codes, paths=paths)))


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
