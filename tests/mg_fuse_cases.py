"""Cases and NumPy fp64 model of the fused multigrid smoother (gmt_mg_smooth_k),
shared by tests/test_mg_fuse_kernels_gpu.py (the gfx950 kernels) and
tests/test_mg_fuse_kernels_cpu.py (the CPU backend: this file run as a program
in a child process, because build/lib-host/libgmt.so shares its SONAME with the
GPU library).  The conventions of tests/mg_cases.py: the C ABI through the
small `impl` of tests/cg_cases.py; everything outside the stated read sets of u
and f is NaN; everything outside out[R] is a sentinel that must be bitwise
intact afterwards; inputs must be bitwise unchanged; out[R] is bitwise
ops/reference.py's mg_smooth_k (k applications of reference.mg_smooth on the
shrinking boxes); only the all-aligned variant may take the fast path and the
path of every case is asserted where the backend has one.

Widths come from gmt_mg_smooth_k_geom (the lane-pair tail, one and two waves,
one and two workgroups and the seams between them, where neighbouring waves
overlap), heights from the rows per segment L that the path query reports (a
region shorter than the warm-up, and the segment seams).  Every width x height
runs the masks 0, 15, 5 (W + S) and 10 (E + N), with and without f, on every
alignment variant: omega 0.8 and 1.0 on the all-aligned one, the two in turn on
the variants that take the one-lane-per-cell kernel; all 16 masks at three
shapes."""
import ctypes
import json
import sys
import types

import numpy as np

import cg_cases as cc
import mg_cases as mc

KS = (2, 3, 4)
C0, C1 = mc.C0, mc.C1
SENTINEL = cc.SENTINEL
OMEGAS = (0.8, 1.0)
MASKS = (0, 15, 5, 10)
ALIGN, ALIGN_F = mc.ALIGN, mc.ALIGN_F
HOST_SEG = 32  # a segment length of the fused walk: the heights of a backend without kernels
Y0 = 5         # room for 4 halo rows and one NaN row below them
PATH_NONE, PATH_SCALAR, PATH_ROW_WALK = cc.PATH_NONE, cc.PATH_SCALAR, cc.PATH_ROW_WALK
same_bits = cc.same_bits


def ref():
    from gpu_mpi_tests_amd.ops import reference

    return reference


def geom(impl, k):
    wc, bc = ctypes.c_int64(0), ctypes.c_int64(0)
    code = impl.lib.gmt_mg_smooth_k_geom(k, ctypes.cast(ctypes.pointer(wc), ctypes.c_void_p),
                                         ctypes.cast(ctypes.pointer(bc), ctypes.c_void_p))
    assert code == 0, code
    return int(wc.value), int(bc.value)


def widths(impl, k):
    w, b = geom(impl, k)
    return (1, 2, 3, w - 1, w, w + 1, w + 2, b - 1, b, b + 1, 2 * b + 1)


def heights(k, L):
    return tuple(sorted({1, 2, k, k + 1, L - 1, L, L + 1, 2 * L + 1}))


def grow(k, mask):
    """(west, east, south, north) cells of u's read set beyond the region."""
    return tuple(k if mask & bit else 1 for bit in (1, 2, 4, 8))


def fields(k, nx, ny, mask, align, with_f, const=None):
    x0, odd, base = (ALIGN_F if with_f else ALIGN)[align]
    y0 = Y0
    gw, ge, gs, gn = grow(k, mask)
    rows = y0 + ny + 5
    g = cc._rng("mg_smooth_k", k, nx, ny, mask)
    u = cc.Field(rows, x0 + nx + 5, "u" in odd, "u" in base, np.nan)
    box = (slice(y0 - gs, y0 + ny + gn), slice(x0 - gw, x0 + nx + ge))
    u.a[box] = g.random((ny + gs + gn, nx + gw + ge)) - 0.5 if const is None else const
    o = cc.Field(rows, x0 + nx + 1, "o" in odd, "o" in base, SENTINEL)
    f = None
    if with_f:
        f = cc.Field(rows, x0 + nx + 4, "f" in odd, 0, np.nan)
        fbox = (slice(y0 - (gs - 1), y0 + ny + gn - 1), slice(x0 - (gw - 1), x0 + nx + ge - 1))
        f.a[fbox] = g.random((ny + gs + gn - 2, nx + gw + ge - 2)) - 0.5
    return u, o, f, (x0, nx, y0, ny)


def reference(k, region, mask, u, f, om):
    x0, nx, y0, ny = region
    out = np.full(u.a.shape, SENTINEL)
    ref().mg_smooth_k(u.a, out, om, x0, nx, y0, ny, k, mask, None if f is None else f.a, C0, C1)
    want = out[y0:y0 + ny, x0:x0 + nx].copy()
    out[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (out == SENTINEL).all()  # the model writes the region only
    return want


def path(impl, k, region, mask, u, o, f=None):
    d = cc.Dev(impl, u=u, o=o, f=f)
    seg = ctypes.c_int64(-1)
    p = impl.lib.gmt_mg_smooth_k_path(k, region[0], region[1], region[3], mask, d.ptr("u"), d.ld("u"), d.ptr("f"),
                                      d.ld("f"), d.ptr("o"), d.ld("o"), ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(p), int(seg.value)


def seg_rows(impl, k, nx):
    """Rows per segment of the fused walk for this width (HOST_SEG on a backend without kernels)."""
    if not impl.has_paths:
        return HOST_SEG
    u, o, _, region = fields(k, nx, 1, 0, "fast", False)
    p, seg = path(impl, k, region, 0, u, o)
    assert p == PATH_ROW_WALK and seg >= 2 * k, (p, seg)
    return seg


def call(impl, k, region, mask, u, o, f, om, c0=C0, c1=C1):
    x0, nx, y0, ny = region
    d = cc.Dev(impl, u=u, o=o, f=f)
    code = impl.lib.gmt_mg_smooth_k(k, x0, nx, y0, ny, mask, d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"), c0, c1, om,
                                    d.ptr("o"), d.ld("o"), impl.stream)
    d.fetch()
    return int(code)


def check(impl, k, nx, ny, mask, align, with_f, om, seg=None):
    what = ("mg_smooth_k", k, nx, ny, mask, align, with_f, om)
    u, o, f, region = fields(k, nx, ny, mask, align, with_f)
    x0, _, y0, _ = region
    if impl.has_paths:
        p, s = path(impl, k, region, mask, u, o, f)
        fast = align == "fast"
        assert p == (PATH_ROW_WALK if fast else PATH_SCALAR), (what, p)
        assert s == (seg if fast else 0), (what, s, seg)
    ubefore = u.store.copy()
    fbefore = None if f is None else f.store.copy()
    want = reference(k, region, mask, u, f, om)
    assert not np.isnan(want).any(), what                          # the model stays inside the read sets
    assert call(impl, k, region, mask, u, o, f, om) == 0, what
    assert same_bits(ubefore, u.store), what                       # u is never written
    assert f is None or same_bits(fbefore, f.store), what
    O = o.a
    got = O[y0:y0 + ny, x0:x0 + nx]
    if not same_bits(got, want):
        bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
        raise AssertionError((what, "cells (row, column) that differ", len(bad), bad[:8].tolist()))
    O[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (o.store == SENTINEL).all(), what                       # nothing outside the region is written


def run_fast_shapes(impl, k, nx):
    """Every height, mask, f and alignment variant at one width: both omegas on the all-aligned variant, the two
    in turn on the others (each of them sees both)."""
    L = seg_rows(impl, k, nx)
    n = 0
    for ny in heights(k, L):
        for mask in MASKS:
            for with_f in (False, True):
                for om in OMEGAS:
                    check(impl, k, nx, ny, mask, "fast", with_f, om, L)
                    n += 1
                for i, align in enumerate(ALIGN_F if with_f else ALIGN):
                    if align != "fast":
                        check(impl, k, nx, ny, mask, align, with_f, OMEGAS[(i + ny + mask) % 2])
                        n += 1
    return n


def scalar_shapes(impl, k):
    w, _ = geom(impl, k)
    return ((1, 1), (2, k), (3, k + 1), (w + 1, 2), (5, HOST_SEG + 1))


def run_scalar_shapes(impl, k):
    """The alignment variants that must take the one-lane-per-cell kernel."""
    n = 0
    for with_f in (False, True):
        for align in (ALIGN_F if with_f else ALIGN):
            if align == "fast":
                continue
            for i, (nx, ny) in enumerate(scalar_shapes(impl, k)):
                for mask in MASKS:
                    check(impl, k, nx, ny, mask, align, with_f, OMEGAS[(i + mask) % 2])
                    n += 1
    return n


def all_mask_shapes(impl, k):
    """The smallest region, one wave seam and one segment seam."""
    w, _ = geom(impl, k)
    return ((1, 1), (w + 1, k + 1), (3, seg_rows(impl, k, 3) + 1))


def run_all_masks(impl, k):
    n = 0
    for nx, ny in all_mask_shapes(impl, k):
        L = seg_rows(impl, k, nx)
        for mask in range(16):
            for with_f in (False, True):
                check(impl, k, nx, ny, mask, "fast", with_f, 0.8, L)
                check(impl, k, nx, ny, mask, "odd_x0", with_f, 0.8)
                n += 2
    return n


def n_fast(k, L=HOST_SEG):
    return len(heights(k, L)) * len(MASKS) * (2 * len(OMEGAS) + len(ALIGN) - 1 + len(ALIGN_F) - 1)


def n_scalar():
    return (len(ALIGN) - 1 + len(ALIGN_F) - 1) * 5 * len(MASKS)


N_ALL_MASKS = 3 * 16 * 2 * 2


# ---------------------------------------------------------------- identities
def run_identities(impl):
    """k single sweeps on a single-rank layout (mask 0: the ring fixed in both buffers) give the bits of one
    fused call; omega = 0 is the identity; a constant field with a constant ring is a fixed point."""
    for k in KS:
        w, _ = geom(impl, k)
        for align in ("fast", "odd_x0"):
            for with_f in (False, True):
                for nx, ny in ((w + 3, 2 * k + 1), (7, HOST_SEG + 2)):
                    u, o, f, region = fields(k, nx, ny, 0, align, with_f)
                    x0, _, y0, _ = region
                    assert call(impl, k, region, 0, u, o, f, 0.8) == 0
                    fused = o.a[y0:y0 + ny, x0:x0 + nx].copy()
                    a, _, _, _ = fields(k, nx, ny, 0, align, with_f)
                    b = cc.Field(a.rows, x0 + nx + 5, False, 0, np.nan)
                    b.a[...] = a.a  # the same ring in either buffer
                    for _ in range(k):
                        d = cc.Dev(impl, u=a, o=b, f=f)
                        code = impl.lib.gmt_mg_smooth(x0, nx, y0, ny, d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"), C0,
                                                      C1, 0.8, d.ptr("o"), d.ld("o"), impl.stream)
                        assert code == 0, code
                        d.fetch()
                        a, b = b, a
                    assert same_bits(a.a[y0:y0 + ny, x0:x0 + nx], fused), (k, align, with_f, nx, ny)
                for mask in (0, 15, 6):
                    u, o, f, region = fields(k, w + 1, k + 2, mask, align, with_f)
                    x0, nx, y0, ny = region
                    assert call(impl, k, region, mask, u, o, f, 0.0) == 0
                    assert same_bits(o.a[y0:y0 + ny, x0:x0 + nx], u.a[y0:y0 + ny, x0:x0 + nx]), (k, align, mask)
            for mask in (0, 15, 9):
                for const in (1.0, -0.3):
                    u, o, _, region = fields(k, w + 1, k + 2, mask, align, False, const=const)
                    x0, nx, y0, ny = region
                    assert call(impl, k, region, mask, u, o, None, 0.8) == 0
                    assert same_bits(o.a[y0:y0 + ny, x0:x0 + nx], np.full((ny, nx), const)), (k, align, mask)


# --------------------------------------------------------- empty and refused
def run_empty_and_refusals(impl):
    """An empty region launches nothing and returns 0; the refused calls, with their codes; out stays intact."""
    L = impl.lib
    k = 3
    u, o, f, (x0, nx, y0, ny) = fields(k, 5, 4, 15, "fast", True)
    d = cc.Dev(impl, u=u, o=o, f=f)

    def sm(k=k, x0=x0, nx=nx, y0=y0, ny=ny, mask=15, pu=d.ptr("u"), ld=u.ld, pf=d.ptr("f"), ldf=f.ld, po=d.ptr("o"),
           ldo=o.ld):
        return L.gmt_mg_smooth_k(k, x0, nx, y0, ny, mask, pu, ld, pf, ldf, C0, C1, 0.8, po, ldo, impl.stream)

    for enx, eny in ((0, 4), (5, 0), (0, 0)):
        assert sm(nx=enx, ny=eny) == 0
    codes = [sm(pu=None), sm(po=None), sm(nx=-1), sm(ny=-1), sm(nx=-1, ny=0),     # gmt_mg_smooth's
             sm(mask=0, x0=0), sm(mask=0, y0=0), sm(mask=0, ld=x0 + nx), sm(ldo=x0 + nx - 1),
             sm(mask=0, ldf=x0 + nx - 1),
             sm(k=0), sm(k=5), sm(k=-1), sm(mask=-1), sm(mask=16),               # k and the mask
             sm(mask=1, x0=k - 1), sm(mask=4, y0=k - 1),                          # the read set's room
             sm(mask=2, ld=x0 + nx + k - 1), sm(mask=2, ldf=x0 + nx + k - 2),     # its pitches
             sm(po=d.ptr("u")), sm(po=d.ptr("u") + 8 * u.ld * 2)]                 # u and out overlapping
    before = o.store.copy()
    d.fetch()
    assert same_bits(o.store, before)
    assert sm(pf=None, ldf=0) == 0                                                # f is optional
    assert sm(mask=1, x0=k + 1) == 0 and sm(mask=0, x0=1, y0=1) == 0              # the least room that is enough
    return [int(c) for c in codes]


N_REFUSALS = 21


def host_impl(lib):
    from gpu_mpi_tests_amd import _native

    _native.bind(lib, [n for n in _native._SIGS if n.startswith("gmt_mg_")])
    return types.SimpleNamespace(lib=lib, stream=None, has_paths=False, upload=lambda a: a.copy(),
                                 download=lambda h: h.copy(), ptr=lambda h: h.ctypes.data)


def main():
    """Every check through the CPU backend; prints one JSON line."""
    impl = host_impl(ctypes.CDLL(sys.argv[1]))
    n = [0, 0, 0]
    for k in KS:
        for nx in widths(impl, k):
            n[0] += run_fast_shapes(impl, k, nx)
        n[1] += run_scalar_shapes(impl, k)
        n[2] += run_all_masks(impl, k)
    run_identities(impl)
    codes = run_empty_and_refusals(impl)
    u, o, _, region = fields(2, 100, 40, 0, "fast", False)
    print(json.dumps(dict(ok=True, cases=n, codes=codes, path=list(path(impl, 2, region, 0, u, o)),
                          geom=[list(geom(impl, k)) for k in KS])))


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
