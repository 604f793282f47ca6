"""Cases and NumPy fp64 model of the red-black smoother (gmt_mg_smooth_rb),
shared by tests/test_mg_rb_kernels_gpu.py (the gfx950 kernels) and
tests/test_mg_rb_kernels_cpu.py (the CPU backend: this file run as a program in
a child process, because build/lib-host/libgmt.so shares its SONAME with the
GPU library).  The conventions and helpers of tests/mg_fuse_cases.py: the C ABI
through the small `impl` of tests/cg_cases.py; everything outside the stated
read sets of u and f is NaN; everything outside out[R] is a sentinel that must
be bitwise intact afterwards; inputs must be bitwise unchanged; out[R] is
bitwise ops/reference.py's mg_smooth_rb (h applications of reference.mg_smooth
on the shrinking boxes, each merged through the colour mask); only the
all-aligned variant may take the fast path and the path of every case is
asserted where the backend has one.

Widths come from gmt_mg_smooth_k_geom(h) (the lane-pair tail, one and two
waves, one and two workgroups and the seams between them), heights from the
rows per segment L that the path query reports.  h = 1..4; every width x height
runs the masks 0, 15, 5 (W + S) and 10 (E + N), with and without f, on every
alignment variant: both par and omega 1.0 and 0.8 on the all-aligned one, par
and omega in turn on the variants that take the one-lane-per-cell kernel; all
16 masks at three shapes."""
import ctypes
import json
import sys

import numpy as np

import cg_cases as cc
import mg_cases as mc
import mg_fuse_cases as fc

HS = (1, 2, 3, 4)
C0, C1 = fc.C0, fc.C1
SENTINEL = fc.SENTINEL
OMEGAS = (1.0, 0.8)
MASKS = fc.MASKS
ALIGN, ALIGN_F = fc.ALIGN, fc.ALIGN_F
HOST_SEG = fc.HOST_SEG
PATH_NONE, PATH_SCALAR, PATH_ROW_WALK = fc.PATH_NONE, fc.PATH_SCALAR, fc.PATH_ROW_WALK
same_bits = fc.same_bits
fields = fc.fields    # gmt_mg_smooth_k's read sets with h for k
geom = fc.geom
widths = fc.widths
heights = fc.heights
host_impl = fc.host_impl


def ref():
    from gpu_mpi_tests_amd.ops import reference

    return reference


def reference(h, par, region, mask, u, f, om):
    x0, nx, y0, ny = region
    out = np.full(u.a.shape, SENTINEL)
    ref().mg_smooth_rb(u.a, out, om, x0, nx, y0, ny, h, par, mask, None if f is None else f.a, C0, C1)
    want = out[y0:y0 + ny, x0:x0 + nx].copy()
    out[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (out == SENTINEL).all()  # the model writes the region only
    return want


def due(region, par, j=1):
    """The cells of the region that half-sweep j (1-based) of a call with `par` updates."""
    _, nx, _, ny = region
    return (np.arange(nx)[None, :] + np.arange(ny)[:, None] + par + (j - 1)) % 2 == 0


def path(impl, h, par, region, mask, u, o, f=None):
    d = cc.Dev(impl, u=u, o=o, f=f)
    seg = ctypes.c_int64(-1)
    p = impl.lib.gmt_mg_smooth_rb_path(h, par, region[0], region[1], region[3], mask, d.ptr("u"), d.ld("u"),
                                       d.ptr("f"), d.ld("f"), d.ptr("o"), d.ld("o"),
                                       ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(p), int(seg.value)


def seg_rows(impl, h, nx):
    """Rows per segment of the walk for this width (HOST_SEG on a backend without kernels)."""
    if not impl.has_paths:
        return HOST_SEG
    u, o, _, region = fields(h, nx, 1, 0, "fast", False)
    p, seg = path(impl, h, 0, region, 0, u, o)
    assert p == PATH_ROW_WALK and seg >= 2 * h, (p, seg)
    return seg


def call(impl, h, par, region, mask, u, o, f, om, c0=C0, c1=C1):
    x0, nx, y0, ny = region
    d = cc.Dev(impl, u=u, o=o, f=f)
    code = impl.lib.gmt_mg_smooth_rb(h, par, x0, nx, y0, ny, mask, d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"), c0, c1,
                                     om, d.ptr("o"), d.ld("o"), impl.stream)
    d.fetch()
    return int(code)


def check(impl, h, par, nx, ny, mask, align, with_f, om, seg=None):
    what = ("mg_smooth_rb", h, par, nx, ny, mask, align, with_f, om)
    u, o, f, region = fields(h, nx, ny, mask, align, with_f)
    x0, _, y0, _ = region
    if impl.has_paths:
        p, s = path(impl, h, par, region, mask, u, o, f)
        fast = align == "fast"
        assert p == (PATH_ROW_WALK if fast else PATH_SCALAR), (what, p)
        assert s == (seg if fast else 0), (what, s, seg)
    ubefore = u.store.copy()
    fbefore = None if f is None else f.store.copy()
    want = reference(h, par, region, mask, u, f, om)
    assert not np.isnan(want).any(), what                          # the model stays inside the read sets
    assert call(impl, h, par, region, mask, u, o, f, om) == 0, what
    assert same_bits(ubefore, u.store), what                       # u is never written
    assert f is None or same_bits(fbefore, f.store), what
    O = o.a
    got = O[y0:y0 + ny, x0:x0 + nx]
    if not same_bits(got, want):
        bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
        raise AssertionError((what, "cells (row, column) that differ", len(bad), bad[:8].tolist()))
    O[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (o.store == SENTINEL).all(), what                       # nothing outside the region is written


def run_fast_shapes(impl, h, nx):
    """Every height, mask, f and alignment variant at one width: both par with omega 1.0 and 0.8 in turn on the
    all-aligned variant (every par sees both omegas over the heights), par and omega in turn on the others."""
    L = seg_rows(impl, h, nx)
    n = 0
    for ny in heights(h, L):
        for mask in MASKS:
            for with_f in (False, True):
                for par in (0, 1):
                    for om in OMEGAS:
                        check(impl, h, par, nx, ny, mask, "fast", with_f, om, L)
                        n += 1
                for i, align in enumerate(ALIGN_F if with_f else ALIGN):
                    if align != "fast":
                        check(impl, h, (i + ny) % 2, nx, ny, mask, align, with_f, OMEGAS[(i + ny + mask) % 2])
                        n += 1
    return n


def scalar_shapes(impl, h):
    w, _ = geom(impl, h)
    return ((1, 1), (2, h), (3, h + 1), (w + 1, 2), (5, HOST_SEG + 1))


def run_scalar_shapes(impl, h):
    """The alignment variants that must take the one-lane-per-cell kernel."""
    n = 0
    for with_f in (False, True):
        for a, align in enumerate(ALIGN_F if with_f else ALIGN):
            if align == "fast":
                continue
            for i, (nx, ny) in enumerate(scalar_shapes(impl, h)):
                for mask in MASKS:
                    check(impl, h, (a + i + mask) % 2, nx, ny, mask, align, with_f, OMEGAS[(i + mask) % 2])
                    n += 1
    return n


def all_mask_shapes(impl, h):
    """The smallest region, one wave seam and one segment seam."""
    w, _ = geom(impl, h)
    return ((1, 1), (w + 1, h + 1), (3, seg_rows(impl, h, 3) + 1))


def run_all_masks(impl, h):
    n = 0
    for nx, ny in all_mask_shapes(impl, h):
        L = seg_rows(impl, h, nx)
        for mask in range(16):
            for with_f in (False, True):
                check(impl, h, mask % 2, nx, ny, mask, "fast", with_f, 1.0, L)
                check(impl, h, (mask + 1) % 2, nx, ny, mask, "odd_x0", with_f, 0.8)
                n += 2
    return n


def n_fast(h, L=HOST_SEG):
    return len(heights(h, L)) * len(MASKS) * (2 * 2 * len(OMEGAS) + len(ALIGN) - 1 + len(ALIGN_F) - 1)


def n_scalar():
    return (len(ALIGN) - 1 + len(ALIGN_F) - 1) * 5 * len(MASKS)


N_ALL_MASKS = 3 * 16 * 2 * 2


# ---------------------------------------------------------------- identities
def _chain(impl, hs, pars, nx, ny, align, with_f, om, tag):
    """Calls with hs[i] half-sweeps and pars[i], mask 0, one after another between two buffers that hold the
    same ring; returns the region after the last one."""
    a, _, f, region = fields(tag, nx, ny, 0, align, with_f)
    x0, _, y0, _ = region
    b = cc.Field(a.rows, x0 + nx + 5, False, 0, np.nan)
    b.a[...] = a.a  # the same ring in either buffer
    for h, par in zip(hs, pars):
        assert call(impl, h, par, region, 0, a, b, f, om) == 0, (hs, pars)
        a, b = b, a
    return a.a[y0:y0 + ny, x0:x0 + nx].copy()


def run_identities(impl):
    """1. h = 2 with par p, mask 0, is h = 1 with p then h = 1 with p ^ 1 through a second buffer with the same
    ring.  2. h = 4 is two h = 2 calls.  3. the due cells of an h = 1 call with par 0 and of one with par 1 are
    together gmt_mg_smooth(u).  4. an h = 1 call leaves every cell that is not due bitwise u.  5. omega = 0 is the
    identity.  6. a constant field with a constant ring is a fixed point.  All bitwise."""
    w, _ = geom(impl, 4)
    shapes = ((w + 3, 9), (7, HOST_SEG + 2))
    for align in ("fast", "odd_x0"):
        for with_f in (False, True):
            for nx, ny in shapes:
                for om in OMEGAS:
                    for p in (0, 1):
                        # fields(k = 4, mask 0) for every chain: the same u whatever h
                        two = _chain(impl, (2,), (p,), nx, ny, align, with_f, om, 4)
                        ones = _chain(impl, (1, 1), (p, p ^ 1), nx, ny, align, with_f, om, 4)
                        assert same_bits(two, ones), (1, align, with_f, nx, ny, om, p)
                        four = _chain(impl, (4,), (p,), nx, ny, align, with_f, om, 4)
                        twos = _chain(impl, (2, 2), (p, p), nx, ny, align, with_f, om, 4)
                        assert same_bits(four, twos), (2, align, with_f, nx, ny, om, p)
                # 3 and 4: one u, h = 1 with either par, and the Jacobi sweep
                u, o, f, region = fields(4, nx, ny, 0, align, with_f)
                x0, _, y0, _ = region
                R = (slice(y0, y0 + ny), slice(x0, x0 + nx))
                got = []
                for p in (0, 1):
                    o.a[...] = SENTINEL
                    assert call(impl, 1, p, region, 0, u, o, f, 0.8) == 0
                    got.append(o.a[R].copy())
                    keep = ~due(region, p)
                    assert same_bits(got[p][keep], u.a[R][keep]), (4, align, with_f, nx, ny, p)
                o.a[...] = SENTINEL
                d = cc.Dev(impl, u=u, o=o, f=f)
                assert impl.lib.gmt_mg_smooth(x0, nx, y0, ny, d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"), C0, C1, 0.8,
                                              d.ptr("o"), d.ld("o"), impl.stream) == 0
                d.fetch()
                jac = o.a[R].copy()
                merged = np.where(due(region, 0), got[0], got[1])
                assert same_bits(merged, jac), (3, align, with_f, nx, ny)
            for h in HS:
                wh, _ = geom(impl, h)
                for mask in (0, 15, 6):
                    for par in (0, 1):
                        u, o, f, region = fields(h, wh + 1, h + 2, mask, align, with_f)
                        x0, nx, y0, ny = region
                        assert call(impl, h, par, region, mask, u, o, f, 0.0) == 0
                        assert same_bits(o.a[y0:y0 + ny, x0:x0 + nx], u.a[y0:y0 + ny, x0:x0 + nx]), (5, h, align, mask)
        for h in HS:
            wh, _ = geom(impl, h)
            for mask in (0, 15, 9):
                for const in (1.0, -0.3):
                    for par, om in ((0, 1.0), (1, 0.8)):
                        u, o, _, region = fields(h, wh + 1, h + 2, mask, align, False, const=const)
                        x0, nx, y0, ny = region
                        assert call(impl, h, par, region, mask, u, o, None, om) == 0
                        assert same_bits(o.a[y0:y0 + ny, x0:x0 + nx], np.full((ny, nx), const)), (6, h, align, mask)


# --------------------------------------------------------- empty and refused
def run_empty_and_refusals(impl):
    """gmt_mg_smooth_k's empty regions and refusals with h for k, and par outside 0..1; out stays intact."""
    L = impl.lib
    h = 3
    u, o, f, (x0, nx, y0, ny) = fields(h, 5, 4, 15, "fast", True)
    d = cc.Dev(impl, u=u, o=o, f=f)

    def sm(h=h, par=1, x0=x0, nx=nx, y0=y0, ny=ny, mask=15, pu=d.ptr("u"), ld=u.ld, pf=d.ptr("f"), ldf=f.ld,
           po=d.ptr("o"), ldo=o.ld):
        return L.gmt_mg_smooth_rb(h, par, x0, nx, y0, ny, mask, pu, ld, pf, ldf, C0, C1, 1.0, po, ldo, impl.stream)

    for enx, eny in ((0, 4), (5, 0), (0, 0)):
        assert sm(nx=enx, ny=eny) == 0
    codes = [sm(pu=None), sm(po=None), sm(nx=-1), sm(ny=-1), sm(nx=-1, ny=0),     # gmt_mg_smooth's
             sm(mask=0, x0=0), sm(mask=0, y0=0), sm(mask=0, ld=x0 + nx), sm(ldo=x0 + nx - 1),
             sm(mask=0, ldf=x0 + nx - 1),
             sm(h=0), sm(h=5), sm(h=-1), sm(mask=-1), sm(mask=16),               # h and the mask
             sm(mask=1, x0=h - 1), sm(mask=4, y0=h - 1),                          # the read set's room
             sm(mask=2, ld=x0 + nx + h - 1), sm(mask=2, ldf=x0 + nx + h - 2),     # its pitches
             sm(po=d.ptr("u")), sm(po=d.ptr("u") + 8 * u.ld * 2),                 # u and out overlapping
             sm(par=-1), sm(par=2)]                                               # the colour phase
    before = o.store.copy()
    d.fetch()
    assert same_bits(o.store, before)
    assert sm(pf=None, ldf=0) == 0 and sm(par=0) == 0                             # f is optional
    assert sm(mask=1, x0=h + 1) == 0 and sm(mask=0, x0=1, y0=1) == 0              # the least room that is enough
    return [int(c) for c in codes]


N_REFUSALS = 23


def main():
    """Every check through the CPU backend; prints one JSON line."""
    impl = host_impl(ctypes.CDLL(sys.argv[1]))
    n = [0, 0, 0]
    for h in HS:
        for nx in widths(impl, h):
            n[0] += run_fast_shapes(impl, h, nx)
        n[1] += run_scalar_shapes(impl, h)
        n[2] += run_all_masks(impl, h)
    run_identities(impl)
    codes = run_empty_and_refusals(impl)
    u, o, _, region = fields(2, 100, 40, 0, "fast", False)
    print(json.dumps(dict(ok=True, cases=n, codes=codes, path=list(path(impl, 2, 0, region, 0, u, o)),
                          geom=[list(geom(impl, h)) for h in HS])))


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
