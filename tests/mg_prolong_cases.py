"""Cases and NumPy fp64 model of the interpolation fused into the first
post-smoothing pass (gmt_mg_prolong_smooth), shared by
tests/test_mg_prolong_kernels_gpu.py (the gfx950 kernels) and
tests/test_mg_prolong_kernels_cpu.py (the CPU backend: this file run as a
program in a child process, because build/lib-host/libgmt.so shares its SONAME
with the GPU library).  The conventions of tests/mg_resid_cases.py: the C ABI
through the small `impl` of tests/cg_cases.py; everything outside the read sets
is NaN (u and f: gmt_mg_smooth_k(h)'s; e: exactly the coarse cells that
gmt_mg_prolong_add's rule names for the cells of B0, the region grown by h on
the sides whose bit is set); out is a sentinel outside the region that must be
bitwise intact afterwards; u, e and f must be bitwise unchanged; out[R] is
bitwise ops/reference.py's mg_prolong_smooth (mg_prolong_add over B0 on a copy,
then mg_smooth_k or mg_smooth_rb); only the all-aligned variant may take the
walk and the path of every case is asserted where the backend has one.

h = 1..4, Jacobi and red-black with either colour phase (MODES), all four
(px, py), without and with f.  Widths come from gmt_mg_prolong_smooth_geom(h)
(the lane-pair tail, the seams between waves and workgroups), heights from the
rows per segment L that the path query reports (regions shorter than the
warm-up, and the segment seams)."""
import ctypes
import json
import sys

import numpy as np

import cg_cases as cc
import mg_cases as mc
import mg_fuse_cases as fc

HS = (1, 2, 3, 4)
MODES = ((0, 0), (1, 0), (1, 1))  # (rb, par)
C0, C1 = fc.C0, fc.C1
SENTINEL = fc.SENTINEL
OMEGAS = (0.8, 1.0)
MASKS = fc.MASKS
PARITIES = mc.PARITIES
ALIGN, ALIGN_F = fc.ALIGN, fc.ALIGN_F
HOST_SEG = fc.HOST_SEG
CX0, CY0 = 4, 4  # room for h/2 + 1 = 3 coarse halo cells and one NaN cell before them
PATH_NONE, PATH_SCALAR, PATH_ROW_WALK = fc.PATH_NONE, fc.PATH_SCALAR, fc.PATH_ROW_WALK
same_bits = fc.same_bits
host_impl = fc.host_impl
heights = fc.heights


def ref():
    from gpu_mpi_tests_amd.ops import reference

    return reference


def geom(impl, h):
    wc, bc = ctypes.c_int64(0), ctypes.c_int64(0)
    code = impl.lib.gmt_mg_prolong_smooth_geom(h, ctypes.cast(ctypes.pointer(wc), ctypes.c_void_p),
                                               ctypes.cast(ctypes.pointer(bc), ctypes.c_void_p))
    assert code == 0, code
    assert (int(wc.value), int(bc.value)) == fc.geom(impl, h)  # gmt_mg_smooth_k_geom(h)
    return int(wc.value), int(bc.value)


def widths(impl, h):
    w, b = geom(impl, h)
    return (1, 2, 3, w - 1, w, w + 1, w + 2, b - 1, b, b + 1, 2 * b + 1)


def coarse_taps(n, p, g0, g1):
    """The first and last coarse index that the rule reads for the fine cells -g0 .. n + g1 - 1 of one axis."""
    idx = set()
    for i in range(-g0, n + g1):
        d = i - p
        idx.add(d // 2)          # floor: the coarse cell the fine cell sits on, or the one before it
        if d % 2:
            idx.add(d // 2 + 1)
    return min(idx), max(idx)


def fields(h, nx, ny, mask, par, align, with_f, e_odd=False, e_base=0):
    """u, out and f of tests/mg_fuse_cases.py for h, and e with exactly the cells that B0 needs."""
    u, o, f, region = fc.fields(h, nx, ny, mask, align, with_f)
    px, py = par
    mx, my = mc.coarse_extent(nx, px), mc.coarse_extent(ny, py)
    gw, ge, gs, gn = (h if mask & bit else 0 for bit in (1, 2, 4, 8))
    i0, i1 = coarse_taps(nx, px, gw, ge)
    j0, j1 = coarse_taps(ny, py, gs, gn)
    d = h // 2 + 1  # what the call may ask for: never less than what the rule reads
    for lo, hi, m, a, b in ((i0, i1, mx, gw, ge), (j0, j1, my, gs, gn)):
        assert -(d if a else 1) <= lo and hi <= m - 1 + (d if b else 1), (h, nx, ny, mask, par)
    e = cc.Field(CY0 + my + 4, CX0 + mx + 4, e_odd, e_base, np.nan)
    g = cc._rng("mg_prolong_smooth", h, nx, ny, mask, par)
    e.a[CY0 + j0:CY0 + j1 + 1, CX0 + i0:CX0 + i1 + 1] = g.random((j1 - j0 + 1, i1 - i0 + 1)) - 0.5
    return e, u, o, f, region


def reference(h, mode, region, par, mask, e, u, f, om):
    x0, nx, y0, ny = region
    out = np.full(u.a.shape, SENTINEL)
    ref().mg_prolong_smooth(e.a, u.a, out, om, x0, nx, y0, ny, par[0], par[1], CX0, CY0, h, mode[0], mode[1], mask,
                            None if f is None else f.a, C0, C1)
    want = out[y0:y0 + ny, x0:x0 + nx].copy()
    out[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (out == SENTINEL).all()  # the model writes the region only
    return want


def path(impl, h, mode, region, par, mask, e, u, o, f=None):
    d = cc.Dev(impl, e=e, u=u, o=o, f=f)
    seg = ctypes.c_int64(-1)
    x0, nx, y0, ny = region
    p = impl.lib.gmt_mg_prolong_smooth_path(h, mode[0], mode[1], x0, nx, y0, ny, par[0], par[1], mask, d.ptr("e"), CX0,
                                            CY0, d.ld("e"), d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"), d.ptr("o"),
                                            d.ld("o"), ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(p), int(seg.value)


def seg_rows(impl, h, nx):
    """Rows per segment of the walk for this width (HOST_SEG on a backend without kernels)."""
    if not impl.has_paths:
        return HOST_SEG
    e, u, o, _, region = fields(h, nx, 1, 0, (0, 0), "fast", False)
    p, seg = path(impl, h, (0, 0), region, (0, 0), 0, e, u, o)
    assert p == PATH_ROW_WALK and seg >= 2 * h, (p, seg)
    return seg


def call(impl, h, mode, region, par, mask, e, u, o, f, om, c0=C0, c1=C1):
    x0, nx, y0, ny = region
    d = cc.Dev(impl, e=e, u=u, o=o, f=f)
    code = impl.lib.gmt_mg_prolong_smooth(h, mode[0], mode[1], x0, nx, y0, ny, par[0], par[1], mask, d.ptr("e"), CX0,
                                          CY0, d.ld("e"), d.ptr("u"), d.ld("u"), d.ptr("f"), d.ld("f"), c0, c1, om,
                                          d.ptr("o"), d.ld("o"), impl.stream)
    d.fetch()
    return int(code)


def check(impl, h, mode, nx, ny, mask, par, align, with_f, om, seg=None, e_odd=False, e_base=0, prep=None):
    what = ("mg_prolong_smooth", h, mode, nx, ny, mask, par, align, with_f, om, e_odd, e_base)
    e, u, o, f, region = fields(h, nx, ny, mask, par, align, with_f, e_odd, e_base)
    if prep:
        prep(e, u, region)
    x0, _, y0, _ = region
    if impl.has_paths:
        p, s = path(impl, h, mode, region, par, mask, e, u, o, f)
        fast = align == "fast"  # e is read 8 B per lane: its alignment never counts
        assert p == (PATH_ROW_WALK if fast else PATH_SCALAR), (what, p)
        assert s == (seg if fast else 0), (what, s, seg)
    before = [None if t is None else t.store.copy() for t in (e, u, f)]
    want = reference(h, mode, region, par, mask, e, u, f, om)
    assert not np.isnan(want).any(), what                          # the model stays inside the read sets
    assert call(impl, h, mode, region, par, mask, e, u, o, f, om) == 0, what
    for t, b in zip((e, u, f), before):
        assert t is None or same_bits(b, t.store), what            # e, u and f are never written
    O = o.a
    got = O[y0:y0 + ny, x0:x0 + nx]
    if not same_bits(got, want):
        bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
        raise AssertionError((what, "cells (row, column) that differ", len(bad), bad[:8].tolist()))
    O[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (o.store == SENTINEL).all(), what                       # nothing outside the region is written


# ------------------------------------------------------------------ the cases
ALL_MASKS_SHAPE = (130, 21)  # two waves at every h, and more than one segment


def run_all_masks(impl, h):
    """All 16 masks x every mode x every parity x with and without f at one small shape on the walk, and every
    mask on the one-lane-per-cell kernel with the other parameters in turn."""
    nx, ny = ALL_MASKS_SHAPE
    L = seg_rows(impl, h, nx)
    n = 0
    for mask in range(16):
        for par in PARITIES:
            for with_f in (False, True):
                for m, mode in enumerate(MODES):
                    check(impl, h, mode, nx, ny, mask, par, "fast", with_f, OMEGAS[(m + mask) % 2], L)
                    n += 1
        for i, par in enumerate(PARITIES):
            check(impl, h, MODES[(mask + i) % 3], nx // 2, ny, mask, par, "odd_x0", bool((mask + i) % 2), 0.8)
            n += 1
    return n


N_ALL_MASKS = 16 * (4 * 2 * 3 + 4)


def _sweep(impl, h, nx, ny, L, k):
    """The four masks and parities on the walk; mode, f and omega in turn (k shifts the turn)."""
    n = 0
    for a, mask in enumerate(MASKS):
        for b, par in enumerate(PARITIES):
            t = a + b + k
            check(impl, h, MODES[t % 3], nx, ny, mask, par, "fast", bool((t // 3) % 2), OMEGAS[t % 2], L)
            n += 1
    return n


N_SWEEP = len(MASKS) * len(PARITIES)


def run_width(impl, h, iw):
    """One width of the geometry's list at a height below the warm-up and across a segment seam."""
    nx = widths(impl, h)[iw]
    L = seg_rows(impl, h, nx)
    return _sweep(impl, h, nx, 2, L, iw) + _sweep(impl, h, nx, L + 1, L, iw + 1)


N_WIDTHS = 11


def prolong_heights(h, L):
    return tuple(sorted(set(heights(h, L)) | {2 * h + 1}))


def run_heights(impl, h):
    """Every height of the segment's list at the lane-pair tail and across a wave seam."""
    w, _ = geom(impl, h)
    n = 0
    for nx in (3, w + 1):
        L = seg_rows(impl, h, nx)
        for k, ny in enumerate(prolong_heights(h, L)):
            n += _sweep(impl, h, nx, ny, L, k)
    return n


def n_heights(h, L=HOST_SEG):
    return 2 * len(prolong_heights(h, L)) * N_SWEEP


def scalar_shapes(impl, h):
    w, _ = geom(impl, h)
    return ((1, 1), (2, h), (3, h + 1), (w + 1, 2), (5, HOST_SEG + 1))


def run_scalar_shapes(impl, h):
    """The alignment variants that must take the one-lane-per-cell kernel; e with an odd pitch and a base off by
    8 B stays on the walk."""
    n = 0
    for with_f in (False, True):
        for a, align in enumerate(ALIGN_F if with_f else ALIGN):
            if align == "fast":
                continue
            for i, (nx, ny) in enumerate(scalar_shapes(impl, h)):
                for mask in MASKS:
                    t = a + i + mask
                    check(impl, h, MODES[t % 3], nx, ny, mask, PARITIES[t % 4], align, with_f, OMEGAS[t % 2])
                    n += 1
    L = seg_rows(impl, h, 37)
    for k, (e_odd, e_base) in enumerate(((True, 0), (False, 1), (True, 1))):
        for mask in MASKS:
            check(impl, h, MODES[(k + mask) % 3], 37, 9, mask, PARITIES[(k + mask) % 4], "fast", bool(k % 2), 0.8, L,
                  e_odd, e_base)
            n += 1
    return n


N_SCALAR = (len(ALIGN) - 1 + len(ALIGN_F) - 1) * 5 * len(MASKS) + 3 * len(MASKS)


def run_negative_zero_ring(impl):
    """The fixed ring on the sides without the bit is -0.0 and the coarse cells beside it are far from zero: a
    ring cell that took the correction would no longer give the model's bits.  (A ring cell that merely lost its
    sign to a + 0.0 cannot show in out[R]: the cell enters sums only, and (W + E) + (N + S) is -0.0 only when
    all four are, after which o - u and u + omega*t give +0.0 for either sign.  The kernels keep the cell by a
    select, never by adding zero, and the bitwise comparison of u before and after covers the field itself.)"""
    def prep(e, u, region):
        x0, nx, y0, ny = region
        a = u.a
        ring = np.zeros(a.shape, dtype=bool)
        ring[y0 - 1:y0 + ny + 1, x0 - 1:x0 + nx + 1] = True
        ring[y0:y0 + ny, x0:x0 + nx] = False
        a[ring & ~np.isnan(a)] = -0.0
        e.a[~np.isnan(e.a)] += 3.0

    n = 0
    for h in HS:
        for mask in (0, 5, 10):
            for m, mode in enumerate(MODES):
                for align in ("fast", "odd_x0"):
                    check(impl, h, mode, 9, 6, mask, PARITIES[(h + m) % 4], align, False, 1.0,
                          seg_rows(impl, h, 9) if align == "fast" else None, prep=prep)
                    n += 1
    return n


# ---------------------------------------------------------------- identities
def grown(region, par, mask, h):
    """gmt_mg_prolong_add's arguments over B0: the region starts g cells earlier, and its parity and first
    coarse cell move with it so that every cell keeps its coarse column and row."""
    x0, nx, y0, ny = region
    gw, ge, gs, gn = (h if mask & bit else 0 for bit in (1, 2, 4, 8))
    qx, qy = (par[0] + gw) % 2, (par[1] + gs) % 2
    return ((x0 - gw, nx + gw + ge, y0 - gs, ny + gs + gn), (qx, qy),
            (CX0 + (qx - gw - par[0]) // 2, CY0 + (qy - gs - par[1]) // 2))


def _two_calls(impl, h, mode, region, par, mask, e, u, f, om):
    """gmt_mg_prolong_add over B0 on a copy of u, then gmt_mg_smooth_k or gmt_mg_smooth_rb."""
    x0, nx, y0, ny = region
    v = cc.Field(u.rows, u.ld, False, 0, np.nan)
    v.a[...] = u.a
    o = cc.Field(u.rows, x0 + nx + 1, False, 0, SENTINEL)
    dev = cc.Dev(impl, e=e, v=v, o=o, f=f)
    (bx, bnx, by, bny), (qx, qy), (cx, cy) = grown(region, par, mask, h)
    code = impl.lib.gmt_mg_prolong_add(bx, bnx, by, bny, qx, qy, dev.ptr("e"), cx, cy, dev.ld("e"), dev.ptr("v"),
                                       dev.ld("v"), impl.stream)
    assert code == 0, code
    if mode[0]:
        code = impl.lib.gmt_mg_smooth_rb(h, mode[1], x0, nx, y0, ny, mask, dev.ptr("v"), dev.ld("v"), dev.ptr("f"),
                                         dev.ld("f"), C0, C1, om, dev.ptr("o"), dev.ld("o"), impl.stream)
    else:
        code = impl.lib.gmt_mg_smooth_k(h, x0, nx, y0, ny, mask, dev.ptr("v"), dev.ld("v"), dev.ptr("f"), dev.ld("f"),
                                        C0, C1, om, dev.ptr("o"), dev.ld("o"), impl.stream)
    assert code == 0, code
    dev.fetch()
    return o.a[y0:y0 + ny, x0:x0 + nx].copy()


def run_identities(impl):
    """The fused pass is the two existing calls, through the backend's own kernels, on the walk and on the
    one-lane-per-cell kernel."""
    n = 0
    for h in HS:
        w, _ = geom(impl, h)
        for align in ("fast", "odd_x0"):
            for nx, ny in ((w + 3, 7), (6, 2 * HOST_SEG + 2)):
                for k, mask in enumerate((0, 15, 6, 9)):
                    for m, mode in enumerate(MODES):
                        par, with_f = PARITIES[(k + m + h) % 4], bool((k + m) % 2)
                        e, u, o, f, region = fields(h, nx, ny, mask, par, align, with_f)
                        x0, _, y0, _ = region
                        assert call(impl, h, mode, region, par, mask, e, u, o, f, 0.8) == 0
                        two = _two_calls(impl, h, mode, region, par, mask, e, u, f, 0.8)
                        assert same_bits(o.a[y0:y0 + ny, x0:x0 + nx], two), (h, align, nx, ny, mask, mode, par)
                        n += 1
    return n


N_IDENTITIES = 4 * 2 * 2 * 4 * 3


# --------------------------------------------------------- empty and refused
def run_empty_and_refusals(impl):
    """An empty region launches nothing and returns 0; the refused calls, with their codes; out stays intact."""
    L = impl.lib
    h = 3
    e, u, o, f, (x0, nx, y0, ny) = fields(h, 5, 4, 15, (1, 1), "fast", True)
    mx = mc.coarse_extent(nx, 1)
    d = cc.Dev(impl, e=e, u=u, o=o, f=f)

    def ps(h=h, rb=1, par=1, x0=x0, nx=nx, y0=y0, ny=ny, px=1, py=1, mask=15, pe=d.ptr("e"), cx0=CX0, cy0=CY0,
           lde=e.ld, pu=d.ptr("u"), ld=u.ld, pf=d.ptr("f"), ldf=f.ld, po=d.ptr("o"), ldo=o.ld):
        return L.gmt_mg_prolong_smooth(h, rb, par, x0, nx, y0, ny, px, py, mask, pe, cx0, cy0, lde, pu, ld, pf, ldf,
                                       C0, C1, 1.0, po, ldo, impl.stream)

    for enx, eny in ((0, 4), (5, 0), (0, 0)):
        assert ps(nx=enx, ny=eny) == 0
    codes = [ps(pu=None), ps(po=None), ps(pe=None), ps(nx=-1), ps(ny=-1), ps(nx=-1, ny=0),  # NULL and extents
             ps(mask=0, x0=0), ps(mask=0, y0=0), ps(mask=0, ld=x0 + nx), ps(ldo=x0 + nx - 1),  # gmt_mg_smooth's
             ps(mask=0, ldf=x0 + nx - 1),
             ps(h=0), ps(h=5), ps(h=-1), ps(mask=-1), ps(mask=16),                     # h and the mask
             ps(rb=-1), ps(rb=2), ps(par=-1), ps(par=2),                               # the smoother
             ps(px=2), ps(px=-1), ps(py=2), ps(py=-1),                                 # gmt_mg_prolong_add's
             ps(mask=0, cx0=0), ps(mask=0, cy0=0), ps(mask=0, lde=CX0 + mx),
             ps(mask=1, x0=h - 1), ps(mask=4, y0=h - 1),                               # the read sets' room
             ps(mask=2, ld=x0 + nx + h - 1), ps(mask=2, ldf=x0 + nx + h - 2),          # and pitches
             ps(mask=1, cx0=h // 2), ps(mask=4, cy0=h // 2), ps(mask=2, lde=CX0 + mx + h // 2),
             ps(po=d.ptr("u")), ps(po=d.ptr("u") + 8 * u.ld * 2),                      # out on u, e or f
             ps(po=d.ptr("e") + 8 * e.ld * 2, ldo=e.ld), ps(po=d.ptr("f") + 8 * f.ld * 2)]
    before = [t.store.copy() for t in (o, e, u, f)]
    d.fetch()
    assert all(same_bits(t.store, b) for t, b in zip((o, e, u, f), before))
    assert ps(pf=None, ldf=0) == 0 and ps(par=0) == 0 and ps(rb=0) == 0               # f is optional
    assert ps(mask=1, x0=h + 1) == 0 and ps(mask=0, x0=1, y0=1, cx0=1, cy0=1) == 0    # the least room that is enough
    assert ps(mask=2, lde=CX0 + mx + h // 2 + 1) == 0 and ps(mask=0, lde=CX0 + mx + 1) == 0
    return [int(c) for c in codes]


N_REFUSALS = 38


def main():
    """Every check through the CPU backend; prints one JSON line."""
    impl = host_impl(ctypes.CDLL(sys.argv[1]))
    n = [0, 0, 0, 0]
    for h in HS:
        n[0] += run_all_masks(impl, h)
        n[1] += sum(run_width(impl, h, iw) for iw in range(N_WIDTHS))
        n[2] += run_heights(impl, h)
        n[3] += run_scalar_shapes(impl, h)
    n.append(run_identities(impl))
    n.append(run_negative_zero_ring(impl))
    codes = run_empty_and_refusals(impl)
    e, u, o, _, region = fields(2, 100, 40, 0, (1, 1), "fast", False)
    print(json.dumps(dict(ok=True, cases=n, codes=codes,
                          path=list(path(impl, 2, (0, 0), region, (1, 1), 0, e, u, o)),
                          geom=[list(geom(impl, h)) for h in HS])))


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
