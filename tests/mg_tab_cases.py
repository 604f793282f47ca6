"""Cases and NumPy fp64 model of the table-driven multigrid transfers
(gmt_mg_xfer_plan_create, gmt_mg_restrict_tab, gmt_mg_prolong_add_tab), shared
by tests/test_mg_tab_kernels_gpu.py (the gfx950 kernels) and
tests/test_mg_tab_kernels_cpu.py (the CPU backend: this file run as a program
in a child process, as tests/mg_cases.py is).

The model is built from engine.mg_axis_table alone: the taps of a coarse point
are found by the definition (every fine i with q(i) = J, or with q(i) + 1 = J
and r(i) != 0), not by the closed forms the backends use.  Outputs are bitwise
the model's.  Everything outside a kernel's read set — the tapped rows x the
tapped columns of d, the interpolated rows x columns of e — is NaN, everything
outside its output region a sentinel that must be bitwise intact afterwards,
and inputs must be bitwise unchanged.  Only the all-aligned variant may take
the fast path; the path of every case is asserted where the backend has one.

An axis case is (n, m, fo, fn, co, cn): global fine and coarse point counts,
the region's fine cells fo+1 .. fo+fn and the coarse cells co+1 .. co+cn that
the anchor rule gives their owner.  x regions are the whole axis and every
share of its 2- and 3-way splits, so both tap halo sides and both coarse ring
ends are read; y regions have the heights of mg_cases.TRANSFER_NYS at the low
ring, in the interior and at the high ring of an even axis and inside an odd
one."""
import ctypes
import functools
import json
import sys
import types

import numpy as np

import cg_cases as cc
import mg_cases as mc

SENTINEL = cc.SENTINEL
ALIGN_R, ALIGN_P = mc.ALIGN_R, mc.ALIGN_P
PATH_NONE, PATH_SCALAR, PATH_PT = cc.PATH_NONE, cc.PATH_SCALAR, cc.PATH_PT
same_bits = cc.same_bits

# (n, m) of the x axis; the last two are odd axes (nested spacing), for mixed cases
X_AXES = ((4, 1), (6, 2), (10, 4), (22, 10), (46, 22), (94, 46), (15, 7), (47, 23))
WIDE = (766, 382)           # 383 fine pairs a row: the lane numbering wraps a 256-lane workgroup
WIDE_NYS = (1, 2, 9)
Y_EVEN, Y_ODD = (22, 10), (15, 7)


class Desc(ctypes.Structure):
    """gmt_mg_xfer_desc"""
    _fields_ = [(k, ctypes.c_int64 * 2) for k in ("n", "m", "fo", "fn", "co", "cn")]


def bounds(n, p):
    base, rem = divmod(n, p)
    return [i * base + min(i, rem) for i in range(p)] + [n]


def anchor_bound(n, m, b):
    """Coarse points whose anchor cell J*(n+1) // (m+1) is one of the fine cells 1 .. b."""
    return sum(1 for J in range(1, m + 1) if J * (n + 1) // (m + 1) <= b)


def share(n, m, fo, fn):
    co = anchor_bound(n, m, fo)
    return (n, m, fo, fn, co, anchor_bound(n, m, fo + fn) - co)


def x_regions(n, m):
    out = []
    for p in (1, 2, 3):
        b = bounds(n, p)
        out += [share(n, m, b[k], b[k + 1] - b[k]) for k in range(p)]
    return out


def y_regions(nys=mc.TRANSFER_NYS):
    out = []
    for h in nys:
        n, m = Y_EVEN
        for fo in sorted({0, (n - h) // 2 | 1, n - h}):
            out.append(share(n, m, fo, h))
        out.append(share(*Y_ODD, 3, h))
    return out


@functools.lru_cache(maxsize=None)
def axis_model(n, m):
    """By the definition, from engine.mg_axis_table: ({i: (q, t)}, {J: [(i, weight), ...] ascending})."""
    from gpu_mpi_tests_amd import engine

    q, t, r = engine.mg_axis_table(n, m)
    fine = {i: (int(q[i - 1]), float(t[i - 1])) for i in range(1, n + 1)}
    taps = {J: [] for J in range(1, m + 1)}
    for i in range(1, n + 1):
        qi, ti, ri = int(q[i - 1]), float(t[i - 1]), int(r[i - 1])
        if qi >= 1:
            taps[qi].append((i, 1.0 - ti))
        if ri != 0 and qi + 1 <= m:
            taps[qi + 1].append((i, ti))
    for J, lst in taps.items():
        lst.sort()
        assert [i for i, _ in lst] == list(range(lst[0][0], lst[0][0] + len(lst))), (n, m, J)  # consecutive
    return fine, taps


def region_model(axis):
    """Region-relative arrays of one axis case: pq, pt (fine), rf, rc, rw (coarse)."""
    n, m, fo, fn, co, cn = axis
    fine, taps = axis_model(n, m)
    pq = np.array([fine[fo + 1 + k][0] - (co + 1) for k in range(fn)], dtype=np.int64)
    pt = np.array([fine[fo + 1 + k][1] for k in range(fn)])
    rf = np.array([taps[co + 1 + k][0][0] - (fo + 1) for k in range(cn)], dtype=np.int64)
    rc = np.array([len(taps[co + 1 + k]) for k in range(cn)], dtype=np.int64)
    rw = np.zeros((cn, 4))
    for k in range(cn):
        for j, (_, w) in enumerate(taps[co + 1 + k]):
            rw[k, j] = w
    return types.SimpleNamespace(pq=pq, pt=pt, rf=rf, rc=rc, rw=rw)


def tapped(mod):
    """The region-relative fine indices the coarse cells of an axis read."""
    return sorted({int(f) + k for f, c in zip(mod.rf, mod.rc) for k in range(int(c))})


def ringed(mod):
    """The region-relative coarse indices the fine cells of an axis read."""
    return sorted({int(q) + k for q in mod.pq for k in (0, 1)})


def make_plan(impl, xaxis, yaxis):
    d = Desc()
    for k, vx, vy in zip(("n", "m", "fo", "fn", "co", "cn"), xaxis, yaxis):
        getattr(d, k)[0], getattr(d, k)[1] = vx, vy
    h = ctypes.c_void_p()
    code = impl.lib.gmt_mg_xfer_plan_create(ctypes.byref(d), ctypes.byref(h))
    return int(code), h


# --------------------------------------------------------------- restriction
def restrict_fields(xaxis, yaxis, align):
    x0, cx0, odd, base = ALIGN_R[align]
    y0, cy0 = 2, 1
    (nx, mx), (ny, my) = (xaxis[3], xaxis[5]), (yaxis[3], yaxis[5])
    mx_, my_ = region_model(xaxis), region_model(yaxis)
    g = cc._rng("mg_restrict_tab", xaxis, yaxis)
    d = cc.Field(y0 + ny + 3, x0 + nx + 4, "d" in odd, "d" in base, np.nan)  # NaN outside the read set
    rows, cols = tapped(my_), tapped(mx_)
    if rows and cols:
        d.a[np.ix_(y0 + np.array(rows), x0 + np.array(cols))] = g.random((len(rows), len(cols))) - 0.5
    s = cc.Field(cy0 + my + 1, cx0 + mx + 1, "s" in odd, "s" in base, SENTINEL)
    return d, s, (x0, y0), (cx0, cy0), (mx_, my_)


def restrict_reference(d, origin, mx_, my_):
    x0, y0 = origin
    D = d.a
    out = np.empty((len(my_.rf), len(mx_.rf)))
    for J in range(out.shape[0]):
        h = []
        for k in range(int(my_.rc[J])):
            row = D[y0 + int(my_.rf[J]) + k]
            col = x0 + mx_.rf
            v = (mx_.rw[:, 0] * row[col] + mx_.rw[:, 1] * row[col + 1]) + mx_.rw[:, 2] * row[col + 2]
            four = mx_.rc == 4
            v4 = v + mx_.rw[:, 3] * row[col + np.where(four, 3, 0)]
            h.append(np.where(four, v4, v))
        s = (my_.rw[J, 0] * h[0] + my_.rw[J, 1] * h[1]) + my_.rw[J, 2] * h[2]
        if len(h) == 4:
            s = s + my_.rw[J, 3] * h[3]
        out[J] = s
    return out


def check_restrict(impl, xaxis, yaxis, align):
    what = ("mg_restrict_tab", xaxis, yaxis, align)
    d, s, (x0, y0), (cx0, cy0), (mx_, my_) = restrict_fields(xaxis, yaxis, align)
    mx, my = xaxis[5], yaxis[5]
    dev = cc.Dev(impl, d=d, s=s)
    if impl.has_paths:
        p = impl.lib.gmt_mg_restrict_tab_path(x0, cx0, dev.ptr("d"), dev.ld("d"), dev.ptr("s"), dev.ld("s"))
        assert p == (PATH_PT if align == "fast" else PATH_SCALAR), (what, p)
    before = d.store.copy()
    want = restrict_reference(d, (x0, y0), mx_, my_)
    assert not np.isnan(want).any(), what  # the model reads nothing outside the read set
    code, plan = make_plan(impl, xaxis, yaxis)
    assert code == 0 and plan, (what, code)
    try:
        code = impl.lib.gmt_mg_restrict_tab(plan, x0, y0, dev.ptr("d"), dev.ld("d"), dev.ptr("s"), cx0, cy0,
                                            dev.ld("s"), impl.stream)
        assert code == 0, (what, code)
        dev.fetch()
    finally:
        impl.lib.gmt_mg_xfer_plan_destroy(plan)
    assert same_bits(before, d.store), what
    S = s.a
    assert same_bits(S[cy0:cy0 + my, cx0:cx0 + mx], want), what
    S[cy0:cy0 + my, cx0:cx0 + mx] = SENTINEL
    assert (s.store == SENTINEL).all(), what


# ------------------------------------------------------------- interpolation
def prolong_fields(xaxis, yaxis, align):
    x0, cx0, odd, base = ALIGN_P[align]
    y0, cy0 = 1, 2
    (nx, mx), (ny, my) = (xaxis[3], xaxis[5]), (yaxis[3], yaxis[5])
    mx_, my_ = region_model(xaxis), region_model(yaxis)
    g = cc._rng("mg_prolong_tab", xaxis, yaxis)
    e = cc.Field(cy0 + my + 2, cx0 + mx + 2, "e" in odd, "e" in base, np.nan)  # NaN outside the read set
    rows, cols = ringed(my_), ringed(mx_)
    if rows and cols:
        e.a[np.ix_(cy0 + np.array(rows), cx0 + np.array(cols))] = g.random((len(rows), len(cols))) - 0.5
    u = cc.Field(y0 + ny + 1, x0 + nx + 1, "u" in odd, "u" in base, SENTINEL)
    u.a[y0:y0 + ny, x0:x0 + nx] = g.random((ny, nx)) - 0.5
    return e, u, (x0, y0), (cx0, cy0), (mx_, my_)


def prolong_reference(e, u, origin, coarse, mx_, my_):
    (x0, y0), (cx0, cy0) = origin, coarse
    E, U = e.a, u.a
    nx, ny = len(mx_.pq), len(my_.pq)
    want = np.empty((ny, nx))
    I = cx0 + mx_.pq
    w1x = mx_.pt
    w0x = 1.0 - w1x
    for j in range(ny):
        J = cy0 + int(my_.pq[j])
        w1y = float(my_.pt[j])
        w0y = 1.0 - w1y
        bot = w0x * E[J, I] + w1x * E[J, I + 1]
        top = w0x * E[J + 1, I] + w1x * E[J + 1, I + 1]
        v = w0y * bot + w1y * top
        want[j] = U[y0 + j, x0:x0 + nx] + v
    return want


def check_prolong(impl, xaxis, yaxis, align):
    what = ("mg_prolong_add_tab", xaxis, yaxis, align)
    e, u, (x0, y0), (cx0, cy0), (mx_, my_) = prolong_fields(xaxis, yaxis, align)
    nx, ny = xaxis[3], yaxis[3]
    dev = cc.Dev(impl, e=e, u=u)
    if impl.has_paths:
        p = impl.lib.gmt_mg_prolong_add_tab_path(x0, dev.ptr("e"), dev.ld("e"), dev.ptr("u"), dev.ld("u"))
        assert p == (PATH_PT if align == "fast" else PATH_SCALAR), (what, p)
    before = e.store.copy()
    want = prolong_reference(e, u, (x0, y0), (cx0, cy0), mx_, my_)
    assert not np.isnan(want).any(), what
    code, plan = make_plan(impl, xaxis, yaxis)
    assert code == 0 and plan, (what, code)
    try:
        code = impl.lib.gmt_mg_prolong_add_tab(plan, x0, y0, dev.ptr("e"), cx0, cy0, dev.ld("e"), dev.ptr("u"),
                                               dev.ld("u"), impl.stream)
        assert code == 0, (what, code)
        dev.fetch()
    finally:
        impl.lib.gmt_mg_xfer_plan_destroy(plan)
    assert same_bits(before, e.store), what
    U = u.a
    assert same_bits(U[y0:y0 + ny, x0:x0 + nx], want), what
    U[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (u.store == SENTINEL).all(), what


# ------------------------------------------------------------------ the sets
def case_list(xpair):
    """Every (xaxis, yaxis) of one x axis."""
    ys = y_regions(WIDE_NYS if xpair == WIDE else mc.TRANSFER_NYS)
    return [(xa, ya) for xa in x_regions(*xpair) for ya in ys]


def run_restrict_shapes(impl, xpair):
    n = 0
    for xa, ya in case_list(xpair):
        for align in ALIGN_R:
            check_restrict(impl, xa, ya, align)
            n += 1
    return n


def run_prolong_shapes(impl, xpair):
    n = 0
    for xa, ya in case_list(xpair):
        for align in ALIGN_P:
            check_prolong(impl, xa, ya, align)
            n += 1
    return n


def n_cases(xpair):
    return len(case_list(xpair))


def assert_coverage():
    """What the set must contain, asserted on the model."""
    axes = [a for xp in X_AXES + (WIDE,) for a in x_regions(*xp)] + y_regions()
    mods = [(a, region_model(a)) for a in axes]
    counts = {int(c) for _, mo in mods for c in mo.rc}
    assert counts == {3, 4}, counts                                    # 3-tap and 4-tap columns and rows
    assert any(0.0 in mo.pt for a, mo in mods if a[0] % 2 == 1)        # a fine point on a coarse point (r = 0)
    assert all(0.0 not in mo.pt for a, mo in mods if a[0] % 2 == 0)    # never on an even axis
    assert any(a[5] and a[4] == 0 for a, _ in mods) and any(a[5] and a[4] + a[5] == a[1] for a, _ in mods)  # rings
    lows = {min(tapped(mo)) for _, mo in mods if len(mo.rf)}
    highs = {max(tapped(mo)) - (a[3] - 1) for a, mo in mods if len(mo.rf)}
    assert min(lows) < 0 and max(highs) > 0, (lows, highs)             # both tap halo sides are read
    assert min(lows) >= -2 and max(highs) <= 2, (lows, highs)
    assert any(-1 in ringed(mo) for _, mo in mods) and any(a[5] in ringed(mo) for a, mo in mods)  # both ring sides
    assert any(a[5] % 2 == 1 for a, _ in mods)                          # an odd coarse width: a single last column
    assert (WIDE[0] + 1) // 2 > 256


# --------------------------------------------------------- empty and refused
BAD_DESCS = (
    ((22, 10, 4, 4, 1, 4), (22, 10, 0, 22, 0, 10)),    # x: the taps of J = 5 lie 5 cells above the region
    ((22, 10, 4, 8, 1, 2), (22, 10, 0, 22, 0, 10)),    # x: fine cell 12 interpolates from J = 5, 6: 2 outside the coarse region
    ((22, 10, 0, 22, 0, 10), (22, 10, 4, 4, 1, 4)),    # the same on y
    ((22, 10, 0, 22, 0, 10), (22, 10, 4, 8, 1, 2)),
    ((22, 21, 0, 22, 0, 21), (22, 10, 0, 22, 0, 10)),  # spacing 23/22: a coarse point with fewer than 3 taps
    ((22, 4, 0, 22, 0, 4), (22, 10, 0, 22, 0, 10)),    # spacing 4.6: more than 4 taps
    ((22, 0, 0, 22, 0, 0), (22, 10, 0, 22, 0, 10)),    # no coarse point
    ((22, 10, 20, 4, 0, 10), (22, 10, 0, 22, 0, 10)),  # a region beyond the axis
    ((22, 10, -1, 4, 0, 2), (22, 10, 0, 22, 0, 10)),
    ((22, 10, 0, 22, 8, 4), (22, 10, 0, 22, 0, 10)),
)


def run_empty_and_refusals(impl):
    """Refused descriptions create no plan; an empty region launches nothing and returns 0; the refused launches."""
    L = impl.lib
    codes = []
    for xa, ya in BAD_DESCS:
        code, plan = make_plan(impl, xa, ya)
        assert not plan, (xa, ya)
        codes.append(code)
    null = ctypes.c_void_p()
    codes.append(L.gmt_mg_xfer_plan_create(None, ctypes.byref(null)))
    codes.append(L.gmt_mg_xfer_plan_create(ctypes.byref(Desc()), None))
    L.gmt_mg_xfer_plan_destroy(None)

    xa, ya = share(22, 10, 7, 8), share(22, 10, 0, 5)
    d, s, (x0, y0), (cx0, cy0), _ = restrict_fields(xa, ya, "fast")
    e, u, (ux0, uy0), (ex0, ey0), _ = prolong_fields(xa, ya, "fast")
    dev = cc.Dev(impl, d=d, s=s, e=e, u=u)
    code, plan = make_plan(impl, xa, ya)
    assert code == 0 and plan
    empties = [make_plan(impl, share(22, 10, 7, 0), ya), make_plan(impl, xa, share(22, 10, 5, 0)),
               make_plan(impl, (22, 10, 7, 0, 3, 0), (22, 10, 0, 0, 0, 0))]
    assert all(c == 0 and p for c, p in empties), empties

    def rs(plan=plan, x0=x0, y0=y0, pd=dev.ptr("d"), ldd=d.ld, ps=dev.ptr("s"), cx0=cx0, cy0=cy0, ldc=s.ld):
        return L.gmt_mg_restrict_tab(plan, x0, y0, pd, ldd, ps, cx0, cy0, ldc, impl.stream)

    def pr(plan=plan, x0=ux0, y0=uy0, pe=dev.ptr("e"), cx0=ex0, cy0=ey0, lde=e.ld, pu=dev.ptr("u"), ld=u.ld):
        return L.gmt_mg_prolong_add_tab(plan, x0, y0, pe, cx0, cy0, lde, pu, ld, impl.stream)

    try:
        for _, p in empties:
            assert rs(plan=p) == 0 and pr(plan=p) == 0
            assert rs(plan=p, pd=None, ps=None) == 0 and pr(plan=p, pe=None, pu=None) == 0  # nothing is looked at
        nx, mx = xa[3], xa[5]
        codes += [rs(plan=None), rs(pd=None), rs(ps=None), rs(x0=1), rs(y0=1), rs(cx0=-1), rs(cy0=-1),
                  rs(ldd=x0 + nx + 1), rs(ldc=cx0 + mx - 1)]
        codes += [pr(plan=None), pr(pe=None), pr(pu=None), pr(x0=0), pr(y0=0), pr(cx0=0), pr(cy0=0),
                  pr(lde=ex0 + mx), pr(ld=ux0 + nx - 1)]
        before = {k: v.store.copy() for k, v in dev.fields.items()}
        dev.fetch()
        assert all(same_bits(before[k], v.store) for k, v in dev.fields.items())
    finally:
        for p in [plan] + [p for _, p in empties]:
            L.gmt_mg_xfer_plan_destroy(p)
    return [int(c) for c in codes]


N_REFUSALS = len(BAD_DESCS) + 2 + 9 + 9


def host_impl(lib):
    from gpu_mpi_tests_amd import _native

    _native.bind(lib, [n for n in _native._SIGS if n.startswith("gmt_mg_")])
    return types.SimpleNamespace(lib=lib, stream=None, has_paths=False, upload=lambda a: a.copy(),
                                 download=lambda h: h.copy(), ptr=lambda h: h.ctypes.data)


def main():
    """Every check through the CPU backend; prints one JSON line."""
    impl = host_impl(ctypes.CDLL(sys.argv[1]))
    assert_coverage()
    n = [0, 0]
    for xp in X_AXES + (WIDE,):
        n[0] += run_restrict_shapes(impl, xp)
        n[1] += run_prolong_shapes(impl, xp)
    codes = run_empty_and_refusals(impl)
    paths = [int(impl.lib.gmt_mg_restrict_tab_path(8, 8, None, 64, None, 64)),
             int(impl.lib.gmt_mg_prolong_add_tab_path(8, None, 64, None, 64))]
    print(json.dumps(dict(ok=True, cases=n, codes=codes, paths=paths)))


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
