"""Cases and NumPy fp64 reference of the read-only Jacobi residual
(gmt_jacobi5_resid), shared by tests/test_resid_gpu.py (the gfx950 kernels
through torch) and tests/test_resid_cpu.py (the CPU backend: this file run as
a program in a child process, because build/lib-host/libgmt.so shares its
SONAME with the GPU library).

A case is a field whose every cell outside the region's 1-wide plus-shaped
read set is NaN — the ring's four corners and everything beyond the ring
included — so a read outside the set poisons the result.  `call(case)` runs
the implementation under test and returns (sum d^2, max |d|); it also owns
the checks that u is bitwise unchanged and the canary behind the workspace."""
import json
import math
import sys

import numpy as np
import torch

NXS = (1, 2, 3, 127, 128, 129, 130, 255, 257, 513)  # lane-pair tail, wave and workgroup column edges
C0, C1 = 0.25, -0.01
# name -> (x0, row pitch parity, base offset in doubles, f's pitch parity); only "walk" may take the fast path
ALIGN = {"walk": (8, 0, 0, 0), "odd_x0": (9, 0, 0, 0), "odd_ld": (8, 1, 0, 0), "base_8B": (8, 0, 1, 0),
         "f_odd_ld": (8, 0, 0, 1)}


def ny_list(L):
    """A window shorter than its depth, and the segment seams (L rows per segment)."""
    return tuple(sorted({1, 2, 3, L - 1, L, L + 1, 2 * L + 1} - {0}))


def make_case(nx, ny, align="walk", with_f=False, seed=0):
    x0, ld_par, off, ldf_par = ALIGN[align]
    y0 = 2
    rows = y0 + ny + 2  # one NaN row beyond the ring on either side
    ld = x0 + nx + 3
    ld += (ld % 2) != ld_par
    g = torch.Generator().manual_seed(1000 * seed + 7 * nx + ny)
    store = np.full(off + rows * ld, np.nan)
    U = store[off:off + rows * ld].reshape(rows, ld)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).numpy()  # noqa: E731
    U[y0:y0 + ny, x0:x0 + nx] = rnd(ny, nx)
    U[y0:y0 + ny, x0 - 1] = rnd(ny)
    U[y0:y0 + ny, x0 + nx] = rnd(ny)
    U[y0 - 1, x0:x0 + nx] = rnd(nx)
    U[y0 + ny, x0:x0 + nx] = rnd(nx)
    case = dict(store=store, off=off, rows=rows, ld=ld, region=(x0, nx, y0, ny), fstore=None, ldf=0, align=align)
    if with_f:
        ldf = x0 + nx
        ldf += (ldf % 2) != ldf_par
        fstore = np.full(rows * ldf, np.nan)
        fstore.reshape(rows, ldf)[y0:y0 + ny, x0:x0 + nx] = rnd(ny, nx)
        case.update(fstore=fstore, ldf=ldf)
    return case


def views(case):
    U = case["store"][case["off"]:case["off"] + case["rows"] * case["ld"]].reshape(case["rows"], case["ld"])
    F = None if case["fstore"] is None else case["fstore"].reshape(case["rows"], case["ldf"])
    return U, F


def reference(case):
    """(fsum of d^2, max |d|, d) in the operation order of the kernels."""
    U, F = views(case)
    x0, nx, y0, ny = case["region"]
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    o = C0 * ((U[ys, x0 - 1:x0 - 1 + nx] + U[ys, x0 + 1:x0 + 1 + nx]) + (U[y0 - 1:y0 - 1 + ny, xs] + U[y0 + 1:y0 + 1 + ny, xs]))
    if F is not None:
        o = o + C1 * F[ys, xs]
    d = o - U[ys, xs]
    return math.fsum((d * d).ravel().tolist()), float(np.abs(d).max()), d


def check(case, got, tol_sum, what):
    s, m, _ = reference(case)
    assert abs(got[0] - s) <= tol_sum * max(1.0, s), (what, got, s)
    if case["fstore"] is None:  # no contractible multiply-add in the cell: bitwise
        assert got[1] == m, (what, got, m)
    else:
        assert abs(got[1] - m) <= 1e-14 * m, (what, got, m)


def run_shapes(call, tol_sum, nx, with_f, seg_rows, path=None):
    """Every ny and alignment of one width.  path(case) -> (is_row_walk, seg_rows), GPU only."""
    for align in ALIGN:
        if align == "f_odd_ld" and not with_f:
            continue
        for ny in ny_list(seg_rows(nx)):
            case = make_case(nx, ny, align, with_f)
            what = (nx, ny, align, with_f)
            if path is not None:
                walk, seg = path(case)
                assert walk == (align == "walk"), what
                assert seg == (seg_rows(nx) if walk else 0), (what, seg)
            check(case, call(case), tol_sum, what)


def spike_positions(nx, ny, L):
    """First / last row and column, both sides of a wave edge (columns 127 | 128) and of a segment seam."""
    return [(0, nx // 2), (ny - 1, nx // 3), (ny // 2, 0), (ny // 3, nx - 1), (ny // 2, 127), (ny // 2, 128),
            (L - 1, nx // 2), (L, nx // 2 + 1)]


def run_spikes(call, nx, ny, L, align="walk"):
    for (y, x) in spike_positions(nx, ny, L):
        case = make_case(nx, ny, align, seed=3)
        U, _ = views(case)
        x0, _, y0, _ = case["region"]
        U[y0 + y, x0 + x] = 1000.0
        _, m, d = reference(case)
        assert np.unravel_index(np.argmax(np.abs(d)), d.shape) == (y, x)
        got = call(case)
        assert got[1] == m, ((y, x), got, m)


def run_nan(call, nx, ny, align="walk"):
    for (y, x) in ((0, 0), (ny - 1, nx - 1), (ny // 2, nx // 2)):
        case = make_case(nx, ny, align, seed=4)
        U, _ = views(case)
        x0, _, y0, _ = case["region"]
        U[y0 + y, x0 + x] = np.nan
        got = call(case)
        assert got[1] == math.inf and math.isnan(got[0]), ((y, x), got)


def run_empty(call):
    for nx, ny in ((0, 5), (5, 0), (0, 0)):
        case = make_case(max(nx, 1), max(ny, 1))
        x0, _, y0, _ = case["region"]
        case["region"] = (x0, nx, y0, ny)
        assert tuple(call(case)) == (0.0, 0.0), (nx, ny)


# ---------------------------------------------------------------- CPU backend
def host_call(lib):
    import ctypes

    i64, dbl, vp = ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    lib.gmt_jacobi5_resid_workspace.restype = i64
    lib.gmt_jacobi5_resid_workspace.argtypes = [i64, i64]
    lib.gmt_jacobi5_resid.restype = ctypes.c_int
    lib.gmt_jacobi5_resid.argtypes = [i64, i64, i64, i64, vp, i64, vp, i64, dbl, dbl, vp, vp, vp]

    def call(case):
        x0, nx, y0, ny = case["region"]
        before = case["store"].copy()
        n = int(lib.gmt_jacobi5_resid_workspace(nx, ny))
        ws = np.full(n + 8, 12345.0)
        out = np.full(2, -1.0)
        u = case["store"][case["off"]:]
        f = case["fstore"]
        rc = lib.gmt_jacobi5_resid(x0, nx, y0, ny, u.ctypes.data, case["ld"], f.ctypes.data if f is not None else None,
                                   case["ldf"], C0, C1 if f is not None else 0.0, out.ctypes.data,
                                   ws.ctypes.data, None)
        assert rc == 0, rc
        assert np.array_equal(before, case["store"], equal_nan=True)  # u is never written
        assert (ws[n:] == 12345.0).all()                              # nor anything past the workspace
        return float(out[0]), float(out[1])

    return call


def main():
    """The definition checks through the CPU backend; prints one JSON line."""
    import ctypes

    lib = ctypes.CDLL(sys.argv[1])
    call = host_call(lib)
    i64 = ctypes.c_int64
    seg = i64(7)
    lib.gmt_jacobi5_resid_path.restype = ctypes.c_int
    path = lib.gmt_jacobi5_resid_path(i64(8), i64(100), i64(100), None, i64(128), None, i64(0), ctypes.byref(seg))
    n = 0
    for nx in NXS:
        for with_f in (False, True):
            run_shapes(call, 1e-12, nx, with_f, lambda _nx: 8)
            n += 1
    run_spikes(call, 300, 2 * 8 + 1, 8)
    run_nan(call, 130, 9)
    run_empty(call)
    big = make_case(4000, 2000, seed=5)
    got = call(big)
    s, m, _ = reference(big)
    assert abs(got[0] - s) <= 1e-10 * s and got[1] == m, (got, s, m)
    assert call(big) == got
    print(json.dumps(dict(ok=True, widths=n, path=[int(path), int(seg.value)])))


if __name__ == "__main__":
    main()
