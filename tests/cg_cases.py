"""Cases and NumPy fp64 model of the conjugate-gradient kernels (gmt_cg_apply,
gmt_cg_update, gmt_cg_dir), shared by tests/test_cg_kernels_gpu.py (the gfx950
kernels) and tests/test_cg_kernels_cpu.py (the CPU backend: this file run as a
program in a child process, because build/lib-host/libgmt.so shares its SONAME
with the GPU library).

Both run the C ABI through a small `impl` (the loaded library, upload /
download of a flat fp64 store, a base pointer): the calls, the references and
the checks below are the same code on either backend.

Fields are bitwise NumPy's (no contraction anywhere in a cell); sums are
compared with math.fsum within tol_sum * max(1, scale), where scale is the sum
of the terms' magnitudes (p*q cancels); maxima are bitwise.  Everything outside
apply's plus-shaped read set is NaN, its output's surroundings a sentinel, and a
canary follows the declared workspace.  Only the all-aligned variant may take
the fast path; the path of every case is asserted where the backend has one."""
import ctypes
import json
import math
import sys
import types
import zlib

import numpy as np

import resid_cases as rc

NXS = rc.NXS  # lane-pair tail, wave and workgroup column edges
C0, C1 = rc.C0, rc.C1
SENTINEL, CANARY = -7777.25, 12345.0
PATH_NONE, PATH_SCALAR, PATH_PT, PATH_ROW_WALK = 0, 1, 2, 5
UPDATE_NYS = (1, 2, 3, 4, 5, 9)  # around the rows a block of the streaming kernels takes (4)
# (num, den): a plain coefficient, then the three denominators that give coefficient 0
COEFS = ((0.7, 1.3), (1.0, 0.0), (1.0, -2.0), (1.0, math.nan))


def aligns(fields, extra=()):
    """name -> (x0, fields with an odd pitch, fields whose base is off by 8 B): resid_cases.ALIGN's variants
    with each field in turn; only `fast` may take the fast path."""
    out = {"fast": (8, (), ()), "odd_x0": (9, (), ())}
    for f in fields:
        out[f + "_odd_ld"] = (8, (f,), ())
        out[f + "_base_8B"] = (8, (), (f,))
    for f in extra:
        out[f + "_odd_ld"] = (8, (f,), ())
    return out


APPLY_ALIGN = aligns("pq")
APPLY_ALIGN_F = aligns("pq", extra="f")
UPDATE_ALIGN = aligns("pqxr")
DIR_ALIGN = aligns("rp")
assert set(rc.ALIGN) == {"walk", "odd_x0", "odd_ld", "base_8B", "f_odd_ld"}  # the variants extended above


class Field:
    """rows x ld doubles at `off` doubles from the start of a flat store."""

    def __init__(self, rows, min_ld, odd_ld, off, fill):
        self.rows, self.off = rows, int(off)
        self.ld = min_ld + ((min_ld % 2) != int(odd_ld))
        self.store = np.full(self.off + rows * self.ld, fill)

    @property
    def a(self):
        return self.store[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def fsum(a):
    return math.fsum(np.asarray(a).ravel().tolist())


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------ the calls
class Dev:
    """The fields of one call on the backend; `fetch` copies them back into the Field stores."""

    def __init__(self, impl, **fields):
        self.impl, self.fields = impl, {k: v for k, v in fields.items() if v is not None}
        self.h = {k: impl.upload(v.store) for k, v in self.fields.items()}

    def ptr(self, k):
        return self.impl.ptr(self.h[k]) + 8 * self.fields[k].off if k in self.h else None

    def ld(self, k):
        return self.fields[k].ld if k in self.fields else 0

    def fetch(self):
        for k, v in self.fields.items():
            v.store[:] = self.impl.download(self.h[k])


def _scalars(impl, *vals):
    h = impl.upload(np.array(vals, dtype=np.float64))
    return h, [impl.ptr(h) + 8 * i for i in range(len(vals))]


def _with_ws(impl, region, fn):
    """fn(out pointer, workspace pointer) -> rc; returns (rc, out) and checks the canary behind the workspace."""
    n = int(impl.lib.gmt_cg_workspace(region[1], region[3]))
    ws = impl.upload(np.full(n + 8, CANARY))
    out = impl.upload(np.full(2, -1.0))
    code = fn(impl.ptr(out), impl.ptr(ws))
    assert (impl.download(ws)[n:] == CANARY).all()
    o = impl.download(out)
    return code, (float(o[0]), float(o[1]))


def call_apply(impl, mode, region, p, q, f=None, c1=C1):
    d = Dev(impl, p=p, q=q, f=f)
    x0, nx, y0, ny = region
    code, out = _with_ws(impl, region, lambda o, w: impl.lib.gmt_cg_apply(
        mode, x0, nx, y0, ny, d.ptr("p"), d.ld("p"), d.ptr("f"), d.ld("f"), C0, c1 if f is not None else 0.0,
        d.ptr("q"), d.ld("q"), o, w, impl.stream))
    assert code == 0, code
    d.fetch()
    return out


def call_update(impl, region, num, den, p, q, x, r):
    d = Dev(impl, p=p, q=q, x=x, r=r)
    sh, (pn, pd) = _scalars(impl, num, den)
    x0, nx, y0, ny = region
    code, out = _with_ws(impl, region, lambda o, w: impl.lib.gmt_cg_update(
        x0, nx, y0, ny, pn, pd, d.ptr("p"), d.ld("p"), d.ptr("q"), d.ld("q"), d.ptr("x"), d.ld("x"), d.ptr("r"),
        d.ld("r"), o, w, impl.stream))
    assert code == 0, code
    d.fetch()
    assert same_bits(impl.download(sh), np.array([num, den]))
    return out


def call_dir(impl, region, num, den, r, p):
    d = Dev(impl, r=r, p=p)
    sh, (pn, pd) = _scalars(impl, num, den)
    x0, nx, y0, ny = region
    code = impl.lib.gmt_cg_dir(x0, nx, y0, ny, pn, pd, d.ptr("r"), d.ld("r"), d.ptr("p"), d.ld("p"), impl.stream)
    assert code == 0, code
    d.fetch()


def apply_path(impl, region, p, q, f=None):
    d = Dev(impl, p=p, q=q, f=f)
    seg = ctypes.c_int64(-1)
    path = impl.lib.gmt_cg_apply_path(region[0], region[1], region[3], d.ptr("p"), d.ld("p"), d.ptr("f"), d.ld("f"),
                                      d.ptr("q"), d.ld("q"), ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def seg_rows(impl, nx):
    """Rows per segment of the row walk for this width (8 on a backend without kernels)."""
    if not impl.has_paths:
        return 8
    p, q, _, region = apply_fields(nx, 1, "fast", False)
    path, seg = apply_path(impl, region, p, q)
    assert path == PATH_ROW_WALK and seg >= 2, (path, seg)
    return seg


# ---------------------------------------------------------------------- apply
def apply_fields(nx, ny, align, with_f, seed=0, table=None):
    x0, odd, base = (table or (APPLY_ALIGN_F if with_f else APPLY_ALIGN))[align]
    y0 = 2
    rows = y0 + ny + 2  # one NaN row beyond the ring on either side
    g = _rng("apply", nx, ny, seed)
    p = Field(rows, x0 + nx + 3, "p" in odd, "p" in base, np.nan)
    P = p.a
    P[y0:y0 + ny, x0:x0 + nx] = g.random((ny, nx)) - 0.5
    P[y0:y0 + ny, x0 - 1] = g.random(ny)
    P[y0:y0 + ny, x0 + nx] = g.random(ny)
    P[y0 - 1, x0:x0 + nx] = g.random(nx)
    P[y0 + ny, x0:x0 + nx] = g.random(nx)
    q = Field(rows, x0 + nx + 1, "q" in odd, "q" in base, SENTINEL)
    f = None
    if with_f:
        f = Field(rows, x0 + nx, "f" in odd, 0, np.nan)
        f.a[y0:y0 + ny, x0:x0 + nx] = g.random((ny, nx))
    return p, q, f, (x0, nx, y0, ny)


def apply_reference(mode, region, p, f):
    """(q, sum, scale of the sum, max) in the operation order of the kernels."""
    x0, nx, y0, ny = region
    U = p.a
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    o = C0 * ((U[ys, x0 - 1:x0 - 1 + nx] + U[ys, x0 + 1:x0 + 1 + nx]) + (U[y0 - 1:y0 - 1 + ny, xs] + U[y0 + 1:y0 + 1 + ny, xs]))
    c = U[ys, xs]
    if mode == 0:
        q = c - o
        return q, fsum(c * q), fsum(np.abs(c * q)), 0.0
    if f is not None:
        o = o + C1 * f.a[ys, xs]
    q = o - c
    return q, fsum(q * q), fsum(q * q), float(np.abs(q).max())


def check_apply(impl, tol_sum, mode, nx, ny, align, with_f, seg=None, seed=0):
    what = ("apply", mode, nx, ny, align, with_f)
    p, q, f, region = apply_fields(nx, ny, align, with_f, seed)
    x0, _, y0, _ = region
    if impl.has_paths:
        path, s = apply_path(impl, region, p, q, f if mode == 1 else None)
        fast = align == "fast" or (mode == 0 and align == "f_odd_ld")  # mode 0 ignores f
        assert path == (PATH_ROW_WALK if fast else PATH_SCALAR), (what, path)
        assert s == (seg if fast else 0), (what, s, seg)
    before = p.store.copy()
    fbefore = None if f is None else f.store.copy()
    got = call_apply(impl, mode, region, p, q, f)
    want, s, scale, m = apply_reference(mode, region, p, f if mode == 1 else None)
    assert same_bits(before, p.store), what                       # p is never written
    assert f is None or same_bits(fbefore, f.store), what
    Q = q.a
    assert same_bits(Q[y0:y0 + ny, x0:x0 + nx], want), what       # bitwise NumPy
    Q[y0:y0 + ny, x0:x0 + nx] = SENTINEL
    assert (q.store == SENTINEL).all(), what                      # nothing outside the region is written
    assert abs(got[0] - s) <= tol_sum * max(1.0, scale), (what, got, s, scale)
    assert got[1] == m, (what, got, m)
    if mode == 1:  # bitwise the d of the residual kernel's reference
        case = dict(store=p.store, off=p.off, rows=p.rows, ld=p.ld, region=region,
                    fstore=None if f is None else f.store, ldf=0 if f is None else f.ld)
        assert same_bits(rc.reference(case)[2], want), what


def run_apply_shapes(impl, tol_sum, nx, mode, with_f):
    L = seg_rows(impl, nx)
    for align in (APPLY_ALIGN_F if with_f else APPLY_ALIGN):
        for ny in rc.ny_list(L):
            check_apply(impl, tol_sum, mode, nx, ny, align, with_f, L)


def run_apply_nan(impl, nx, ny):
    """A NaN cell: mode 1 reports {NaN, +inf}."""
    for (y, x) in ((0, 0), (ny - 1, nx - 1), (ny // 2, nx // 2)):
        p, q, _, region = apply_fields(nx, ny, "fast", False, seed=4)
        p.a[region[2] + y, region[0] + x] = np.nan
        got = call_apply(impl, 1, region, p, q)
        assert math.isnan(got[0]) and got[1] == math.inf, ((y, x), got)


# ------------------------------------------------------------- update and dir
def stream_fields(names, table, nx, ny, align, seed=0):
    """Random fields (every cell, so a write outside the region shows) for update / dir."""
    x0, odd, base = table[align]
    y0 = 1
    g = _rng("stream", names, nx, ny, seed)
    out = {}
    for k in names:
        fld = Field(y0 + ny + 1, x0 + nx + 1, k in odd, k in base, 0.0)
        fld.store[:] = g.random(fld.store.shape) - 0.5
        out[k] = fld
    return out, (x0, nx, y0, ny)


def coef(num, den):
    return num / den if den > 0 else 0.0


def check_update(impl, tol_sum, nx, ny, align, num=0.7, den=1.3, nan_cell=None, seed=0):
    what = ("update", nx, ny, align, num, den, nan_cell)
    F, region = stream_fields("pqxr", UPDATE_ALIGN, nx, ny, align, seed)
    x0, _, y0, _ = region
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    if nan_cell is not None:
        F["r"].a[y0 + nan_cell[0], x0 + nan_cell[1]] = np.nan
    if impl.has_paths:
        d = Dev(impl, **F)
        path = impl.lib.gmt_cg_update_path(x0, d.ptr("p"), d.ld("p"), d.ptr("q"), d.ld("q"), d.ptr("x"), d.ld("x"),
                                           d.ptr("r"), d.ld("r"))
        assert path == (PATH_PT if align == "fast" else PATH_SCALAR), (what, path)
    old = {k: v.store.copy() for k, v in F.items()}
    a = coef(num, den)
    want_x, want_r = F["x"].store.copy(), F["r"].store.copy()
    wx = want_x[F["x"].off:].reshape(F["x"].rows, F["x"].ld)
    wr = want_r[F["r"].off:].reshape(F["r"].rows, F["r"].ld)
    wx[ys, xs] = F["x"].a[ys, xs] + a * F["p"].a[ys, xs]
    wr[ys, xs] = F["r"].a[ys, xs] - a * F["q"].a[ys, xs]
    got = call_update(impl, region, num, den, F["p"], F["q"], F["x"], F["r"])
    assert same_bits(F["p"].store, old["p"]) and same_bits(F["q"].store, old["q"]), what
    assert same_bits(F["x"].store, want_x), what  # bitwise NumPy in the region, untouched outside
    assert same_bits(F["r"].store, want_r), what
    if a == 0.0:  # den = 0, < 0 or NaN: nothing moves
        assert same_bits(F["x"].store, old["x"]) and same_bits(F["r"].store, old["r"]), what
    rr = wr[ys, xs]
    if nan_cell is not None:
        assert math.isnan(got[0]) and got[1] == math.inf, (what, got)
        return
    s = fsum(rr * rr)
    assert abs(got[0] - s) <= tol_sum * max(1.0, s), (what, got, s)
    assert got[1] == float(np.abs(rr).max()), (what, got)


def check_dir(impl, nx, ny, align, num=0.9, den=1.7, seed=0):
    what = ("dir", nx, ny, align, num, den)
    F, region = stream_fields("rp", DIR_ALIGN, nx, ny, align, seed)
    x0, _, y0, _ = region
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    if impl.has_paths:
        d = Dev(impl, **F)
        path = impl.lib.gmt_cg_dir_path(x0, d.ptr("r"), d.ld("r"), d.ptr("p"), d.ld("p"))
        assert path == (PATH_PT if align == "fast" else PATH_SCALAR), (what, path)
    old = {k: v.store.copy() for k, v in F.items()}
    b = coef(num, den)
    want = F["p"].store.copy()
    wp = want[F["p"].off:].reshape(F["p"].rows, F["p"].ld)
    wp[ys, xs] = F["r"].a[ys, xs] + b * F["p"].a[ys, xs]
    call_dir(impl, region, num, den, F["r"], F["p"])
    assert same_bits(F["r"].store, old["r"]), what
    assert same_bits(F["p"].store, want), what
    if b == 0.0:
        assert same_bits(F["p"].a[ys, xs], old["r"][F["r"].off:].reshape(F["r"].rows, F["r"].ld)[ys, xs]), what


def run_stream_shapes(impl, tol_sum, nx):
    for ny in UPDATE_NYS:
        for align in UPDATE_ALIGN:
            check_update(impl, tol_sum, nx, ny, align)
        for align in DIR_ALIGN:
            check_dir(impl, nx, ny, align)


def run_coefs(impl, tol_sum):
    """den = 0, den < 0 and den = NaN give coefficient 0 on both paths; a NaN cell in r gives {NaN, +inf}."""
    for nx, ny in ((129, 5), (513, 9)):
        for align in ("fast", "odd_x0"):
            for num, den in COEFS:
                check_update(impl, tol_sum, nx, ny, align, num, den)
                check_dir(impl, nx, ny, align, num, den)
            for cell in ((0, 0), (ny - 1, nx - 1), (ny // 2, nx // 2)):
                check_update(impl, tol_sum, nx, ny, align, nan_cell=cell)


# ------------------------------------------------- empty regions and refusals
def run_empty_and_refusals(impl):
    """An empty region sets out to {0, 0} and touches no field; the refused calls, with their codes."""
    L = impl.lib
    p, q, f, (x0, nx, y0, ny) = apply_fields(5, 4, "fast", True)
    F, (sx0, snx, sy0, sny) = stream_fields("pqxr", UPDATE_ALIGN, 5, 4, "fast")
    d = Dev(impl, p=p, q=q, f=f)
    s = Dev(impl, **F)
    sh, (pn, pd) = _scalars(impl, 1.0, 2.0)
    st = impl.stream

    def apply(mode=0, x0=x0, nx=nx, y0=y0, ny=ny, pp=d.ptr("p"), ldp=p.ld, pf=d.ptr("f"), ldf=f.ld, pq=d.ptr("q"),
              ldq=q.ld, out=True, region=(x0, nx, y0, ny)):
        return _with_ws(impl, region, lambda o, w: L.gmt_cg_apply(mode, x0, nx, y0, ny, pp, ldp, pf, ldf, C0, C1, pq,
                                                                  ldq, o if out else None, w, st))

    def update(x0=sx0, nx=snx, y0=sy0, ny=sny, num=pn, den=pd, ptrs=None, lds=None, out=True):
        ptrs = dict({k: s.ptr(k) for k in "pqxr"}, **(ptrs or {}))
        lds = dict({k: s.ld(k) for k in "pqxr"}, **(lds or {}))
        return _with_ws(impl, (sx0, snx, sy0, sny), lambda o, w: L.gmt_cg_update(
            x0, nx, y0, ny, num, den, ptrs["p"], lds["p"], ptrs["q"], lds["q"], ptrs["x"], lds["x"], ptrs["r"],
            lds["r"], o if out else None, w, st))

    def dirc(x0=sx0, nx=snx, y0=sy0, ny=sny, num=pn, den=pd, pr=s.ptr("r"), ldr=s.ld("r"), pp=s.ptr("p"),
             ldp=s.ld("p")):
        return L.gmt_cg_dir(x0, nx, y0, ny, num, den, pr, ldr, pp, ldp, st)

    for enx, eny in ((0, 4), (5, 0), (0, 0)):
        assert apply(nx=enx, ny=eny) == (0, (0.0, 0.0))
        assert apply(mode=1, nx=enx, ny=eny) == (0, (0.0, 0.0))
        assert update(nx=enx, ny=eny) == (0, (0.0, 0.0))
        assert dirc(nx=enx, ny=eny) == 0
    codes = [
        apply(pp=None)[0], apply(pq=None)[0], apply(out=False)[0], apply(mode=2)[0], apply(mode=-1)[0],
        apply(x0=0)[0], apply(y0=0)[0], apply(ldp=x0 + nx)[0], apply(ldq=x0 + nx - 1)[0],
        apply(mode=1, ldf=x0 + nx - 1)[0],
        update(out=False)[0], update(num=None)[0], update(den=None)[0], update(x0=-1)[0], update(y0=-1)[0],
    ]
    for k in "pqxr":
        codes += [update(ptrs={k: None})[0], update(lds={k: sx0 + snx - 1})[0]]
    codes += [dirc(num=None), dirc(den=None), dirc(pr=None), dirc(pp=None), dirc(ldr=sx0 + snx - 1),
              dirc(ldp=sx0 + snx - 1), dirc(x0=-1), dirc(y0=-1)]
    assert apply(mode=0, pf=None, ldf=0)[0] == 0 and apply(mode=1, pf=None, ldf=0)[0] == 0  # f is optional
    assert apply(mode=0, ldf=0)[0] == 0                                                     # and ignored by mode 0
    # nothing was written by the empty or the refused calls
    before = {k: v.store.copy() for k, v in F.items()}
    s.fetch()
    assert all(same_bits(F[k].store, before[k]) for k in F)
    del sh
    return [int(c) for c in codes]


def host_impl(lib):
    from gpu_mpi_tests_amd import _native

    _native.bind(lib, [n for n in _native._SIGS if n.startswith("gmt_cg_")])
    return types.SimpleNamespace(lib=lib, stream=None, has_paths=False, upload=lambda a: a.copy(),
                                 download=lambda h: h.copy(), ptr=lambda h: h.ctypes.data)


def main():
    """Every check through the CPU backend; prints one JSON line."""
    impl = host_impl(ctypes.CDLL(sys.argv[1]))
    n = 0
    for nx in NXS:
        for mode, with_f in ((0, False), (1, False), (1, True)):
            run_apply_shapes(impl, 1e-12, nx, mode, with_f)
            n += 1
        run_stream_shapes(impl, 1e-12, nx)
    run_apply_nan(impl, 130, 9)
    run_coefs(impl, 1e-12)
    codes = run_empty_and_refusals(impl)
    p, q, _, region = apply_fields(100, 100, "fast", False)
    paths = [apply_path(impl, region, p, q)]
    F, reg = stream_fields("pqxr", UPDATE_ALIGN, 8, 2, "fast")
    d = Dev(impl, **F)
    paths.append(int(impl.lib.gmt_cg_update_path(reg[0], d.ptr("p"), 10, d.ptr("q"), 10, d.ptr("x"), 10, d.ptr("r"), 10)))
    paths.append(int(impl.lib.gmt_cg_dir_path(reg[0], d.ptr("r"), 10, d.ptr("p"), 10)))
    print(json.dumps(dict(ok=True, widths=n, codes=codes, paths=paths)))


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
