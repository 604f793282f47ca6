"""Cases, NumPy models and derived bounds of the Poisson source tests
(tests/test_source_cpu.py, tests/test_add2d_gpu.py, tests/test_source_gpu.py).

gmt_add2d cases are NumPy allocations with a region inside; a backend runs
them through ``run_add_cases(add, path)``.  As a program,
``source_cases.py <libgmt.so of the CPU backend>`` runs the add and fill cases
on that library (its SONAME is the GPU library's, so: in a child process) and
prints one JSON line.

Error bound of a fused source run against n exact (long double) single source
sweeps, derived, not measured.  u = 2^-53.  One sweep's three additions
contribute at most 2.01 u M (M: the largest |u| of the reference trajectory,
ring included), the source addition one more rounding, the multiplication by
1/4 is exact; the averaging map is non-expansive in the max norm, so per-sweep
errors add.  The Laplace part of a block is bitwise its single sweeps (the
fused kernel's guarantee).  The block field g costs at most 3.01 u per sweep
on |g| <= B S (B sweeps per block, S = max |s|), and adding it is one more
rounding: at most (5.02 B + 1) u (M + B S) per block.  ``bound`` is
6 (n + blocks) u (M + B S): that with margin."""
import ctypes
import functools
import json
import math
import os
import sys

import numpy as np

U = 2.0 ** -53
AMP = 2.0 ** -6
SEED = 11
PATH_NONE, PATH_SCALAR, PATH_PT = 0, 1, 2

# ---------------------------------------------------------------- gmt_add2d
# name: (rows, ldg, ld, y0, x0 in g, x0 in u, ny, nx, path on the GPU)
ADD_CASES = {
    "aligned": (70, 320, 320, 2, 8, 8, 67, 256, PATH_PT),
    "odd nx": (70, 320, 320, 2, 8, 8, 67, 257, PATH_PT),
    "nx 1": (70, 64, 64, 1, 4, 6, 67, 1, PATH_PT),
    "ny 1": (5, 320, 320, 3, 8, 10, 1, 257, PATH_PT),
    "ldg != ld": (40, 384, 292, 1, 2, 8, 33, 255, PATH_PT),
    "odd column offset": (40, 320, 320, 1, 8, 9, 33, 130, PATH_SCALAR),
    "odd offset in g": (40, 320, 320, 1, 7, 8, 33, 130, PATH_SCALAR),
    "odd pitch": (40, 320, 321, 1, 8, 8, 33, 257, PATH_SCALAR),
    "odd pitch of g": (40, 323, 320, 1, 8, 8, 3, 65, PATH_SCALAR),
    "empty nx": (8, 64, 64, 1, 8, 8, 4, 0, None),
    "empty ny": (8, 64, 64, 1, 8, 8, 0, 40, None),
}
# (ny, nx, ldg, ld): refused with code 1 on both backends, nothing written
ADD_REFUSED = [(-1, 8, 64, 64), (8, -1, 64, 64), (-2, -2, 64, 64), (4, 40, 39, 64), (4, 40, 64, 39), (4, 40, 0, 0)]
# more than 2^32 bytes between the first and the last row of the region
BIG_LD, BIG_LDG, BIG_NY, BIG_NX = (1 << 28) + 2, (1 << 28) + 6, 3, 5


def _values(rng, shape):
    return (rng.random(shape) - 0.5) * 2.0 ** rng.integers(-8, 9, shape)


def add_case(name):
    """g (NaN outside the region), u (sentinels outside) and the expected u."""
    rows, ldg, ld, y0, xg, xu, ny, nx, path = ADD_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    g = np.full((rows, ldg), np.nan)
    u = _values(rng, (rows, ld)) + 1000.0
    g[y0:y0 + ny, xg:xg + nx] = _values(rng, (ny, nx))
    want = u.copy()
    want[y0:y0 + ny, xu:xu + nx] = u[y0:y0 + ny, xu:xu + nx] + g[y0:y0 + ny, xg:xg + nx]
    return dict(g=g, u=u, want=want, gs=(slice(y0, y0 + ny), slice(xg, xg + nx)),
                us=(slice(y0, y0 + ny), slice(xu, xu + nx)), path=path, ny=ny, nx=nx)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


# --------------------------------------------------------------- fill modes
def lattice_uniform(gx, gy, seed):
    from gpu_mpi_tests_amd import engine

    return engine.lattice_uniform(gx, gy, seed)


def fill_model(mode, nx, ny, x0, dx, y0, dy):
    """NumPy model of gmt_fill_poly modes 6 and 7, bitwise."""
    ix = np.arange(nx, dtype=np.int64)[None, :]
    iy = np.arange(ny, dtype=np.int64)[:, None]
    if mode == 6:
        r = lattice_uniform(np.broadcast_to(int(x0) + ix, (ny, nx)), np.broadcast_to(int(y0) + iy, (ny, nx)), int(dx))
        return dy * (2.0 * r - 1.0)
    if mode == 7:
        x = (float(x0) + np.arange(nx, dtype=np.float64)) * dx
        return np.broadcast_to((-(1.5 * x + 0.5) * dx * dx)[None, :], (ny, nx)).copy()
    raise ValueError(mode)


# (mode, nx, ny, x0, dx, y0, dy)
FILL_CASES = [(6, 131, 9, -3.0, 12.0, 5.0, 0.25), (6, 64, 3, 1000.0, 2.0 ** 40 + 1, -7.0, 3.0),
              (7, 131, 9, -3.0, 1.0 / 301, 5.0, 1.0 / 301), (7, 70, 2, 40.0, 1.0 / 71, 0.0, 1.0 / 71)]


def check_fills(fill):
    """fill(mode, nx, ny, x0, dx, y0, dy) -> ndarray [ny][nx] of a backend."""
    for c in FILL_CASES:
        got, want = fill(*c), fill_model(*c)
        assert same_bits(got, want), (c, np.abs(got - want).max())
    # mode 6 is a function of the lattice point: a block at another offset of
    # the same lattice holds the same values (decomposition independence)
    whole = fill(6, 40, 30, -2.0, 9.0, -4.0, 0.5)
    part = fill(6, 17, 11, -2.0 + 13, 9.0, -4.0 + 8, 0.5)
    assert same_bits(whole[8:19, 13:30], part)
    assert whole.min() >= -0.5 and whole.max() < 0.5 and whole.std() > 0.2
    # mode 7 is the sweep source of mode 4's field: h^2/4 (6x + 2), negated
    h = 1.0 / 301
    s = fill(7, 50, 2, 0.0, h, 0.0, h)
    x = np.arange(50) * h
    assert np.allclose(s[1], -0.25 * h * h * (6 * x + 2), rtol=1e-14, atol=0)


# ------------------------------------------------- engine references, bounds
def host_source(ny, nx):
    """The random source of the fused-path tests: amplitude 2^-6, set through set_source."""
    return (np.random.default_rng(20240).random((ny, nx)) * 2.0 - 1.0) * AMP


def _wrap(u):
    u[1:-1, 0] = u[1:-1, -2]
    u[1:-1, -1] = u[1:-1, 1]
    u[0, 1:-1] = u[-2, 1:-1]
    u[-1, 1:-1] = u[1, 1:-1]


@functools.lru_cache(maxsize=8)
def ld_reference(ny, nx, periodic, counts, init="random", source="host"):
    """Long double single source sweeps: {n: interior after n sweeps} for n in
    counts, and M = the largest |u| the trajectory reaches (ring included)."""
    from gpu_mpi_tests_amd import engine

    LD = np.longdouble
    s = (host_source(ny, nx) if source == "host" else engine.source_field(ny, nx, source)).astype(LD)
    u = engine.initial_field(ny, nx, init, SEED).astype(LD)
    un = u.copy()
    out, big = {}, 0.0
    for n in range(max(counts) + 1):
        if periodic:
            _wrap(u)
        big = max(big, float(np.abs(u).max()))
        if n in counts:
            out[n] = u[1:-1, 1:-1].astype(np.float64)
        un[1:-1, 1:-1] = LD(0.25) * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1])) + s
        u, un = un, u
    return out, big


def bound(n, blocks, src_every, big, smax):
    return 6.0 * (n + blocks) * U * (big + src_every * smax)


def resid_with_source(u, s, periodic):
    """(L2, max) of d = J(u) + s - u over the interior of the ghosted float64 field u (fsum)."""
    if periodic:
        _wrap(u)
    d = (0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1])) + s) - u[1:-1, 1:-1]
    return math.sqrt(math.fsum((d * d).ravel().tolist())), float(np.abs(d).max())


@functools.lru_cache(maxsize=8)
def ref_series(ny, nx, periodic, sweeps):
    """{n: (L2, max)} of the float64 single source sweeps (random init SEED, host_source) at n in sweeps."""
    from gpu_mpi_tests_amd import engine

    s = host_source(ny, nx)
    u = engine.initial_field(ny, nx, "random", SEED)
    un = u.copy()
    out = {}
    for n in range(max(sweeps) + 1):
        if n in sweeps:
            out[n] = resid_with_source(u, s, periodic)
        if periodic:
            _wrap(u)
        un[1:-1, 1:-1] = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1])) + s
        u, un = un, u
    return out


def pick_tol(ny, nx, periodic, every, c, norm="l2"):
    """An absolute tol the reference series with the source first meets at
    check c: the geometric mean of its residuals at checks c - 1 and c, which
    must differ by more than 1e-6 relative so rounding cannot move the decision."""
    k = 0 if norm == "l2" else 1
    ser = ref_series(ny, nx, periodic, tuple(i * every for i in range(c + 1)))
    r = [ser[i * every][k] for i in range(c + 1)]
    assert r[c] < r[c - 1] * (1.0 - 1e-6), r
    assert all(r[i] > r[c - 1] for i in range(c - 1)), r
    return math.sqrt(r[c - 1] * r[c]), r


@functools.lru_cache(maxsize=2)
def converged_reference(n):
    """The NumPy iteration on the n x n Dirichlet problem (random init, host
    source) run until its own max |d| <= 1e-15 M: (interior, M, S).

    In float64 the iteration cannot get there: a mode that decays by
    1 - cos(pi / (n + 1)) a sweep stalls once that decay is below the rounding
    of a sweep, at max |d| of about 2^-53 / (1 - cos(pi / 65)) = 1e-13 (4.7e-14
    measured at n = 64).  So the float64 sweeps run until they stall and long
    double sweeps finish the job (their stall is 2000 times lower)."""
    from gpu_mpi_tests_amd import engine

    s = host_source(n, n)
    u = engine.initial_field(n, n, "random", SEED)
    big = float(np.abs(u).max())
    un = u.copy()
    last = np.inf
    for it in range(1, 400001):
        un[1:-1, 1:-1] = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1])) + s
        u, un = un, u
        if it % 500 == 0:
            big = max(big, float(np.abs(u).max()))  # M: the largest |u| on the way (sampled), ring included
            d = float(np.abs(u[1:-1, 1:-1] - un[1:-1, 1:-1]).max())
            if d <= 1e-15 * big or d > 0.5 * last:
                break
            last = d
    LD = np.longdouble
    u, s = u.astype(LD), s.astype(LD)
    un = u.copy()
    for it in range(1, 100001):
        un[1:-1, 1:-1] = LD(0.25) * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1])) + s
        u, un = un, u
        if it % 100 == 0 and float(np.abs(u[1:-1, 1:-1] - un[1:-1, 1:-1]).max()) <= 1e-15 * big:
            return u[1:-1, 1:-1].astype(np.float64), big, float(np.abs(s).max())
    raise AssertionError("the reference iteration did not converge")


# ------------------------------------------------- jobs of source_worker.py
# The fused configurations (the list of tests/test_solve_gpu.py): name, ranks, settings
FUSED = [
    ("one rank, local", 1, dict(ny=300, nx=700, tsteps=12, transport="local")),
    ("one rank, periodic, inline halo from graphs", 1,
     dict(ny=300, nx=700, tsteps=20, periodic=True, push=True, graph=True, transport="local")),
    ("2x1 periodic inline halo", 2, dict(ny=400, nx=900, tsteps=20, dims=(2, 1), periodic=True, push=True)),
    ("1x2 Dirichlet serial exchange from graphs", 2, dict(ny=300, nx=1200, tsteps=12, dims=(1, 2), graph=True)),
    ("2x2 band-first", 4, dict(ny=600, nx=1100, tsteps=20, dims=(2, 2), overlap=True)),
]


def fused_jobs(cfg, prefix):
    """Both block lengths of a fused configuration: run(2 * src_every + 3)."""
    ts = cfg["tsteps"]
    return [dict(cfg, kind="run", src_every=se, sweeps=2 * se + 3, save=f"{prefix}_{se}", zero=se == ts, late=se == ts)
            for se in (ts, 2 * ts)]


def baseline_jobs(cfg, prefix):
    """The one-rank engine of the same problem: plain passes, no graphs, no inline halo."""
    ts = cfg["tsteps"]
    base = dict(ny=cfg["ny"], nx=cfg["nx"], tsteps=ts, periodic=cfg.get("periodic", False), transport="local")
    return [dict(base, kind="run", src_every=se, sweeps=2 * se + 3, save=f"{prefix}_{se}") for se in (ts, 2 * ts)]


def check_fused(cfg, res, prefix, base_prefix, gpu):
    """Assertions 1-4 of a fused configuration on the worker's results and saved fields."""
    ny, nx, ts, periodic = cfg["ny"], cfg["nx"], cfg["tsteps"], bool(cfg.get("periodic", False))
    smax = float(np.abs(host_source(ny, nx)).max())
    ref, big = ld_reference(ny, nx, periodic, (2 * ts + 3, 4 * ts + 3))
    for r, se in zip(res, (ts, 2 * ts)):
        n = 2 * se + 3
        got, base = np.load(f"{prefix}_{se}.npy"), np.load(f"{base_prefix}_{se}.npy")
        tol = bound(n, 2, se, big, smax)
        diff = float(np.abs(got - ref[n]).max())
        print(f"src_every {se}: {n} sweeps, max|diff| vs long double {diff:.3e}, bound {tol:.3e} "
              f"(M {big:.4f}, S {smax:.5f}); bits equal to one rank: {same_bits(got, base)}")
        assert same_bits(got, base), (se, float(np.abs(got - base).max()))  # 1: decomposition independent
        assert diff <= tol, (se, diff, tol)  # 2
        assert r["source_plan"] == dict(blocks=2, src_every=se, tail=3), r  # 4: what ran
        assert r["src_every"] == se and r["tsteps"] == ts and r["plan"] == [ts] * (se // ts), r
        assert r["setup"]["sweeps"] == se and r["setup"]["max_abs"] == smax, r
        if cfg.get("push"):
            assert r["push"], r
        if cfg.get("graph") and gpu:
            assert r["graph"] and r["graph_fused"], r
        if se == ts:
            zero = np.load(f"{prefix}_{se}_zero.npy")
            seen = float(np.abs(zero - got).max())
            print(f"  source zeroed: max|diff| {seen:.3e}")
            assert seen > 1000.0 * tol, (seen, tol)  # 3: the test can see the term
            assert "already run" in r["late"], r


def check_resid(job, r, prefix):
    """residual_norm with a source: read-only, repeatable, equal to the NumPy residual that includes s."""
    ny, nx, periodic = job["ny"], job["nx"], bool(job.get("periodic", False))
    n1, n2 = job["pre"]
    assert r["unchanged"] and r["rn_same"], r
    assert r["rn"][0] == r["rn"][1], r["rn"]
    ser = ref_series(ny, nx, periodic, tuple(sorted({0, n1})))
    for got, s in ((r["rn"][0], 0), (r["rn"][2], n1)):
        print(f"residual after {s} sweeps: {got} reference {ser[s]}")
        for g, w in zip(got, ser[s]):
            assert abs(g - w) <= 1e-11 * max(1.0, w), (s, got, ser[s])
    # the later sweeps are the reference's: no stale ghost, parity unchanged
    se = r["src_every"]
    ref, big = ld_reference(ny, nx, periodic, (n1 + n2,))
    blocks = (n1 // se + n2 // se) if se else 0
    tol = bound(n1 + n2, blocks, se, big, float(np.abs(host_source(ny, nx)).max()))
    diff = float(np.abs(np.load(prefix + ".npy") - ref[n1 + n2]).max())
    print(f"field after {n1} + {n2} sweeps: max|diff| {diff:.3e}, bound {tol:.3e}")
    assert diff <= tol, (diff, tol)


def solve_job(cfg, every, c, lag, norm, save):
    tol, _ = pick_tol(cfg["ny"], cfg["nx"], bool(cfg.get("periodic", False)), every, c, norm)
    return dict(cfg, kind="solve", src_every=every, save=save,
                solve=dict(tol=tol, norm=norm, lag=lag, max_sweeps=12 * every, check_every=every))


def check_solve(job, got, every, c, lag, norm):
    """A solve whose tolerance the reference series with the source first meets at check c."""
    ny, nx, periodic = job["ny"], job["nx"], bool(job.get("periodic", False))
    res = got["res"]
    print(f"solve: {res}")
    assert got["same"], got
    assert res["converged"] == 1 and res["failed"] == 0, res
    assert res["residual_sweeps"] == c * every and res["sweeps"] == (c + lag) * every, res
    assert res["checks"] == c + lag + 1, res
    k = 0 if norm == "l2" else 1
    ser = ref_series(ny, nx, periodic, tuple(i * every for i in range(c + 1)))
    assert abs(res["residual"] - ser[c * every][k]) <= 1e-11 * max(1.0, ser[c * every][k]), (res, ser[c * every])
    assert abs(res["r0"] - ser[0][k]) <= 1e-11 * max(1.0, ser[0][k]), (res, ser[0])
    n = res["sweeps"]
    ref, big = ld_reference(ny, nx, periodic, (n,))
    tol = bound(n, n // every, every, big, float(np.abs(host_source(ny, nx)).max()))
    diff = float(np.abs(np.load(job["save"] + ".npy") - ref[n]).max())
    print(f"  field after {n} sweeps: max|diff| {diff:.3e}, bound {tol:.3e}")
    assert diff <= tol, (diff, tol)


N_CONV = 64  # the convergence case: 64 x 64 Dirichlet, tblock 4, blocks of 20 sweeps


def converge_job(save, **kw):
    return dict(ny=N_CONV, nx=N_CONV, tsteps=4, src_every=20, kind="solve", save=save,
                solve=dict(tol=1e-9, norm="max", lag=1, max_sweeps=40000, check_every=20), **kw)


def check_converged(job, got):
    """|u - u_ref| <= ||(I - A)^-1|| residual_max + the rounding bound: the
    comparison function 2 i (n + 1 - i) bounds the inverse's max norm by (n + 1)^2 / 2."""
    res = got["res"]
    assert res["converged"] == 1 and got["same"] and res["residual_max"] <= 1e-9, res
    uref, big, smax = converged_reference(N_CONV)
    n = res["sweeps"]
    tol = (N_CONV + 1) ** 2 / 2.0 * res["residual_max"] + bound(n, n // 20, 20, big, smax)
    diff = float(np.abs(np.load(job["save"] + ".npy") - uref).max())
    print(f"converged after {n} sweeps (residual max {res['residual_max']:.3e}): max|u - u_ref| {diff:.3e}, "
          f"bound {tol:.3e}")
    assert diff <= tol, (diff, tol)


SINGLE = dict(ny=40, nx=70, tsteps=1, kind="run", sweeps=7, transport="local")


def check_single(job, prefix):
    """The single-sweep source path: bitwise the float64 NumPy sweeps in the kernel's summation order."""
    from gpu_mpi_tests_amd import engine

    want = engine.serial_jacobi(job["ny"], job["nx"], job["sweeps"], bool(job.get("periodic", False)), init="random",
                                seed=SEED, source=host_source(job["ny"], job["nx"]))
    got = np.load(prefix + ".npy")
    assert same_bits(got, want), float(np.abs(got - want).max())


def check_fixed_point(r, prefix, n, src_every):
    """init 0 with the poly source, Dirichlet: x^3 + y^2 is the discrete fixed point."""
    from gpu_mpi_tests_amd import engine

    u0 = engine.initial_field(N_CONV, N_CONV)
    umax = float(np.abs(u0).max())
    # 16 ulps from the fill, the source and the sweep; x 4 margin
    print(f"fixed point: residual {r['rn0']}, allowed max {64 * U * umax:.3e}")
    assert r["rn0"][1] <= 64 * U * umax, r["rn0"]
    _, big = ld_reference(N_CONV, N_CONV, False, (n,), "analytic", "poly")
    smax = float(np.abs(engine.source_field(N_CONV, N_CONV, "poly")).max())
    tol = bound(n, n // src_every, src_every, big, smax)
    diff = float(np.abs(np.load(prefix + ".npy") - u0[1:-1, 1:-1]).max())
    print(f"  after {n} sweeps max|u - u0| {diff:.3e}, bound {tol:.3e}")
    assert diff <= tol, (diff, tol)


# ------------------------------------------------------------ host backend
def run_add_cases(add, path=None):
    """add(g_full, gs, u_full, us) runs gmt_add2d on the region views and
    returns (g_after, u_after) as full ndarrays; path(...) the same -> PATH_*
    of a backend that picks kernels, else None."""
    for name in ADD_CASES:
        c = add_case(name)
        g0 = c["g"].copy()
        if path is not None and c["path"] is not None:
            got = path(c["g"], c["gs"], c["u"], c["us"])
            assert got is None or got == c["path"], (name, got)
        g1, u1 = add(c["g"], c["gs"], c["u"], c["us"])
        assert same_bits(u1, c["want"]), (name, "u")
        assert same_bits(g1, g0), (name, "g was written")
    return len(ADD_CASES)


def _host_main(libpath):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gpu_mpi_tests_amd import _native

    lib = _native.bind(ctypes.CDLL(libpath), ["gmt_add2d", "gmt_add2d_path", "gmt_fill_poly"])

    def ptr(a, sl):
        return a.ctypes.data + (sl[0].start * a.shape[1] + sl[1].start) * 8

    def add(g, gs, u, us):
        ny, nx = us[0].stop - us[0].start, us[1].stop - us[1].start
        assert lib.gmt_add2d(nx, ny, ptr(g, gs), g.shape[1], ptr(u, us), u.shape[1], None) == 0
        return g, u

    def path(g, gs, u, us):
        # the CPU backend has no kernel to pick
        assert lib.gmt_add2d_path(us[1].stop - us[1].start, ptr(g, gs), g.shape[1], ptr(u, us), u.shape[1]) == PATH_NONE
        return None

    n = run_add_cases(add, path)
    codes = []
    for ny, nx, ldg, ld in ADD_REFUSED:
        g, u = np.full((8, 64), np.nan), np.ones((8, 64))
        codes.append(lib.gmt_add2d(nx, ny, g.ctypes.data, ldg, u.ctypes.data, ld, None))
        assert np.all(u == 1.0)
    u = np.ones((4, 8))
    codes.append(lib.gmt_add2d(4, 4, None, 8, u.ctypes.data, 8, None))
    codes.append(lib.gmt_add2d(4, 4, u.ctypes.data, 8, None, 8, None))
    # rows more than 2^32 bytes apart: untouched pages of the allocation cost nothing
    big = None
    try:
        ub = np.empty((BIG_NY - 1) * BIG_LD + BIG_NX + 2)
        gb = np.empty((BIG_NY - 1) * BIG_LDG + BIG_NX + 2)
    except MemoryError:
        ub = gb = None
    if ub is not None:
        rng = np.random.default_rng(5)
        want = []
        for j in range(BIG_NY):
            ub[j * BIG_LD:j * BIG_LD + BIG_NX + 2] = _values(rng, BIG_NX + 2)
            gb[j * BIG_LDG:j * BIG_LDG + BIG_NX + 2] = np.nan
            gb[j * BIG_LDG + 1:j * BIG_LDG + 1 + BIG_NX] = _values(rng, BIG_NX)
            w = ub[j * BIG_LD:j * BIG_LD + BIG_NX + 2].copy()
            w[1:-1] += gb[j * BIG_LDG + 1:j * BIG_LDG + 1 + BIG_NX]
            want.append(w)
        assert lib.gmt_add2d(BIG_NX, BIG_NY, gb.ctypes.data + 8, BIG_LDG, ub.ctypes.data + 8, BIG_LD, None) == 0
        big = all(same_bits(ub[j * BIG_LD:j * BIG_LD + BIG_NX + 2], want[j]) for j in range(BIG_NY))

    def fill(mode, nx, ny, x0, dx, y0, dy):
        z = np.full((ny, nx + 3), np.nan)
        assert lib.gmt_fill_poly(mode, nx, ny, x0, dx, y0, dy, z.ctypes.data, nx + 3, None) == 0
        assert np.isnan(z[:, nx:]).all()
        return z[:, :nx].copy()

    check_fills(fill)
    print(json.dumps(dict(ok=True, cases=n, refused=codes, big=big)))


if __name__ == "__main__":
    _host_main(sys.argv[1])
