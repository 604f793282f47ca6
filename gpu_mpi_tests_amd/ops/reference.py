"""Plain-PyTorch fp64 reference implementations of every libgmt kernel.

These are (1) the CPU execution path of the ops (the gtensor ``host`` backend
analogue, reference ``CMakeLists.txt:59-69``) and (2) the numerics oracle the
GPU tests compare the HIP kernels against.  Summation orders match the HIP
kernels where it matters for bitwise distributed-vs-serial checks.
"""
from __future__ import annotations

import numpy as np
import torch

# 4th-order central first-derivative coefficients (mpi_stencil2d_gt.cc:75-76).
DERIV5 = (1.0 / 12.0, -2.0 / 3.0, 0.0, 2.0 / 3.0, -1.0 / 12.0)


def daxpy(a: float, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    y.copy_(a * x + y)
    return y


def stencil5_1d(inp: torch.Tensor, scale: float = 1.0, coef=DERIV5) -> torch.Tensor:
    n = inp.numel() - 4
    out = torch.zeros(n, dtype=inp.dtype, device=inp.device)
    for k in range(5):
        out += (coef[k] * scale) * inp[k : k + n]
    return out


def stencil5_2d(inp: torch.Tensor, dim: int, scale: float = 1.0, coef=DERIV5) -> torch.Tensor:
    """dim 0 = contiguous axis (tensor dim -1), dim 1 = strided axis (tensor dim 0)."""
    ny, nx = inp.shape
    if dim == 0:
        n = nx - 4
        out = torch.zeros(ny, n, dtype=inp.dtype, device=inp.device)
        for k in range(5):
            out += (coef[k] * scale) * inp[:, k : k + n]
    else:
        n = ny - 4
        out = torch.zeros(n, nx, dtype=inp.dtype, device=inp.device)
        for k in range(5):
            out += (coef[k] * scale) * inp[k : k + n, :]
    return out


def sum_axis(z: torch.Tensor, keep_dim: int) -> torch.Tensor:
    # keep_dim 0 keeps x (sum over rows), keep_dim 1 keeps y (sum over x).
    return z.sum(dim=0) if keep_dim == 0 else z.sum(dim=1)


def diff_sq(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    d = a - b
    return (d * d).sum()


def poly(mode: int, nx: int, ny: int, x0: float, dx: float, y0: float, dy: float,
         dtype=torch.float64, device="cpu") -> torch.Tensor:
    x = x0 + torch.arange(nx, dtype=torch.float64, device=device) * dx
    y = y0 + torch.arange(ny, dtype=torch.float64, device=device) * dy
    X = x.unsqueeze(0).expand(ny, nx)
    Y = y.unsqueeze(1).expand(ny, nx)
    if mode == 0:
        v = X * X * X + Y * Y
    elif mode == 1:
        v = 3 * X * X
    elif mode == 2:
        v = 2 * Y
    elif mode == 3:
        v = X.clone()  # linear ramp (DAXPY inputs), gmt_fill_poly mode 3
    else:
        raise ValueError(f"poly: mode {mode} (0-3 here; mode 4 is the engine's integer lattice)")
    return v.to(dtype)


def jacobi5(u: torch.Tensor, un: torch.Tensor, x0: int, nx: int, y0: int, ny: int,
            f: torch.Tensor | None = None, c0: float = 0.25, c1: float = 0.0) -> torch.Tensor | None:
    """Update un[y0:y0+ny, x0:x0+nx] from u; returns sum((un-u)^2) over the region."""
    if nx <= 0 or ny <= 0:
        return torch.zeros((), dtype=u.dtype, device=u.device)
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    w = u[ys, x0 - 1 : x0 - 1 + nx]
    e = u[ys, x0 + 1 : x0 + 1 + nx]
    n = u[y0 - 1 : y0 - 1 + ny, xs]
    s = u[y0 + 1 : y0 + 1 + ny, xs]
    o = c0 * ((w + e) + (n + s))
    if f is not None:
        o = o + c1 * f[ys, xs]
    d = o - u[ys, xs]
    un[ys, xs] = o
    return (d * d).sum()


def jacobi5_resid(u: torch.Tensor, x0: int, nx: int, y0: int, ny: int, f: torch.Tensor | None = None,
                  c0: float = 0.25, c1: float = 0.0) -> torch.Tensor:
    """(sum d^2, max |d| with NaN as +inf) of the Jacobi update over the region; u is not written."""
    if nx <= 0 or ny <= 0:
        return torch.zeros(2, dtype=u.dtype, device=u.device)
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    o = c0 * ((u[ys, x0 - 1 : x0 - 1 + nx] + u[ys, x0 + 1 : x0 + 1 + nx])
              + (u[y0 - 1 : y0 - 1 + ny, xs] + u[y0 + 1 : y0 + 1 + ny, xs]))
    if f is not None:
        o = o + c1 * f[ys, xs]
    d = o - u[ys, xs]
    return torch.stack(((d * d).sum(), d.abs().nan_to_num(nan=float("inf")).max()))


def _nan_inf_max(v: torch.Tensor) -> torch.Tensor:
    return v.abs().nan_to_num(nan=float("inf")).max()


def cg_apply(p: torch.Tensor, q: torch.Tensor, x0: int, nx: int, y0: int, ny: int, mode: int = 0,
             f: torch.Tensor | None = None, c0: float = 0.25, c1: float = 0.0) -> torch.Tensor:
    """gmt_cg_apply: q over the region, and (sum p*q, 0) (mode 0) or (sum q^2, max |q|) (mode 1)."""
    if mode not in (0, 1):
        raise ValueError(f"cg_apply: mode must be 0 or 1, got {mode!r}")
    if nx <= 0 or ny <= 0:
        return torch.zeros(2, dtype=p.dtype, device=p.device)
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    o = c0 * ((p[ys, x0 - 1 : x0 - 1 + nx] + p[ys, x0 + 1 : x0 + 1 + nx])
              + (p[y0 - 1 : y0 - 1 + ny, xs] + p[y0 + 1 : y0 + 1 + ny, xs]))
    c = p[ys, xs]
    if mode == 0:
        v = c - o
        q[ys, xs] = v
        return torch.stack(((c * v).sum(), torch.zeros((), dtype=p.dtype, device=p.device)))
    if f is not None:
        o = o + c1 * f[ys, xs]
    v = o - c
    q[ys, xs] = v
    return torch.stack(((v * v).sum(), _nan_inf_max(v)))


def _cg_coef(num: torch.Tensor, den: torch.Tensor) -> float:
    n, d = float(num.reshape(-1)[0]), float(den.reshape(-1)[0])
    return n / d if d > 0 else 0.0


def cg_update(num, den, p, q, x, r, x0: int, nx: int, y0: int, ny: int) -> torch.Tensor:
    """gmt_cg_update: x += a*p, r -= a*q over the region; (sum r^2, max |r|) of the new r."""
    if nx <= 0 or ny <= 0:
        return torch.zeros(2, dtype=x.dtype, device=x.device)
    a = _cg_coef(num, den)
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    x[ys, xs] = x[ys, xs] + a * p[ys, xs]
    v = r[ys, xs] - a * q[ys, xs]
    r[ys, xs] = v
    return torch.stack(((v * v).sum(), _nan_inf_max(v)))


def cg_dir(num, den, r, p, x0: int, nx: int, y0: int, ny: int) -> torch.Tensor:
    """gmt_cg_dir: p = r + b*p over the region."""
    if nx > 0 and ny > 0:
        b = _cg_coef(num, den)
        ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
        p[ys, xs] = r[ys, xs] + b * p[ys, xs]
    return p


def cheby_step(u: torch.Tensor, v: torch.Tensor, w: float, x0: int, nx: int, y0: int, ny: int,
               f: torch.Tensor | None = None, c0: float = 0.25, c1: float = 1.0) -> torch.Tensor:
    """gmt_cheby_step: v <- v + w*(G(u) - v) over the region, every operation rounded once."""
    if nx < 0 or ny < 0:
        raise ValueError("cheby_step: negative extent")
    if nx > 0 and ny > 0:
        ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
        o = c0 * ((u[ys, x0 - 1 : x0 - 1 + nx] + u[ys, x0 + 1 : x0 + 1 + nx])
                  + (u[y0 - 1 : y0 - 1 + ny, xs] + u[y0 + 1 : y0 + 1 + ny, xs]))
        if f is not None:
            o = o + c1 * f[ys, xs]
        pv = v[ys, xs]
        t = o - pv
        v[ys, xs] = pv + w * t
    return v


def mg_smooth(u, out, omega: float, x0: int, nx: int, y0: int, ny: int, f=None, c0: float = 0.25, c1: float = 1.0):
    """gmt_mg_smooth: out = u + omega*(G(u) - u) over the region, every operation
    rounded once.  Works on torch tensors and NumPy arrays alike."""
    if nx < 0 or ny < 0:
        raise ValueError("mg_smooth: negative extent")
    if nx > 0 and ny > 0:
        ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
        o = c0 * ((u[ys, x0 - 1 : x0 - 1 + nx] + u[ys, x0 + 1 : x0 + 1 + nx])
                  + (u[y0 - 1 : y0 - 1 + ny, xs] + u[y0 + 1 : y0 + 1 + ny, xs]))
        if f is not None:
            o = o + c1 * f[ys, xs]
        c = u[ys, xs]
        t = o - c
        out[ys, xs] = c + omega * t
    return out


MG_MAX_FUSE = 4
MG_HALO_W, MG_HALO_E, MG_HALO_S, MG_HALO_N = 1, 2, 4, 8


def mg_smooth_k(u, out, omega: float, x0: int, nx: int, y0: int, ny: int, k: int, halo_mask: int = 0, f=None,
                c0: float = 0.25, c1: float = 1.0):
    """gmt_mg_smooth_k: ``k`` applications of :func:`mg_smooth` over a copy of
    ``u``, the j-th on the region grown by ``k - j`` cells on every side whose
    bit is set in ``halo_mask`` (W = 1, E = 2, S = 4, N = 8) and by none on the
    others; every cell outside a box keeps its value.  ``out[region]`` gets the
    last one; no other cell of ``out`` is written.  Works on torch tensors and
    NumPy arrays alike."""
    if not 1 <= k <= MG_MAX_FUSE or not 0 <= halo_mask <= 15:
        raise ValueError("mg_smooth_k: k outside 1..4 or a mask outside 0..15")
    if nx < 0 or ny < 0:
        raise ValueError("mg_smooth_k: negative extent")
    if nx > 0 and ny > 0:
        a = u.clone() if hasattr(u, "clone") else u.copy()
        b = u.clone() if hasattr(u, "clone") else u.copy()
        for j in range(1, k + 1):
            g = k - j
            gw, ge = (g if halo_mask & MG_HALO_W else 0), (g if halo_mask & MG_HALO_E else 0)
            gs, gn = (g if halo_mask & MG_HALO_S else 0), (g if halo_mask & MG_HALO_N else 0)
            bx, by, bnx, bny = x0 - gw, y0 - gs, nx + gw + ge, ny + gs + gn
            mg_smooth(a, b, omega, bx, bnx, by, bny, f, c0, c1)
            a[by : by + bny, bx : bx + bnx] = b[by : by + bny, bx : bx + bnx]
        out[y0 : y0 + ny, x0 : x0 + nx] = a[y0 : y0 + ny, x0 : x0 + nx]
    return out


def mg_smooth_rb(u, out, omega: float, x0: int, nx: int, y0: int, ny: int, h: int, par: int, halo_mask: int = 0,
                 f=None, c0: float = 0.25, c1: float = 1.0):
    """gmt_mg_smooth_rb: ``h`` coloured half-sweeps over a copy of ``u``.  The
    j-th is :func:`mg_smooth` on the box of :func:`mg_smooth_k` (``h`` for
    ``k``), merged through the colour mask: cell (x, y) takes the new value iff
    ``(x - x0) + (y - y0) + par + (j - 1)`` is even and keeps its own otherwise.
    ``out[region]`` gets the last one.  Works on torch tensors and NumPy arrays
    alike."""
    if not 1 <= h <= MG_MAX_FUSE or not 0 <= halo_mask <= 15 or par not in (0, 1):
        raise ValueError("mg_smooth_rb: h outside 1..4, a mask outside 0..15 or par outside 0..1")
    if nx < 0 or ny < 0:
        raise ValueError("mg_smooth_rb: negative extent")
    if nx > 0 and ny > 0:
        tensor = hasattr(u, "clone")
        a = u.clone() if tensor else u.copy()
        b = u.clone() if tensor else u.copy()
        for j in range(1, h + 1):
            g = h - j
            gw, ge = (g if halo_mask & MG_HALO_W else 0), (g if halo_mask & MG_HALO_E else 0)
            gs, gn = (g if halo_mask & MG_HALO_S else 0), (g if halo_mask & MG_HALO_N else 0)
            bx, by, bnx, bny = x0 - gw, y0 - gs, nx + gw + ge, ny + gs + gn
            mg_smooth(a, b, omega, bx, bnx, by, bny, f, c0, c1)
            if tensor:
                import torch

                xs, ys = torch.arange(bx, bx + bnx), torch.arange(by, by + bny)
            else:
                import numpy as np

                xs, ys = np.arange(bx, bx + bnx), np.arange(by, by + bny)
            due = ((xs - x0)[None, :] + (ys - y0)[:, None] + (par + j - 1)) % 2 == 0  # % is the mathematical mod
            box = a[by : by + bny, bx : bx + bnx]
            box[due] = b[by : by + bny, bx : bx + bnx][due]
        out[y0 : y0 + ny, x0 : x0 + nx] = a[y0 : y0 + ny, x0 : x0 + nx]
    return out


def mg_coarse_extent(n: int, p: int) -> int:
    """Coarse cells of a fine region of n cells whose first coarse point has the region-relative index p."""
    return (n - p + 1) // 2


def mg_restrict(d, sc, cs: float, x0: int, nx: int, y0: int, ny: int, px: int, py: int, cx0: int, cy0: int):
    """gmt_mg_restrict: full weighting of d over the fine region into the
    ``mx x my`` coarse cells of sc at (cx0, cy0):
    ``cs*((H(y-1) + H(y+1)) + 2*H(y))``, ``H(r) = (d[r][x-1] + d[r][x+1]) + 2*d[r][x]``."""
    if nx < 0 or ny < 0 or px not in (0, 1) or py not in (0, 1):
        raise ValueError("mg_restrict: negative extent or a parity outside 0..1")
    mx, my = mg_coarse_extent(nx, px), mg_coarse_extent(ny, py)
    if nx > 0 and ny > 0 and mx > 0 and my > 0:
        xc, yc = x0 + px, y0 + py  # the first coarse point's fine cell

        def h(r):
            ys = slice(r, r + 2 * my - 1, 2)
            return (d[ys, xc - 1 : xc - 1 + 2 * mx - 1 : 2] + d[ys, xc + 1 : xc + 1 + 2 * mx - 1 : 2]) \
                + 2.0 * d[ys, xc : xc + 2 * mx - 1 : 2]

        sc[cy0 : cy0 + my, cx0 : cx0 + mx] = cs * ((h(yc - 1) + h(yc + 1)) + 2.0 * h(yc))
    return sc


def mg_resid_restrict(u, sc, cs: float, x0: int, nx: int, y0: int, ny: int, px: int, py: int, halo_mask: int = 0,
                      cx0: int = 0, cy0: int = 0, f=None, c0: float = 0.25, c1: float = 1.0):
    """gmt_mg_resid_restrict: :func:`cg_apply` mode 1 on the region grown by one
    cell on every side whose bit is set in ``halo_mask`` (W = 1, E = 2, S = 4,
    N = 8), into a zeroed scratch field, then :func:`mg_restrict` of that field
    over the region.  Works on torch tensors and NumPy arrays alike."""
    if not 0 <= halo_mask <= 15 or nx < 0 or ny < 0 or px not in (0, 1) or py not in (0, 1):
        raise ValueError("mg_resid_restrict: a mask outside 0..15, a negative extent or a parity outside 0..1")
    if nx > 0 and ny > 0:
        def t(a):
            return a if isinstance(a, torch.Tensor) else torch.from_numpy(a)

        gw, ge = int(bool(halo_mask & MG_HALO_W)), int(bool(halo_mask & MG_HALO_E))
        gs, gn = int(bool(halo_mask & MG_HALO_S)), int(bool(halo_mask & MG_HALO_N))
        d = torch.zeros_like(t(u))
        cg_apply(t(u), d, x0 - gw, nx + gw + ge, y0 - gs, ny + gs + gn, 1, None if f is None else t(f), c0, c1)
        mg_restrict(d, t(sc), cs, x0, nx, y0, ny, px, py, cx0, cy0)
    return sc


def mg_prolong_add(e, u, x0: int, nx: int, y0: int, ny: int, px: int, py: int, cx0: int, cy0: int):
    """gmt_mg_prolong_add: u += bilinear interpolation of the coarse field e over
    the fine region; by position: ``u + e``, ``u + 0.5*(eW + eE)``,
    ``u + 0.5*(eS + eN)``, ``u + 0.25*((eSW + eSE) + (eNW + eNE))``."""
    if nx < 0 or ny < 0 or px not in (0, 1) or py not in (0, 1):
        raise ValueError("mg_prolong_add: negative extent or a parity outside 0..1")
    if nx == 0 or ny == 0:
        return u

    def split(n, p, c0):
        """fine indices on a coarse point with their coarse index; fine indices between two with the lower one's"""
        on = list(range(p, n, 2))
        bt = list(range(1 - p, n, 2))
        return (on, [c0 + (i - p) // 2 for i in on]), (bt, [c0 + (i - p + 1) // 2 - 1 for i in bt])

    (xon, Xon), (xbt, Xbt) = split(nx, px, cx0)
    (yon, Yon), (ybt, Ybt) = split(ny, py, cy0)

    def sel(rows, cols):
        return (slice(rows[0], rows[-1] + 1, 2), slice(cols[0], cols[-1] + 1, 2)) if rows and cols else None

    def at(Y, X, dy=0, dx=0):
        return e[Y[0] + dy : Y[-1] + dy + 1, X[0] + dx : X[-1] + dx + 1]

    fy = lambda idx: [y0 + j for j in idx]  # noqa: E731
    fx = lambda idx: [x0 + i for i in idx]  # noqa: E731
    s = sel(fy(yon), fx(xon))
    if s:
        u[s] = u[s] + at(Yon, Xon)
    s = sel(fy(yon), fx(xbt))
    if s:
        u[s] = u[s] + 0.5 * (at(Yon, Xbt) + at(Yon, Xbt, 0, 1))
    s = sel(fy(ybt), fx(xon))
    if s:
        u[s] = u[s] + 0.5 * (at(Ybt, Xon) + at(Ybt, Xon, 1, 0))
    s = sel(fy(ybt), fx(xbt))
    if s:
        u[s] = u[s] + 0.25 * ((at(Ybt, Xbt) + at(Ybt, Xbt, 0, 1)) + (at(Ybt, Xbt, 1, 0) + at(Ybt, Xbt, 1, 1)))
    return u


def mg_prolong_smooth(e, u, out, omega: float, x0: int, nx: int, y0: int, ny: int, px: int, py: int, cx0: int,
                      cy0: int, h: int, rb: int = 0, par: int = 0, halo_mask: int = 0, f=None, c0: float = 0.25,
                      c1: float = 1.0):
    """gmt_mg_prolong_smooth: :func:`mg_prolong_add` over a copy of ``u`` on the
    region grown by ``h`` cells on every side whose bit is set in ``halo_mask``,
    then :func:`mg_smooth_k` (``rb = 0``) or :func:`mg_smooth_rb` (``rb = 1``)
    with ``h`` of that copy into ``out``.  The grown region starts ``g`` cells
    earlier, so its parity and first coarse cell move with it: every fine cell
    keeps its coarse column and row."""
    if not 1 <= h <= MG_MAX_FUSE or not 0 <= halo_mask <= 15 or rb not in (0, 1) or par not in (0, 1) \
            or px not in (0, 1) or py not in (0, 1):
        raise ValueError("mg_prolong_smooth: h, rb, par, px, py or the mask out of range")
    if nx < 0 or ny < 0:
        raise ValueError("mg_prolong_smooth: negative extent")
    if nx > 0 and ny > 0:
        v = u.clone() if hasattr(u, "clone") else u.copy()
        gw, ge = (h if halo_mask & MG_HALO_W else 0), (h if halo_mask & MG_HALO_E else 0)
        gs, gn = (h if halo_mask & MG_HALO_S else 0), (h if halo_mask & MG_HALO_N else 0)
        # the first coarse point at or after the grown region's first cell: parity p', coarse index (p' - g - p) / 2
        qx, qy = (px + gw) % 2, (py + gs) % 2
        mg_prolong_add(e, v, x0 - gw, nx + gw + ge, y0 - gs, ny + gs + gn, qx, qy,
                       cx0 + (qx - gw - px) // 2, cy0 + (qy - gs - py) // 2)
        if rb:
            mg_smooth_rb(v, out, omega, x0, nx, y0, ny, h, par, halo_mask, f, c0, c1)
        else:
            mg_smooth_k(v, out, omega, x0, nx, y0, ny, h, halo_mask, f, c0, c1)
    return out


def _np_view(a):
    """A NumPy view of a CPU tensor's storage (the array itself for NumPy)."""
    return a.numpy() if isinstance(a, torch.Tensor) else a


def mg_restrict_tab(d, sc, xaxis, yaxis, x0: int, y0: int, cx0: int, cy0: int):
    """gmt_mg_restrict_tab: ``sc = P^T d`` between two levels that are not
    nested.  ``xaxis`` / ``yaxis`` = ``(n, m, fo, fn, co, cn)``: the global
    fine and coarse point counts and the region's fine and coarse cells
    (mg_tab.region_tables).  Per coarse cell, over its 3 or 4 taps per axis:
    ``h_k = ((wx0*d0 + wx1*d1) + wx2*d2) [+ wx3*d3]`` per tapped row, then
    ``s = ((wy0*h0 + wy1*h1) + wy2*h2) [+ wy3*h3]``; only real taps are read."""
    from .. import mg_tab

    tx, ty = mg_tab.region_tables(*xaxis), mg_tab.region_tables(*yaxis)
    D, S = _np_view(d), _np_view(sc)
    mx, my = len(tx["rf"]), len(ty["rf"])
    if mx == 0 or my == 0 or int(xaxis[3]) == 0 or int(yaxis[3]) == 0:
        return sc
    if x0 < mg_tab.TAP_HALO or y0 < mg_tab.TAP_HALO or cx0 < 0 or cy0 < 0:
        raise ValueError("mg_restrict_tab: x0 and y0 >= 2, cx0 and cy0 >= 0")

    def gather(A, f, c, w, axis_first):
        """((w0*A0 + w1*A1) + w2*A2) [+ w3*A3] over the taps f .. f+c-1 of each coarse index."""
        take = (lambda i: A[i]) if axis_first else (lambda i: A[:, i])
        shape = (lambda v: v[:, None]) if axis_first else (lambda v: v[None, :])
        out = (shape(w[:, 0]) * take(f) + shape(w[:, 1]) * take(f + 1)) + shape(w[:, 2]) * take(f + 2)
        four = c == 4
        if four.any():
            t3 = shape(w[:, 3]) * take(f + np.where(four, 3, 2))  # a column with 3 taps re-reads its third
            out = np.where(shape(four), out + t3, out)
        return out

    r0, r1 = int(ty["rf"].min()), int((ty["rf"] + ty["rc"]).max())  # the tapped fine rows, region-relative
    H = gather(D[y0 + r0:y0 + r1], x0 + tx["rf"], tx["rc"], tx["rw"], False)
    S[cy0:cy0 + my, cx0:cx0 + mx] = gather(H, ty["rf"] - r0, ty["rc"], ty["rw"], True)
    return sc


def mg_prolong_add_tab(e, u, xaxis, yaxis, x0: int, y0: int, cx0: int, cy0: int):
    """gmt_mg_prolong_add_tab: ``u += P e``; axes as for :func:`mg_restrict_tab`.
    Per fine cell with ``(I, tx)`` of its column and ``(J, ty)`` of its row,
    ``w0 = 1.0 - t``: ``bot = w0x*e[J][I] + tx*e[J][I+1]``,
    ``top = w0x*e[J+1][I] + tx*e[J+1][I+1]``, ``v = w0y*bot + ty*top``, ``u = u + v``."""
    from .. import mg_tab

    tx, ty = mg_tab.region_tables(*xaxis), mg_tab.region_tables(*yaxis)
    E, U = _np_view(e), _np_view(u)
    nx, ny = len(tx["pq"]), len(ty["pq"])
    if nx == 0 or ny == 0:
        return u
    if x0 < 1 or y0 < 1 or cx0 < mg_tab.RING_HALO or cy0 < mg_tab.RING_HALO:
        raise ValueError("mg_prolong_add_tab: x0, y0, cx0 and cy0 >= 1")
    I, J = (cx0 + tx["pq"])[None, :], (cy0 + ty["pq"])[:, None]
    t1x, t1y = tx["pt"][None, :], ty["pt"][:, None]
    w0x, w0y = 1.0 - t1x, 1.0 - t1y
    bot = w0x * E[J, I] + t1x * E[J, I + 1]
    top = w0x * E[J + 1, I] + t1x * E[J + 1, I + 1]
    v = w0y * bot + t1y * top
    U[y0:y0 + ny, x0:x0 + nx] = U[y0:y0 + ny, x0:x0 + nx] + v
    return u


def jacobi5xk(k: int, u: torch.Tensor, un: torch.Tensor, rects, dom, halo_mask: int = 0) -> None:
    """fp64 reference of k fused Laplace sweeps with the ghost-side rule of
    csrc/kernels/jacobi5tb.hip: a ring cell outside ``dom`` gets an
    intermediate update only if its side's bit is set in ``halo_mask``."""
    dx0, dnx, dy0, dny = dom
    dx1, dy1 = dx0 + dnx, dy0 + dny
    for (x0, nx, y0, ny) in rects:
        cur = u[y0 - k:y0 + ny + k, x0 - k:x0 + nx + k].clone()
        for p in range(1, k + 1):
            r = k - p  # ring of this level
            xs = torch.arange(x0 - r, x0 + nx + r)
            ys = torch.arange(y0 - r, y0 + ny + r)
            sl = (slice(p, cur.shape[0] - p), slice(p, cur.shape[1] - p))
            upd = 0.25 * ((cur[p:-p, p - 1:cur.shape[1] - p - 1] + cur[p:-p, p + 1:cur.shape[1] - p + 1])
                          + (cur[p - 1:cur.shape[0] - p - 1, p:-p] + cur[p + 1:cur.shape[0] - p + 1, p:-p]))
            if p == k:
                un[y0:y0 + ny, x0:x0 + nx] = upd
                break
            rx = ((xs >= dx0) & (xs < dx1)) | torch.where(xs < dx0, bool(halo_mask & 1), bool(halo_mask & 2))
            ry = ((ys >= dy0) & (ys < dy1)) | torch.where(ys < dy0, bool(halo_mask & 4), bool(halo_mask & 8))
            nxt = cur.clone()
            nxt[sl] = torch.where(ry[:, None] & rx[None, :], upd, cur[sl])
            cur = nxt


