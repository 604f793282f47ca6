"""Torch-facing wrappers of the libgmt gfx950 kernels.

Device tensors dispatch to the hand-written HIP kernels (``csrc/kernels``)
on the caller's current HIP stream; CPU tensors run the PyTorch reference
(``reference.py``).  There is no silent device fallback: if libgmt is
missing, device calls raise (see ``_native.lib``).

2-D fields follow ``gmt/kernels.h``: a tensor of shape ``[ny, nx]`` with
``stride(1) == 1`` (x contiguous = the reference's "dim 0"); ``stride(0)``
is the row pitch ``ld``, so views into padded / ghosted storage are accepted
without copies.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import torch

from .. import _native
from . import reference as ref
from .reference import DERIV5


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _is_dev(t: torch.Tensor) -> bool:
    return t.device.type == "cuda"


def _check2d(t: torch.Tensor, name: str):
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected a 2-D tensor with unit x-stride, got {tuple(t.shape)} "
                         f"strides {t.stride()}")
    if t.dtype != torch.float64:
        raise TypeError(f"{name}: kernels are fp64 (reference precision), got {t.dtype}")


class _Coef:
    """Keeps the ctypes array alive for the duration of the (synchronous) launch call."""

    def __init__(self, coef):
        self.arr = (ctypes.c_double * 5)(*[float(c) for c in coef])
        self.ptr = ctypes.cast(self.arr, ctypes.c_void_p)


# --------------------------------------------------------------------- DAXPY
def daxpy(a: float, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """In-place ``y <- a*x + y`` (fp64, contiguous).  K1/K2."""
    if x.numel() != y.numel():
        raise ValueError("daxpy: size mismatch")
    if not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("daxpy: contiguous vectors required (incx = incy = 1)")
    if not _is_dev(y):
        return ref.daxpy(a, x, y)
    L = _native.lib()
    _native.check(L.gmt_daxpy(y.numel(), float(a), x.data_ptr(), y.data_ptr(), _stream(y)),
                  "gmt_daxpy")
    return y


def _add2d_views(g: torch.Tensor, u: torch.Tensor):
    _check2d(g, "add2d.g")
    _check2d(u, "add2d.u")
    if tuple(g.shape) != tuple(u.shape):
        raise ValueError(f"add2d: shape mismatch {tuple(g.shape)} vs {tuple(u.shape)}")
    return u.shape[0], u.shape[1]


def add2d(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """In-place ``u += g`` over a 2-D fp64 region (views into padded storage
    welcome: each tensor's ``stride(0)`` is its row pitch), one rounding per
    cell; nothing outside the region is touched (gmt_add2d).  The add that
    ends a source block of the Jacobi engine."""
    ny, nx = _add2d_views(g, u)
    if not _is_dev(u):
        u += g
        return u
    _native.check(_native.lib().gmt_add2d(nx, ny, g.data_ptr(), g.stride(0), u.data_ptr(), u.stride(0),
                                          _stream(u)), "gmt_add2d")
    return u


def add2d_path(g: torch.Tensor, u: torch.Tensor) -> int:
    """The kernel :func:`add2d` would launch for these device tensors
    (gmt_add2d_path, no launch): PATH_PT (column pairs) or PATH_SCALAR."""
    _, nx = _add2d_views(g, u)
    return int(_native.lib().gmt_add2d_path(nx, g.data_ptr(), g.stride(0), u.data_ptr(), u.stride(0)))


# ------------------------------------------------------------ 5-tap stencils
def stencil5_1d(inp: torch.Tensor, out: torch.Tensor | None = None, scale: float = 1.0,
                coef=DERIV5) -> torch.Tensor:
    """``out[i] = scale * sum_k coef[k]*inp[i+k]``; len(out) = len(inp)-4.  K3."""
    n = inp.numel() - 4
    if not _is_dev(inp):
        r = ref.stencil5_1d(inp, scale, coef)
        if out is None:
            return r
        out.copy_(r)
        return out
    if out is None:
        out = torch.empty(n, dtype=inp.dtype, device=inp.device)
    assert inp.is_contiguous() and out.is_contiguous() and out.numel() == n
    L = _native.lib()
    cf = _Coef(coef)
    _native.check(L.gmt_stencil5_1d(n, cf.ptr, float(scale), inp.data_ptr(),
                                    out.data_ptr(), _stream(inp)), "gmt_stencil5_1d")
    return out


def stencil5_2d(inp: torch.Tensor, dim: int, out: torch.Tensor | None = None,
                scale: float = 1.0, coef=DERIV5) -> torch.Tensor:
    """5-tap stencil along ``dim`` (0 = contiguous x, 1 = strided y).  K4/K5."""
    _check2d(inp, "stencil5_2d.inp")
    ny_in, nx_in = inp.shape
    nx_out, ny_out = (nx_in - 4, ny_in) if dim == 0 else (nx_in, ny_in - 4)
    if not _is_dev(inp):
        r = ref.stencil5_2d(inp, dim, scale, coef)
        if out is None:
            return r
        out.copy_(r)
        return out
    if out is None:
        out = torch.empty(ny_out, nx_out, dtype=inp.dtype, device=inp.device)
    _check2d(out, "stencil5_2d.out")
    assert tuple(out.shape) == (ny_out, nx_out), (out.shape, ny_out, nx_out)
    L = _native.lib()
    cf = _Coef(coef)
    _native.check(L.gmt_stencil5_2d(dim, nx_out, ny_out, cf.ptr, float(scale),
                                    inp.data_ptr(), inp.stride(0), out.data_ptr(),
                                    out.stride(0), _stream(inp)), "gmt_stencil5_2d")
    return out


def stencil5_bands(n: int, sides: int) -> tuple[int, int]:
    """``(lo_w, hi_w)`` of the band rule (gmt/kernels.h): the edges of an output
    of extent ``n`` along the stencil's axis are ``[0, lo_w)`` and
    ``[n - hi_w, n)``, the interior is ``[lo_w, n - hi_w)``."""
    n = max(int(n), 0)
    lo_w = min(2, n) if sides & 1 else 0
    hi_w = min(2, n - lo_w) if sides & 2 else 0
    return lo_w, hi_w


def _stencil5_2d_part(name: str, inp, dim, out, sides, scale, coef):
    _check2d(inp, f"{name}.inp")
    _check2d(out, f"{name}.out")
    if dim not in (0, 1) or sides not in (0, 1, 2, 3):
        raise ValueError(f"{name}: dim must be 0 or 1 and sides 0..3, got dim {dim}, sides {sides}")
    ny_in, nx_in = inp.shape
    nx_out, ny_out = (nx_in - 4, ny_in) if dim == 0 else (nx_in, ny_in - 4)
    assert tuple(out.shape) == (ny_out, nx_out), (out.shape, ny_out, nx_out)
    if not _is_dev(inp):
        n = nx_out if dim == 0 else ny_out
        lo_w, hi_w = stencil5_bands(n, sides)
        spans = [(0, lo_w), (n - hi_w, n)] if name.endswith("edges") else [(lo_w, n - hi_w)]
        r = ref.stencil5_2d(inp, dim, scale, coef)
        for a, b in spans:
            if dim == 0:
                out[:, a:b] = r[:, a:b]
            else:
                out[a:b, :] = r[a:b, :]
        return out
    L = _native.lib()
    cf = _Coef(coef)
    fn = getattr(L, f"gmt_{name}")
    _native.check(fn(dim, nx_out, ny_out, cf.ptr, float(scale), inp.data_ptr(), inp.stride(0),
                     out.data_ptr(), out.stride(0), int(sides), _stream(inp)), f"gmt_{name}")
    return out


def stencil5_2d_edges(inp: torch.Tensor, dim: int, out: torch.Tensor, sides: int = 3,
                      scale: float = 1.0, coef=DERIV5) -> torch.Tensor:
    """The cells of :func:`stencil5_2d`'s output that read ghost cells: the
    2-deep bands at the low (``sides`` bit 0) and high (bit 1) end along
    ``dim``, both in one launch of the band kernel; no other cell of ``out``
    is written (:func:`stencil5_bands`)."""
    return _stencil5_2d_part("stencil5_2d_edges", inp, dim, out, sides, scale, coef)


def stencil5_2d_interior(inp: torch.Tensor, dim: int, out: torch.Tensor, sides: int = 3,
                         scale: float = 1.0, coef=DERIV5) -> torch.Tensor:
    """The complement of :func:`stencil5_2d_edges` for the same ``sides``, by
    the production kernels on the sub-rectangle between the bands."""
    return _stencil5_2d_part("stencil5_2d_interior", inp, dim, out, sides, scale, coef)


# gmt/kernels.h GMT_PATH_*: the kernel a launcher picks
PATH_NONE, PATH_SCALAR, PATH_PT, PATH_D1_WIN, PATH_D1_DMA, PATH_ROW_WALK = range(6)


def stencil5_2d_path(inp: torch.Tensor, dim: int, out: torch.Tensor) -> tuple[int, int]:
    """The kernel :func:`stencil5_2d` would launch for these device tensors
    (gmt_stencil5_2d_path, no launch): ``(PATH_*, rows per segment)``; the
    rows are 0 for the kernels that do not walk segments."""
    _check2d(inp, "stencil5_2d_path.inp")
    _check2d(out, "stencil5_2d_path.out")
    ny_out, nx_out = out.shape
    seg = ctypes.c_int64(0)
    path = _native.lib().gmt_stencil5_2d_path(int(dim), nx_out, ny_out, inp.data_ptr(), inp.stride(0),
                                              out.data_ptr(), out.stride(0),
                                              ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def jacobi5_path(u: torch.Tensor, un: torch.Tensor, region: tuple[int, int, int, int],
                 f: torch.Tensor | None = None) -> int:
    """The kernel :func:`jacobi5` would launch (gmt_jacobi5_path): PATH_PT or PATH_SCALAR."""
    return int(_native.lib().gmt_jacobi5_path(int(region[0]), u.data_ptr(), un.data_ptr(), u.stride(0),
                                              f.data_ptr() if f is not None else 0,
                                              f.stride(0) if f is not None else 0))


# ------------------------------------------------------- halo pack / unpack
def copy2d_batched(pairs: Sequence[tuple[torch.Tensor, torch.Tensor]], max_wgs: int = 0) -> None:
    """Copy each ``src`` 2-D view into ``dst`` (same shape) in ONE launch.  K6/K7/K8.
    max_wgs > 0: at most that many workgroups in a grid-stride loop (the
    exchange a band-first pass hides, Halo2D::set_pack_wgs)."""
    pairs = [(s, d) for s, d in pairs if s.numel() > 0]
    if not pairs:
        return
    if not _is_dev(pairs[0][1]):
        for s, d in pairs:
            d.copy_(s)
        return
    L = _native.lib()
    elem = pairs[0][0].element_size()
    stream = _stream(pairs[0][1])
    for i in range(0, len(pairs), _native.MAX_COPY2D):
        chunk = pairs[i : i + _native.MAX_COPY2D]
        arr = (_native.Copy2dDesc * len(chunk))()
        for k, (s, d) in enumerate(chunk):
            if s.dim() == 1:
                s = s.view(1, -1)
            if d.dim() == 1:
                d = d.view(1, -1)
            if tuple(s.shape) != tuple(d.shape):
                raise ValueError(f"copy2d: shape mismatch {tuple(s.shape)} vs {tuple(d.shape)}")
            if s.element_size() != elem or d.element_size() != elem:
                raise TypeError("copy2d: mixed element sizes")
            if (s.shape[1] > 1 and s.stride(1) != 1) or (d.shape[1] > 1 and d.stride(1) != 1):
                raise ValueError("copy2d: unit inner stride required")
            arr[k].src = s.data_ptr()
            arr[k].dst = d.data_ptr()
            arr[k].src_ld = s.stride(0)
            arr[k].dst_ld = d.stride(0)
            arr[k].width = s.shape[1]
            arr[k].height = s.shape[0]
        _native.check(L.gmt_copy2d_batched_wgs(len(chunk), ctypes.cast(arr, ctypes.c_void_p), elem,
                                               int(max_wgs), stream), "gmt_copy2d_batched_wgs")


# ---------------------------------------------------------------- reductions
def sum_axis(z: torch.Tensor, keep_dim: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Axis sums; keep_dim 0 -> length nx (sum over y), 1 -> length ny.  K9."""
    _check2d(z, "sum_axis.z")
    ny, nx = z.shape
    n_out = nx if keep_dim == 0 else ny
    if not _is_dev(z):
        r = ref.sum_axis(z, keep_dim)
        if out is None:
            return r
        out.copy_(r)
        return out
    if out is None:
        out = torch.empty(n_out, dtype=z.dtype, device=z.device)
    L = _native.lib()
    ws = torch.empty(max(1, L.gmt_sum_axis_workspace(keep_dim, nx, ny)), dtype=torch.float64,
                     device=z.device)
    _native.check(L.gmt_sum_axis(keep_dim, nx, ny, z.data_ptr(), z.stride(0), out.data_ptr(),
                                 ws.data_ptr(), _stream(z)), "gmt_sum_axis")
    return out


def vsum(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Sum of a contiguous fp64 vector into a 1-element tensor (one HBM pass,
    deterministic order): the DAXPY partial sums, mpi_daxpy_nvtx.cc:251-268."""
    if x.dtype != torch.float64 or not x.is_contiguous():
        raise ValueError("vsum: contiguous float64 vector required")
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=x.device)
    if not _is_dev(x):
        out.copy_(x.sum().reshape(1))
        return out
    L = _native.lib()
    n = x.numel()
    ws = torch.empty(max(1, L.gmt_sum_workspace(n)), dtype=torch.float64, device=x.device)
    _native.check(L.gmt_sum(n, x.data_ptr(), out.data_ptr(), ws.data_ptr(), _stream(x)), "gmt_sum")
    return out


def abs_max(z: torch.Tensor) -> torch.Tensor:
    """0-d tensor max |z| over a 2-D (or 1-D) fp64 tensor with unit x-stride."""
    if z.dim() == 1:
        z = z.view(1, -1)
    _check2d(z, "abs_max.z")
    if not _is_dev(z):
        return z.abs().max()
    ny, nx = z.shape
    L = _native.lib()
    ws = torch.empty(max(1, L.gmt_diff_sq_workspace(nx, ny)), dtype=torch.float64, device=z.device)
    out = torch.empty((), dtype=torch.float64, device=z.device)
    _native.check(L.gmt_abs_max(nx, ny, z.data_ptr(), z.stride(0), out.data_ptr(), ws.data_ptr(), _stream(z)),
                  "gmt_abs_max")
    return out


def diff_sq(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """0-d tensor ``sum((a-b)^2)`` (un-rooted so it can be all-reduced).  K10/K12."""
    if a.dim() == 1:
        a, b = a.view(1, -1), b.view(1, -1)
    _check2d(a, "diff_sq.a")
    _check2d(b, "diff_sq.b")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("diff_sq: shape mismatch")
    if not _is_dev(a):
        return ref.diff_sq(a, b)
    ny, nx = a.shape
    L = _native.lib()
    ws = torch.empty(max(1, L.gmt_diff_sq_workspace(nx, ny)), dtype=torch.float64, device=a.device)
    out = torch.empty((), dtype=torch.float64, device=a.device)
    _native.check(L.gmt_diff_sq(nx, ny, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0),
                                out.data_ptr(), ws.data_ptr(), _stream(a)), "gmt_diff_sq")
    return out


def diff_bits(a: torch.Tensor, b: torch.Tensor) -> tuple[float, int]:
    """Bitwise comparison of two 2-D fp64 regions (gmt_diff_bits): (max
    |a - b| with NaN as +inf, number of elements whose 64 bits differ)."""
    if a.dim() == 1:
        a, b = a.view(1, -1), b.view(1, -1)
    _check2d(a, "diff_bits.a")
    _check2d(b, "diff_bits.b")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("diff_bits: shape mismatch")
    if not _is_dev(a):
        ne = a.view(torch.int64) != b.view(torch.int64)
        d = (a - b).abs().nan_to_num(nan=float("inf"))[ne]
        return (float(d.max()) if d.numel() else 0.0), int(ne.sum())
    ny, nx = a.shape
    L = _native.lib()
    ws = torch.empty(max(2, 2 * L.gmt_diff_sq_workspace(nx, ny)), dtype=torch.float64, device=a.device)
    out = torch.empty(2, dtype=torch.float64, device=a.device)
    _native.check(L.gmt_diff_bits(nx, ny, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0),
                                  out.data_ptr(), ws.data_ptr(), _stream(a)), "gmt_diff_bits")
    o = out.cpu()
    return float(o[0]), int(o[1])


def xcd_of_workgroups(n: int, device: str = "cuda") -> list[int]:
    """The XCD each workgroup of one n-workgroup launch ran on (test hook of
    gmt_push_sync's per-XCD acquire)."""
    out = torch.zeros(n, dtype=torch.int32, device=device)
    _native.check(_native.lib().gmt_xcd_of_workgroups(int(n), out.data_ptr(),
                                                      torch.cuda.current_stream(out.device).cuda_stream),
                  "gmt_xcd_of_workgroups")
    return out.cpu().tolist()


def diff_norm(a: torch.Tensor, b: torch.Tensor) -> float:
    return float(diff_sq(a, b).sqrt())


# -------------------------------------------------------------- initialisers
def fill_poly(z: torch.Tensor, mode: int, x0: float, dx: float, y0: float, dy: float) -> torch.Tensor:
    """z = x^3 + y^2 (mode 0), 3x^2 (mode 1) or 2y (mode 2) on a uniform grid."""
    if z.dim() == 1:
        z2 = z.view(1, -1)
    else:
        z2 = z
    _check2d(z2, "fill_poly.z")
    ny, nx = z2.shape
    if not _is_dev(z):
        z2.copy_(ref.poly(mode, nx, ny, x0, dx, y0, dy, dtype=z.dtype))
        return z
    L = _native.lib()
    _native.check(L.gmt_fill_poly(mode, nx, ny, float(x0), float(dx), float(y0), float(dy),
                                  z2.data_ptr(), z2.stride(0), _stream(z)), "gmt_fill_poly")
    return z


# -------------------------------------------------------------------- Jacobi
def jacobi5(u: torch.Tensor, un: torch.Tensor, region: tuple[int, int, int, int],
            f: torch.Tensor | None = None, c0: float = 0.25, c1: float = 0.0,
            resid: bool = False) -> torch.Tensor | None:
    """One 5-point Jacobi sweep of ``region = (x0, nx, y0, ny)`` (absolute
    coordinates in the 2-D storage ``u``/``un``).  Returns the 0-d tensor
    ``sum((un-u)^2)`` over the region if ``resid``."""
    _check2d(u, "jacobi5.u")
    _check2d(un, "jacobi5.un")
    x0, nx, y0, ny = (int(v) for v in region)
    if not _is_dev(u):
        r = ref.jacobi5(u, un, x0, nx, y0, ny, f, c0, c1)
        return r if resid else None
    if u.stride(0) != un.stride(0):
        raise ValueError("jacobi5: u and un must share a row pitch")
    L = _native.lib()
    r = None
    rp = 0
    if resid:
        r = torch.empty(max(2, L.gmt_jacobi_resid_workspace(nx, ny)), dtype=torch.float64,
                        device=u.device)
        rp = r.data_ptr()
    _native.check(L.gmt_jacobi5(x0, nx, y0, ny, u.data_ptr(), un.data_ptr(), u.stride(0),
                                f.data_ptr() if f is not None else 0,
                                f.stride(0) if f is not None else 0, float(c0), float(c1), rp,
                                _stream(u)), "gmt_jacobi5")
    return r[0] if resid else None


def jacobi5_resid(u: torch.Tensor, region: tuple[int, int, int, int], f: torch.Tensor | None = None,
                  c0: float = 0.25, c1: float = 0.0) -> torch.Tensor:
    """Read-only residual of the Jacobi update over ``region = (x0, nx, y0, ny)``
    (gmt_jacobi5_resid; ``u`` is not written): the 2-element fp64 tensor
    ``(sum d^2, max |d|)`` on ``u``'s device, with
    ``d = c0*((W + E) + (N + S)) [+ c1*f] - u`` and a NaN ``d`` counted as
    ``+inf`` in the max."""
    _check2d(u, "jacobi5_resid.u")
    if f is not None:
        _check2d(f, "jacobi5_resid.f")
    x0, nx, y0, ny = (int(v) for v in region)
    if not _is_dev(u):
        return ref.jacobi5_resid(u, x0, nx, y0, ny, f, c0, c1)
    L = _native.lib()
    ws = torch.empty(max(2, L.gmt_jacobi5_resid_workspace(nx, ny)), dtype=torch.float64, device=u.device)
    out = torch.empty(2, dtype=torch.float64, device=u.device)
    _native.check(L.gmt_jacobi5_resid(x0, nx, y0, ny, u.data_ptr(), u.stride(0),
                                      f.data_ptr() if f is not None else 0,
                                      f.stride(0) if f is not None else 0, float(c0), float(c1),
                                      out.data_ptr(), ws.data_ptr(), _stream(u)), "gmt_jacobi5_resid")
    return out


def jacobi5_resid_path(u: torch.Tensor, region: tuple[int, int, int, int],
                       f: torch.Tensor | None = None) -> tuple[int, int]:
    """The kernel :func:`jacobi5_resid` would launch (gmt_jacobi5_resid_path, no
    launch): ``(PATH_ROW_WALK or PATH_SCALAR, rows per segment of the row walk)``."""
    x0, nx, _, ny = (int(v) for v in region)
    seg = ctypes.c_int64(0)
    path = _native.lib().gmt_jacobi5_resid_path(x0, nx, ny, u.data_ptr(), u.stride(0),
                                                f.data_ptr() if f is not None else 0,
                                                f.stride(0) if f is not None else 0,
                                                ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def _ptr_ld(t: "torch.Tensor | None") -> tuple[int, int]:
    return (t.data_ptr(), t.stride(0)) if t is not None else (0, 0)


def cg_apply(p: torch.Tensor, q: torch.Tensor, region: tuple[int, int, int, int], mode: int = 0,
             f: torch.Tensor | None = None, c0: float = 0.25, c1: float = 0.0) -> torch.Tensor:
    """The operator launch of a conjugate-gradient iteration over
    ``region = (x0, nx, y0, ny)`` (gmt_cg_apply), written to ``q``.
    mode 0: ``q = p - c0*((W + E) + (S + N))`` of ``p``, returns
    ``(sum p*q, 0)``; mode 1: ``q = c0*((W + E) + (S + N)) [+ c1*f] - p``
    (bitwise :func:`jacobi5_resid`'s d), returns ``(sum q^2, max |q|)`` with a
    NaN counted as ``+inf``.  No contraction: ``q`` is bitwise NumPy's."""
    _check2d(p, "cg_apply.p")
    _check2d(q, "cg_apply.q")
    if f is not None:
        _check2d(f, "cg_apply.f")
    x0, nx, y0, ny = (int(v) for v in region)
    if not _is_dev(p):
        return ref.cg_apply(p, q, x0, nx, y0, ny, mode, f, c0, c1)
    L = _native.lib()
    ws = torch.empty(max(2, L.gmt_cg_workspace(nx, ny)), dtype=torch.float64, device=p.device)
    out = torch.empty(2, dtype=torch.float64, device=p.device)
    _native.check(L.gmt_cg_apply(int(mode), x0, nx, y0, ny, p.data_ptr(), p.stride(0), *_ptr_ld(f), float(c0),
                                 float(c1), q.data_ptr(), q.stride(0), out.data_ptr(), ws.data_ptr(), _stream(p)),
                  "gmt_cg_apply")
    return out


def cg_update(num: torch.Tensor, den: torch.Tensor, p: torch.Tensor, q: torch.Tensor, x: torch.Tensor,
              r: torch.Tensor, region: tuple[int, int, int, int]) -> torch.Tensor:
    """``a = den > 0 ? num / den : 0`` from the one-element tensors ``num`` and
    ``den`` (read on the device); ``x += a*p``; ``r -= a*q`` over ``region``
    (gmt_cg_update).  Returns ``(sum r^2, max |r|)`` of the new ``r`` (NaN
    counted as ``+inf``)."""
    for t, n in ((p, "p"), (q, "q"), (x, "x"), (r, "r")):
        _check2d(t, "cg_update." + n)
    x0, nx, y0, ny = (int(v) for v in region)
    if not _is_dev(x):
        return ref.cg_update(num, den, p, q, x, r, x0, nx, y0, ny)
    L = _native.lib()
    ws = torch.empty(max(2, L.gmt_cg_workspace(nx, ny)), dtype=torch.float64, device=x.device)
    out = torch.empty(2, dtype=torch.float64, device=x.device)
    _native.check(L.gmt_cg_update(x0, nx, y0, ny, num.data_ptr(), den.data_ptr(), p.data_ptr(), p.stride(0),
                                  q.data_ptr(), q.stride(0), x.data_ptr(), x.stride(0), r.data_ptr(), r.stride(0),
                                  out.data_ptr(), ws.data_ptr(), _stream(x)), "gmt_cg_update")
    return out


def cg_dir(num: torch.Tensor, den: torch.Tensor, r: torch.Tensor, p: torch.Tensor,
           region: tuple[int, int, int, int]) -> torch.Tensor:
    """``b = den > 0 ? num / den : 0``; ``p = r + b*p`` over ``region``
    (gmt_cg_dir), in place; returns ``p``."""
    _check2d(r, "cg_dir.r")
    _check2d(p, "cg_dir.p")
    x0, nx, y0, ny = (int(v) for v in region)
    if not _is_dev(p):
        return ref.cg_dir(num, den, r, p, x0, nx, y0, ny)
    _native.check(_native.lib().gmt_cg_dir(x0, nx, y0, ny, num.data_ptr(), den.data_ptr(), r.data_ptr(),
                                           r.stride(0), p.data_ptr(), p.stride(0), _stream(p)), "gmt_cg_dir")
    return p


def cg_apply_path(p: torch.Tensor, q: torch.Tensor, region: tuple[int, int, int, int],
                  f: torch.Tensor | None = None) -> tuple[int, int]:
    """The kernel :func:`cg_apply` would launch (gmt_cg_apply_path, no launch):
    ``(PATH_ROW_WALK or PATH_SCALAR, rows per segment of the row walk)``."""
    x0, nx, _, ny = (int(v) for v in region)
    seg = ctypes.c_int64(0)
    path = _native.lib().gmt_cg_apply_path(x0, nx, ny, p.data_ptr(), p.stride(0), *_ptr_ld(f), q.data_ptr(),
                                           q.stride(0), ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def cg_update_path(p: torch.Tensor, q: torch.Tensor, x: torch.Tensor, r: torch.Tensor,
                   region: tuple[int, int, int, int]) -> int:
    """PATH_PT or PATH_SCALAR: the kernel :func:`cg_update` would launch (no launch)."""
    return int(_native.lib().gmt_cg_update_path(int(region[0]), p.data_ptr(), p.stride(0), q.data_ptr(), q.stride(0),
                                                x.data_ptr(), x.stride(0), r.data_ptr(), r.stride(0)))


def cg_dir_path(r: torch.Tensor, p: torch.Tensor, region: tuple[int, int, int, int]) -> int:
    """PATH_PT or PATH_SCALAR: the kernel :func:`cg_dir` would launch (no launch)."""
    return int(_native.lib().gmt_cg_dir_path(int(region[0]), r.data_ptr(), r.stride(0), p.data_ptr(), p.stride(0)))


def _storage_span(t: torch.Tensor) -> tuple[int, int]:
    """[first byte, one past the last byte) a 2-D view can touch."""
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    last = (t.shape[0] - 1) * t.stride(0) + (t.shape[1] - 1) * t.stride(1)
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def cheby_step(u: torch.Tensor, v: torch.Tensor, w: float, region: tuple[int, int, int, int],
               f: torch.Tensor | None = None, c0: float = 0.25, c1: float = 1.0) -> torch.Tensor:
    """One Chebyshev semi-iteration over ``region = (x0, nx, y0, ny)``
    (gmt_cheby_step): ``v <- v + w*(G(u) - v)`` with
    ``G(u) = c0*((W + E) + (S + N)) [+ c1*f]``; ``u`` is the current iterate,
    ``v`` the previous one, overwritten by the next.  No contraction: ``v`` is
    bitwise NumPy's (:func:`reference.cheby_step`).  ``u`` and ``v`` must not
    share storage.  Returns ``v``."""
    _check2d(u, "cheby_step.u")
    _check2d(v, "cheby_step.v")
    if f is not None:
        _check2d(f, "cheby_step.f")
    (ua, ub), (va, vb) = _storage_span(u), _storage_span(v)
    if ua < vb and va < ub:
        raise ValueError("cheby_step: u and v must not share storage")
    x0, nx, y0, ny = (int(t) for t in region)
    if not _is_dev(v):
        return ref.cheby_step(u, v, w, x0, nx, y0, ny, f, c0, c1)
    _native.check(_native.lib().gmt_cheby_step(x0, nx, y0, ny, u.data_ptr(), u.stride(0), *_ptr_ld(f), float(c0),
                                               float(c1), float(w), v.data_ptr(), v.stride(0), _stream(v)),
                  "gmt_cheby_step")
    return v


def cheby_step_path(u: torch.Tensor, v: torch.Tensor, region: tuple[int, int, int, int],
                    f: torch.Tensor | None = None) -> tuple[int, int]:
    """The kernel :func:`cheby_step` would launch (gmt_cheby_step_path, no
    launch): ``(PATH_ROW_WALK or PATH_SCALAR, rows per segment of the row walk)``."""
    x0, nx, _, ny = (int(t) for t in region)
    seg = ctypes.c_int64(0)
    path = _native.lib().gmt_cheby_step_path(x0, nx, ny, u.data_ptr(), u.stride(0), *_ptr_ld(f), v.data_ptr(),
                                             v.stride(0), ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    (aa, ab), (ba, bb) = _storage_span(a), _storage_span(b)
    return aa < bb and ba < ab


def mg_smooth(u: torch.Tensor, out: torch.Tensor, omega: float, region: tuple[int, int, int, int],
              f: torch.Tensor | None = None, c0: float = 0.25, c1: float = 1.0) -> torch.Tensor:
    """One damped Jacobi sweep of the multigrid cycle over
    ``region = (x0, nx, y0, ny)`` (gmt_mg_smooth):
    ``out = u + omega*(G(u) - u)``, ``G(u) = c0*((W + E) + (N + S)) [+ c1*f]``.
    No contraction: ``out`` is bitwise NumPy's (:func:`reference.mg_smooth`).
    ``u`` and ``out`` must not share storage.  Returns ``out``."""
    _check2d(u, "mg_smooth.u")
    _check2d(out, "mg_smooth.out")
    if f is not None:
        _check2d(f, "mg_smooth.f")
    if _overlap(u, out):
        raise ValueError("mg_smooth: u and out must not share storage")
    x0, nx, y0, ny = (int(t) for t in region)
    if not _is_dev(out):
        return ref.mg_smooth(u, out, omega, x0, nx, y0, ny, f, c0, c1)
    _native.check(_native.lib().gmt_mg_smooth(x0, nx, y0, ny, u.data_ptr(), u.stride(0), *_ptr_ld(f), float(c0),
                                              float(c1), float(omega), out.data_ptr(), out.stride(0), _stream(out)),
                  "gmt_mg_smooth")
    return out


def mg_smooth_path(u: torch.Tensor, out: torch.Tensor, region: tuple[int, int, int, int],
                   f: torch.Tensor | None = None) -> tuple[int, int]:
    """The kernel :func:`mg_smooth` would launch (gmt_mg_smooth_path, no launch):
    ``(PATH_ROW_WALK or PATH_SCALAR, rows per segment of the row walk)``."""
    x0, nx, _, ny = (int(t) for t in region)
    seg = ctypes.c_int64(0)
    path = _native.lib().gmt_mg_smooth_path(x0, nx, ny, u.data_ptr(), u.stride(0), *_ptr_ld(f), out.data_ptr(),
                                            out.stride(0), ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def mg_smooth_k(u: torch.Tensor, out: torch.Tensor, omega: float, region: tuple[int, int, int, int], k: int,
                halo_mask: int = 0, f: torch.Tensor | None = None, c0: float = 0.25, c1: float = 1.0) -> torch.Tensor:
    """``k`` (1..4) sweeps of :func:`mg_smooth` over ``region`` in one memory
    pass (gmt_mg_smooth_k).  ``halo_mask`` (W = 1, E = 2, S = 4, N = 8): a set
    bit marks a side whose ``k`` cells beyond the region are a neighbour's
    current cells and are updated along (on a box that shrinks by one cell per
    sweep); a clear bit a side whose one cell beyond the region is fixed.
    Bitwise :func:`reference.mg_smooth_k`.  ``u`` and ``out`` must not share
    storage.  Returns ``out``."""
    _check2d(u, "mg_smooth_k.u")
    _check2d(out, "mg_smooth_k.out")
    if f is not None:
        _check2d(f, "mg_smooth_k.f")
    if _overlap(u, out):
        raise ValueError("mg_smooth_k: u and out must not share storage")
    x0, nx, y0, ny = (int(t) for t in region)
    if not _is_dev(out):
        return ref.mg_smooth_k(u, out, omega, x0, nx, y0, ny, int(k), int(halo_mask), f, c0, c1)
    _native.check(_native.lib().gmt_mg_smooth_k(int(k), x0, nx, y0, ny, int(halo_mask), u.data_ptr(), u.stride(0),
                                                *_ptr_ld(f), float(c0), float(c1), float(omega), out.data_ptr(),
                                                out.stride(0), _stream(out)), "gmt_mg_smooth_k")
    return out


def mg_smooth_k_path(u: torch.Tensor, out: torch.Tensor, region: tuple[int, int, int, int], k: int,
                     halo_mask: int = 0, f: torch.Tensor | None = None) -> tuple[int, int]:
    """The kernel :func:`mg_smooth_k` would launch (gmt_mg_smooth_k_path, no
    launch): ``(PATH_ROW_WALK or PATH_SCALAR, output rows per segment of the fused walk)``."""
    x0, nx, _, ny = (int(t) for t in region)
    seg = ctypes.c_int64(0)
    path = _native.lib().gmt_mg_smooth_k_path(int(k), x0, nx, ny, int(halo_mask), u.data_ptr(), u.stride(0),
                                              *_ptr_ld(f), out.data_ptr(), out.stride(0),
                                              ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def mg_smooth_k_geom(k: int) -> tuple[int, int]:
    """``(output columns per wave, per workgroup)`` of the fused walk for ``k`` sweeps (gmt_mg_smooth_k_geom)."""
    wc, bc = ctypes.c_int64(0), ctypes.c_int64(0)
    if _native.lib().gmt_mg_smooth_k_geom(int(k), ctypes.cast(ctypes.pointer(wc), ctypes.c_void_p),
                                          ctypes.cast(ctypes.pointer(bc), ctypes.c_void_p)) != 0:
        raise ValueError(f"mg_smooth_k_geom: k = {k} outside 1..4")
    return int(wc.value), int(bc.value)


def mg_smooth_rb(u: torch.Tensor, out: torch.Tensor, omega: float, region: tuple[int, int, int, int], h: int,
                 par: int, halo_mask: int = 0, f: torch.Tensor | None = None, c0: float = 0.25,
                 c1: float = 1.0) -> torch.Tensor:
    """``h`` (1..4) coloured half-sweeps of red-black Gauss-Seidel over
    ``region`` in one memory pass (gmt_mg_smooth_rb): :func:`mg_smooth_k` with
    ``h`` for ``k``, where half-sweep ``j`` updates only the cells whose offset
    from the region's first cell has ``dx + dy + par + (j - 1)`` even.  Two
    half-sweeps are one red-black sweep.  Bitwise
    :func:`reference.mg_smooth_rb`.  ``u`` and ``out`` must not share storage.
    Returns ``out``."""
    _check2d(u, "mg_smooth_rb.u")
    _check2d(out, "mg_smooth_rb.out")
    if f is not None:
        _check2d(f, "mg_smooth_rb.f")
    if _overlap(u, out):
        raise ValueError("mg_smooth_rb: u and out must not share storage")
    x0, nx, y0, ny = (int(t) for t in region)
    if not _is_dev(out):
        return ref.mg_smooth_rb(u, out, omega, x0, nx, y0, ny, int(h), int(par), int(halo_mask), f, c0, c1)
    _native.check(_native.lib().gmt_mg_smooth_rb(int(h), int(par), x0, nx, y0, ny, int(halo_mask), u.data_ptr(),
                                                 u.stride(0), *_ptr_ld(f), float(c0), float(c1), float(omega),
                                                 out.data_ptr(), out.stride(0), _stream(out)), "gmt_mg_smooth_rb")
    return out


def mg_smooth_rb_path(u: torch.Tensor, out: torch.Tensor, region: tuple[int, int, int, int], h: int, par: int = 0,
                      halo_mask: int = 0, f: torch.Tensor | None = None) -> tuple[int, int]:
    """The kernel :func:`mg_smooth_rb` would launch (gmt_mg_smooth_rb_path, no
    launch): ``(PATH_ROW_WALK or PATH_SCALAR, output rows per segment of the walk)``."""
    x0, nx, _, ny = (int(t) for t in region)
    seg = ctypes.c_int64(0)
    path = _native.lib().gmt_mg_smooth_rb_path(int(h), int(par), x0, nx, ny, int(halo_mask), u.data_ptr(),
                                               u.stride(0), *_ptr_ld(f), out.data_ptr(), out.stride(0),
                                               ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def mg_restrict(d: torch.Tensor, sc: torch.Tensor, region: tuple[int, int, int, int], parity: tuple[int, int],
                coarse: tuple[int, int], cs: float = 0.25) -> torch.Tensor:
    """Full weighting of the fine field ``d`` over ``region = (x0, nx, y0, ny)``
    into the coarse field ``sc`` at ``coarse = (cx0, cy0)`` (gmt_mg_restrict).
    ``parity = (px, py)``: the region-relative fine index of the first coarse
    column / row.  Bitwise :func:`reference.mg_restrict`.  Returns ``sc``."""
    _check2d(d, "mg_restrict.d")
    _check2d(sc, "mg_restrict.sc")
    x0, nx, y0, ny = (int(t) for t in region)
    (px, py), (cx0, cy0) = (int(t) for t in parity), (int(t) for t in coarse)
    if not _is_dev(sc):
        return ref.mg_restrict(d, sc, cs, x0, nx, y0, ny, px, py, cx0, cy0)
    _native.check(_native.lib().gmt_mg_restrict(x0, nx, y0, ny, px, py, d.data_ptr(), d.stride(0), float(cs),
                                                sc.data_ptr(), cx0, cy0, sc.stride(0), _stream(sc)),
                  "gmt_mg_restrict")
    return sc


def mg_restrict_path(d: torch.Tensor, sc: torch.Tensor, region: tuple[int, int, int, int],
                     coarse: tuple[int, int]) -> int:
    """PATH_PT or PATH_SCALAR: the kernel :func:`mg_restrict` would launch (no launch)."""
    return int(_native.lib().gmt_mg_restrict_path(int(region[0]), int(coarse[0]), d.data_ptr(), d.stride(0),
                                                  sc.data_ptr(), sc.stride(0)))


def mg_resid_restrict(u: torch.Tensor, sc: torch.Tensor, region: tuple[int, int, int, int], parity: tuple[int, int],
                      coarse: tuple[int, int], halo_mask: int = 0, f: torch.Tensor | None = None, c0: float = 0.25,
                      c1: float = 1.0, cs: float = 0.25) -> torch.Tensor:
    """The residual of ``u`` and its full weighting into ``sc`` in one memory
    pass (gmt_mg_resid_restrict): :func:`cg_apply` mode 1 followed by
    :func:`mg_restrict` without the field between them.  ``halo_mask`` (W = 1,
    E = 2, S = 4, N = 8): a set bit marks a side whose 2 cells of ``u`` (1 of
    ``f``) beyond the region are a neighbour's current cells, so the ring of the
    residual is computed there; on a clear side it is zero and the one cell of
    ``u`` beyond the region is the fixed ring.  Bitwise
    :func:`reference.mg_resid_restrict`.  ``sc`` must not share storage with
    ``u`` or ``f``.  Returns ``sc``."""
    _check2d(u, "mg_resid_restrict.u")
    _check2d(sc, "mg_resid_restrict.sc")
    if f is not None:
        _check2d(f, "mg_resid_restrict.f")
    if _overlap(u, sc) or (f is not None and _overlap(f, sc)):
        raise ValueError("mg_resid_restrict: sc must not share storage with u or f")
    x0, nx, y0, ny = (int(t) for t in region)
    (px, py), (cx0, cy0) = (int(t) for t in parity), (int(t) for t in coarse)
    if not _is_dev(sc):
        return ref.mg_resid_restrict(u, sc, cs, x0, nx, y0, ny, px, py, int(halo_mask), cx0, cy0, f, c0, c1)
    _native.check(_native.lib().gmt_mg_resid_restrict(x0, nx, y0, ny, px, py, int(halo_mask), u.data_ptr(),
                                                      u.stride(0), *_ptr_ld(f), float(c0), float(c1), float(cs),
                                                      sc.data_ptr(), cx0, cy0, sc.stride(0), _stream(sc)),
                  "gmt_mg_resid_restrict")
    return sc


def mg_resid_restrict_path(u: torch.Tensor, sc: torch.Tensor, region: tuple[int, int, int, int],
                           parity: tuple[int, int], coarse: tuple[int, int], halo_mask: int = 0,
                           f: torch.Tensor | None = None) -> tuple[int, int]:
    """The kernel :func:`mg_resid_restrict` would launch (gmt_mg_resid_restrict_path,
    no launch): ``(PATH_ROW_WALK or PATH_SCALAR, fine rows per segment of the walk)``."""
    x0, nx, y0, ny = (int(t) for t in region)
    seg = ctypes.c_int64(0)
    path = _native.lib().gmt_mg_resid_restrict_path(x0, nx, y0, ny, int(parity[0]), int(parity[1]), int(halo_mask),
                                                    u.data_ptr(), u.stride(0), *_ptr_ld(f), sc.data_ptr(),
                                                    int(coarse[0]), int(coarse[1]), sc.stride(0),
                                                    ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def mg_resid_restrict_geom() -> tuple[int, int]:
    """``(fine columns per wave, per workgroup)`` of the fused transfer's walk (gmt_mg_resid_restrict_geom)."""
    wc, bc = ctypes.c_int64(0), ctypes.c_int64(0)
    _native.check(_native.lib().gmt_mg_resid_restrict_geom(ctypes.cast(ctypes.pointer(wc), ctypes.c_void_p),
                                                           ctypes.cast(ctypes.pointer(bc), ctypes.c_void_p)),
                  "gmt_mg_resid_restrict_geom")
    return int(wc.value), int(bc.value)


def mg_prolong_smooth(e: torch.Tensor, u: torch.Tensor, out: torch.Tensor, omega: float,
                      region: tuple[int, int, int, int], parity: tuple[int, int], coarse: tuple[int, int], h: int,
                      rb: int = 0, par: int = 0, halo_mask: int = 0, f: torch.Tensor | None = None, c0: float = 0.25,
                      c1: float = 1.0) -> torch.Tensor:
    """The interpolation ``u + P e`` and the first ``h`` (1..4) sweeps
    (``rb = 0``, :func:`mg_smooth_k`) or coloured half-sweeps (``rb = 1``,
    :func:`mg_smooth_rb` with ``par``) of the result in one memory pass
    (gmt_mg_prolong_smooth).  The correction is :func:`mg_prolong_add`'s cell
    rule on the region grown by ``h`` cells on every side whose bit is set in
    ``halo_mask``; the fixed ring of ``u`` enters as it is.  ``u`` and ``e`` are
    read only.  Bitwise :func:`reference.mg_prolong_smooth`.  ``out`` must not
    share storage with ``u``, ``e`` or ``f``.  Returns ``out``."""
    _check2d(e, "mg_prolong_smooth.e")
    _check2d(u, "mg_prolong_smooth.u")
    _check2d(out, "mg_prolong_smooth.out")
    if f is not None:
        _check2d(f, "mg_prolong_smooth.f")
    if _overlap(u, out) or _overlap(e, out) or (f is not None and _overlap(f, out)):
        raise ValueError("mg_prolong_smooth: out must not share storage with u, e or f")
    x0, nx, y0, ny = (int(t) for t in region)
    (px, py), (cx0, cy0) = (int(t) for t in parity), (int(t) for t in coarse)
    if not _is_dev(out):
        return ref.mg_prolong_smooth(e, u, out, omega, x0, nx, y0, ny, px, py, cx0, cy0, int(h), int(rb), int(par),
                                     int(halo_mask), f, c0, c1)
    _native.check(_native.lib().gmt_mg_prolong_smooth(int(h), int(rb), int(par), x0, nx, y0, ny, px, py,
                                                      int(halo_mask), e.data_ptr(), cx0, cy0, e.stride(0),
                                                      u.data_ptr(), u.stride(0), *_ptr_ld(f), float(c0), float(c1),
                                                      float(omega), out.data_ptr(), out.stride(0), _stream(out)),
                  "gmt_mg_prolong_smooth")
    return out


def mg_prolong_smooth_path(e: torch.Tensor, u: torch.Tensor, out: torch.Tensor, region: tuple[int, int, int, int],
                           parity: tuple[int, int], coarse: tuple[int, int], h: int, rb: int = 0, par: int = 0,
                           halo_mask: int = 0, f: torch.Tensor | None = None) -> tuple[int, int]:
    """The kernel :func:`mg_prolong_smooth` would launch (gmt_mg_prolong_smooth_path,
    no launch): ``(PATH_ROW_WALK or PATH_SCALAR, output rows per segment of the walk)``."""
    x0, nx, y0, ny = (int(t) for t in region)
    seg = ctypes.c_int64(0)
    path = _native.lib().gmt_mg_prolong_smooth_path(int(h), int(rb), int(par), x0, nx, y0, ny, int(parity[0]),
                                                    int(parity[1]), int(halo_mask), e.data_ptr(), int(coarse[0]),
                                                    int(coarse[1]), e.stride(0), u.data_ptr(), u.stride(0),
                                                    *_ptr_ld(f), out.data_ptr(), out.stride(0),
                                                    ctypes.cast(ctypes.pointer(seg), ctypes.c_void_p))
    return int(path), int(seg.value)


def mg_prolong_smooth_geom(h: int) -> tuple[int, int]:
    """``(output columns per wave, per workgroup)`` of the fused pass's walk (gmt_mg_prolong_smooth_geom)."""
    wc, bc = ctypes.c_int64(0), ctypes.c_int64(0)
    if _native.lib().gmt_mg_prolong_smooth_geom(int(h), ctypes.cast(ctypes.pointer(wc), ctypes.c_void_p),
                                                ctypes.cast(ctypes.pointer(bc), ctypes.c_void_p)) != 0:
        raise ValueError(f"mg_prolong_smooth_geom: h = {h} outside 1..4")
    return int(wc.value), int(bc.value)


def mg_prolong_add(e: torch.Tensor, u: torch.Tensor, region: tuple[int, int, int, int], parity: tuple[int, int],
                   coarse: tuple[int, int]) -> torch.Tensor:
    """``u += P e`` over the fine ``region = (x0, nx, y0, ny)``, P the bilinear
    interpolation from the coarse field ``e`` whose first cell of the region is
    at ``coarse = (cx0, cy0)`` (gmt_mg_prolong_add); ``parity`` as for
    :func:`mg_restrict`.  Bitwise :func:`reference.mg_prolong_add`.  ``e`` and
    ``u`` must not share storage.  Returns ``u``."""
    _check2d(e, "mg_prolong_add.e")
    _check2d(u, "mg_prolong_add.u")
    if _overlap(e, u):
        raise ValueError("mg_prolong_add: e and u must not share storage")
    x0, nx, y0, ny = (int(t) for t in region)
    (px, py), (cx0, cy0) = (int(t) for t in parity), (int(t) for t in coarse)
    if not _is_dev(u):
        return ref.mg_prolong_add(e, u, x0, nx, y0, ny, px, py, cx0, cy0)
    _native.check(_native.lib().gmt_mg_prolong_add(x0, nx, y0, ny, px, py, e.data_ptr(), cx0, cy0, e.stride(0),
                                                   u.data_ptr(), u.stride(0), _stream(u)), "gmt_mg_prolong_add")
    return u


def mg_prolong_add_path(e: torch.Tensor, u: torch.Tensor, region: tuple[int, int, int, int]) -> int:
    """PATH_PT or PATH_SCALAR: the kernel :func:`mg_prolong_add` would launch (no launch)."""
    return int(_native.lib().gmt_mg_prolong_add_path(int(region[0]), e.data_ptr(), e.stride(0), u.data_ptr(),
                                                     u.stride(0)))


class MgXferDesc(ctypes.Structure):
    """gmt_mg_xfer_desc (csrc/include/gmt/kernels.h): index 0 of each pair is x, 1 is y."""
    _fields_ = [(k, ctypes.c_int64 * 2) for k in ("n", "m", "fo", "fn", "co", "cn")]


class _XferPlan:
    """A gmt_mg_xfer_plan of one call: built and checked on the host, destroyed
    once the launch that used it has finished."""

    def __init__(self, xaxis, yaxis, what: str):
        d = MgXferDesc()
        for k, (vx, vy) in zip(("n", "m", "fo", "fn", "co", "cn"), zip(xaxis, yaxis)):
            getattr(d, k)[0], getattr(d, k)[1] = int(vx), int(vy)
        self.h = ctypes.c_void_p()
        if _native.lib().gmt_mg_xfer_plan_create(ctypes.byref(d), ctypes.byref(self.h)) or not self.h:
            raise ValueError(f"{what}: gmt_mg_xfer_plan_create refused the description {tuple(xaxis)}, {tuple(yaxis)}")

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _native.lib().gmt_mg_xfer_plan_destroy(self.h)


def mg_restrict_tab(d: torch.Tensor, sc: torch.Tensor, xaxis: tuple, yaxis: tuple, origin: tuple[int, int],
                    coarse: tuple[int, int]) -> torch.Tensor:
    """``sc = P^T d`` between two levels that are not nested
    (gmt_mg_restrict_tab): ``xaxis`` / ``yaxis`` = ``(n, m, fo, fn, co, cn)``,
    the global fine and coarse point counts of the axis and the region's fine
    cells ``fo+1 .. fo+fn`` and coarse cells ``co+1 .. co+cn``; the fine region
    sits at ``origin = (x0, y0)`` of ``d``, the coarse one at
    ``coarse = (cx0, cy0)`` of ``sc``.  The call builds its own plan
    (gmt_mg_xfer_plan_create checks every table index on the host); ValueError
    where that refuses.  Bitwise :func:`reference.mg_restrict_tab`.  Returns ``sc``."""
    _check2d(d, "mg_restrict_tab.d")
    _check2d(sc, "mg_restrict_tab.sc")
    (x0, y0), (cx0, cy0) = (int(t) for t in origin), (int(t) for t in coarse)
    if not _is_dev(sc):
        return ref.mg_restrict_tab(d, sc, xaxis, yaxis, x0, y0, cx0, cy0)
    with _XferPlan(xaxis, yaxis, "mg_restrict_tab") as plan:
        _native.check(_native.lib().gmt_mg_restrict_tab(plan, x0, y0, d.data_ptr(), d.stride(0), sc.data_ptr(), cx0,
                                                        cy0, sc.stride(0), _stream(sc)), "gmt_mg_restrict_tab")
    return sc


def mg_restrict_tab_path(d: torch.Tensor, sc: torch.Tensor, origin: tuple[int, int], coarse: tuple[int, int]) -> int:
    """PATH_PT or PATH_SCALAR: the kernel :func:`mg_restrict_tab` would launch (no launch)."""
    return int(_native.lib().gmt_mg_restrict_tab_path(int(origin[0]), int(coarse[0]), d.data_ptr(), d.stride(0),
                                                      sc.data_ptr(), sc.stride(0)))


def mg_prolong_add_tab(e: torch.Tensor, u: torch.Tensor, xaxis: tuple, yaxis: tuple, origin: tuple[int, int],
                       coarse: tuple[int, int]) -> torch.Tensor:
    """``u += P e``, P linear interpolation between two levels that are not
    nested (gmt_mg_prolong_add_tab); arguments as for :func:`mg_restrict_tab`
    with ``e`` the coarse field.  Bitwise :func:`reference.mg_prolong_add_tab`.
    ``e`` and ``u`` must not share storage.  Returns ``u``."""
    _check2d(e, "mg_prolong_add_tab.e")
    _check2d(u, "mg_prolong_add_tab.u")
    if _overlap(e, u):
        raise ValueError("mg_prolong_add_tab: e and u must not share storage")
    (x0, y0), (cx0, cy0) = (int(t) for t in origin), (int(t) for t in coarse)
    if not _is_dev(u):
        return ref.mg_prolong_add_tab(e, u, xaxis, yaxis, x0, y0, cx0, cy0)
    with _XferPlan(xaxis, yaxis, "mg_prolong_add_tab") as plan:
        _native.check(_native.lib().gmt_mg_prolong_add_tab(plan, x0, y0, e.data_ptr(), cx0, cy0, e.stride(0),
                                                           u.data_ptr(), u.stride(0), _stream(u)),
                      "gmt_mg_prolong_add_tab")
    return u


def mg_prolong_add_tab_path(e: torch.Tensor, u: torch.Tensor, origin: tuple[int, int]) -> int:
    """PATH_PT or PATH_SCALAR: the kernel :func:`mg_prolong_add_tab` would launch (no launch)."""
    return int(_native.lib().gmt_mg_prolong_add_tab_path(int(origin[0]), e.data_ptr(), e.stride(0), u.data_ptr(),
                                                         u.stride(0)))


def jacobi5_rects(u: torch.Tensor, un: torch.Tensor, rects: Sequence[tuple[int, int, int, int]],
                  f: torch.Tensor | None = None, c0: float = 0.25, c1: float = 0.0) -> None:
    """Sweep up to 4 rectangles (the boundary frame of an overlapped step) in one launch."""
    rects = [tuple(int(v) for v in r) for r in rects if r[1] > 0 and r[3] > 0]
    if not rects:
        return
    if not _is_dev(u):
        for (x0, nx, y0, ny) in rects:
            ref.jacobi5(u, un, x0, nx, y0, ny, f, c0, c1)
        return
    assert len(rects) <= 4
    L = _native.lib()
    arr = (ctypes.c_int64 * (4 * len(rects)))(*[v for r in rects for v in r])
    _native.check(L.gmt_jacobi5_rects(len(rects), ctypes.cast(arr, ctypes.c_void_p),
                                      u.data_ptr(), un.data_ptr(), u.stride(0),
                                      f.data_ptr() if f is not None else 0,
                                      f.stride(0) if f is not None else 0, float(c0), float(c1),
                                      _stream(u)), "gmt_jacobi5_rects")


TB_MAX_SWEEPS = 20  # GMT_TB_MAX_SWEEPS (csrc/include/gmt/kernels.h)


def tb_supported(k: int) -> bool:
    """Sweep counts the temporal-blocking kernel is built for: 1..10 (one wave
    per strip) and even 12..20 (two waves per strip, levels split)."""
    return 1 <= k <= 10 or (10 < k <= TB_MAX_SWEEPS and k % 2 == 0)


def _check_xk_bounds(k: int, u: torch.Tensor, un: torch.Tensor, rects) -> None:
    """Host-side guard before a K-sweep launch: the kernel reads each rect plus a
    K-wide ring, so both tensors must be whole row-major fp64 arrays holding
    that ring."""
    if u.dim() != 2 or u.shape != un.shape or not (u.is_contiguous() and un.is_contiguous()):
        raise ValueError("jacobi5tb: u and un must be contiguous 2-D tensors of one shape")
    if u.dtype != torch.float64 or un.dtype != torch.float64:
        raise ValueError("jacobi5tb: fp64 only")
    rows, cols = u.shape
    for x0, nx, y0, ny in rects:
        if x0 - k < 0 or y0 - k < 0 or x0 + nx + k > cols or y0 + ny + k > rows:
            raise ValueError(f"jacobi5tb: rect {(x0, nx, y0, ny)} with its {k}-cell ring does not fit "
                             f"a {rows}x{cols} array")


def jacobi5tb(k: int, u: torch.Tensor, un: torch.Tensor, rects: Sequence[tuple[int, int, int, int]],
              dom: tuple[int, int, int, int], halo_mask: int = 0, *, wg_waves: int = 0, seg_rows: int = 0,
              exact: bool = False, push: "dict | None" = None, push_w: int = 0, shared: int = 0) -> None:
    """``k`` fused Laplace sweeps per memory pass with the temporal-blocking kernel
    (csrc/kernels/jacobi5tb.hip): ``un = J^k(u)`` on up to 8 output rects (absolute
    coordinates, each with its k-wide ring inside the array); the rest of ``un``
    is never written.  ``dom`` is the interior; bits of ``halo_mask`` (1 W, 2 E,
    4 S, 8 N) mark ghost sides owned by a neighbour (the others are fixed
    Dirichlet rings).  ``k``: see :func:`tb_supported`.  ``wg_waves``: 256-column
    strips per workgroup (0 = default), ``seg_rows``: output rows per strip (0 =
    default), ``exact``: 1/4 multiply per level instead of power-of-two scaled
    levels.  ``push`` ({direction: tensor}, directions "S" "N" "W" "E" "SW" "SE"
    "NW" "NE") with ``push_w``: the inline halo exchange (gmt_tb_opts.push) —
    the output's face cells are also stored into each tensor at the same
    coordinates (a tensor with ``un``'s row pitch).  ``shared``: the shared hand-off
    group launch (gmt_tb_opts.shared: 1 / 4 on with four-strip groups, 2 with
    two-strip groups, -1 off, 0 default = on where it applies; a push pass takes
    groups only when asked for, see :func:`jacobi5tb_shared_path`)."""
    rects = [tuple(int(v) for v in r) for r in rects if r[1] > 0 and r[3] > 0]
    if not tb_supported(k):
        raise ValueError(f"jacobi5tb: {k} sweeps per pass is not built (1..10 or even 12..{TB_MAX_SWEEPS})")
    if not rects:
        return
    if len(rects) > 8:
        raise ValueError("jacobi5tb: at most 8 rects per launch")
    if not _is_dev(u):
        ref.jacobi5xk(k, u, un, rects, dom, halo_mask)
        return
    if u.stride(0) != un.stride(0):
        raise ValueError("jacobi5tb: u and un must share a row pitch")
    _check_xk_bounds(k, u, un, rects)
    L = _native.lib()
    arr = (ctypes.c_int64 * (4 * len(rects)))(*[v for r in rects for v in r])
    d = (ctypes.c_int64 * 4)(*[int(v) for v in dom])
    o = _native.TbOpts(int(k), int(wg_waves), int(seg_rows), int(bool(exact)))
    o.shared = int(shared)
    if push:
        order = ("S", "N", "W", "E", "SW", "SE", "NW", "NE")
        for dirn, t in push.items():
            if t.stride(0) != un.stride(0) or t.shape[0] < un.shape[0] or t.dtype != un.dtype:
                raise ValueError("jacobi5tb: a push target needs un's row pitch, rows and dtype")
            o.push[order.index(dirn)] = t.data_ptr()
        o.push_w = int(push_w)
    _native.check(L.gmt_jacobi5tb(ctypes.byref(o), len(rects), ctypes.cast(arr, ctypes.c_void_p),
                                  ctypes.cast(d, ctypes.c_void_p), int(halo_mask), u.data_ptr(),
                                  un.data_ptr(), u.stride(0), u.shape[0], _stream(u)),
                  "gmt_jacobi5tb")


def jacobi5tb_plan(k: int, rects: Sequence[tuple[int, int, int, int]], dom: tuple[int, int, int, int],
                   halo_mask: int, ld: int, nrows: int, *, wg_waves: int = 0, seg_rows: int = 0,
                   shared: int = 0, push: "dict | None" = None, push_w: int = 0) -> dict:
    """The launch :func:`jacobi5tb` would make (gmt_jacobi5tb_plan), without
    launching: workgroups, resident workgroups, threads per workgroup (512 for
    a four-strip shared hand-off group launch), interior segment rows and
    count, VGPRs.  ``push`` / ``push_w``: as in :func:`jacobi5tb` (only which
    directions are pushed matters: a value may be a tensor or anything true)."""
    L = _native.lib()
    rects = [tuple(int(v) for v in r) for r in rects]
    arr = (ctypes.c_int64 * (4 * len(rects)))(*[v for r in rects for v in r])
    d = (ctypes.c_int64 * 4)(*[int(v) for v in dom])
    o = _native.TbOpts(int(k), int(wg_waves), int(seg_rows), 0)
    o.shared = int(shared)
    if push:
        for dirn, t in push.items():
            if t is not None and t is not False:
                # (nothing is dereferenced: any aligned non-null address)
                o.push[_PUSH_DIRS.index(dirn)] = t.data_ptr() if isinstance(t, torch.Tensor) else 8
        o.push_w = int(push_w)
    info = (ctypes.c_int64 * 6)()
    _native.check(L.gmt_jacobi5tb_plan(ctypes.byref(o), len(rects), ctypes.cast(arr, ctypes.c_void_p),
                                       ctypes.cast(d, ctypes.c_void_p), int(halo_mask), int(ld), int(nrows),
                                       ctypes.cast(info, ctypes.c_void_p)), "gmt_jacobi5tb_plan")
    keys = ("workgroups", "resident", "threads", "seg_rows", "segments", "vgprs")
    return dict(zip(keys, (int(v) for v in info)))


_PUSH_DIRS = ("S", "N", "W", "E", "SW", "SE", "NW", "NE")


def jacobi5tb_shared_path(k: int, rects: Sequence[tuple[int, int, int, int]], halo_mask: int, *, shared: int = 0,
                          wg_waves: int = 0, push_w: int = 0) -> int:
    """Strips per shared hand-off group (2 or 4) that :func:`jacobi5tb` would
    launch for these arguments, 0 for a per-strip launch
    (gmt_jacobi5tb_shared_path: the launcher's own decision, nothing is
    launched).  ``push_w`` > 0: an inline-halo pass, which takes groups only
    when ``shared`` (or GMT_TB_SHARED) asks for them and a push-group kernel
    is built (:func:`tb_push_shared_supported`)."""
    rects = [tuple(int(v) for v in r) for r in rects]
    arr = (ctypes.c_int64 * max(4, 4 * len(rects)))(*[v for r in rects for v in r])
    o = _native.TbOpts(int(k), int(wg_waves), 0, 0)
    o.shared = int(shared)
    o.push_w = int(push_w)
    return int(_native.lib().gmt_jacobi5tb_shared_path(ctypes.byref(o), len(rects), ctypes.cast(arr, ctypes.c_void_p),
                                                       int(halo_mask)))


def tb_push_shared_supported(k: int, strips: int) -> bool:
    """An inline-halo (push) kernel in shared hand-off groups of ``strips``
    strips is built for ``k`` sweeps (gmt_jacobi5tb_push_shared_supported)."""
    return bool(_native.lib().gmt_jacobi5tb_push_shared_supported(int(k), int(strips)))


def jacobi5tb_shared_geom(k: int, strips: int = 4) -> dict:
    """Column geometry of the shared hand-off group kernel for ``k`` sweeps and
    ``strips`` (2 or 4) per group (gmt_jacobi5tb_shared_geom, the kernel's own
    constants): GOUT, ML, NL, O, S0, S1, kJW, kJE.  Raises where no group
    kernel exists."""
    out = (ctypes.c_int64 * 8)()
    if _native.lib().gmt_jacobi5tb_shared_geom(int(k), int(strips), ctypes.cast(out, ctypes.c_void_p)) != 0:
        raise ValueError(f"jacobi5tb_shared_geom: no shared group kernel for {k} sweeps, {strips} strips")
    return dict(zip(("GOUT", "ML", "NL", "O", "S0", "S1", "kJW", "kJE"), (int(v) for v in out)))


def jacobi5xk(k: int, u: torch.Tensor, un: torch.Tensor, rects: Sequence[tuple[int, int, int, int]],
              dom: tuple[int, int, int, int], halo_mask: int = 0) -> None:
    """``k`` fused Laplace sweeps with the default launch: :func:`jacobi5tb`."""
    jacobi5tb(k, u, un, rects, dom, halo_mask)
