"""The per-axis tables of the table-driven multigrid transfers, from integers
(the Python definition of csrc/include/gmt/mg_tab.hpp; NumPy only).

An axis has ``n`` fine and ``m`` coarse interior points on the same interval,
rings at 0 and n + 1 (fine) and at 0 and m + 1 (coarse); every index here is
global and 1-based.  Fine point ``i`` lies between coarse points ``q`` and
``q + 1`` with ``q, r = divmod(i*(m+1), n+1)`` and ``t = r/(n+1)`` (one fp64
division); it interpolates with the weights ``1.0 - t`` and ``t``.  Coarse
point ``J`` gathers from the fine points with ``q(i) = J`` (weight
``1.0 - t(i)``) or with ``q(i) + 1 = J`` and ``r(i) != 0`` (weight ``t(i)``),
in ascending order: the transpose, bit for bit.  Coarse point ``J`` is owned by
the rank that owns fine cell ``J*(n+1) // (m+1)``."""
from __future__ import annotations

import numpy as np

MIN_TAPS, MAX_TAPS = 3, 4  # taps of a coarse point per axis that the kernels take
TAP_HALO = 2               # fine cells outside a region its coarse points may gather from
RING_HALO = 1              # coarse cells outside a region its fine points may interpolate from


def coarse_extent(n: int) -> int:
    """Coarse points of an axis of ``n`` fine ones under ``coarsen="any"``:
    ``(n-1)/2`` for odd ``n`` (the nested rule), ``n/2 - 1`` for even ``n``."""
    n = int(n)
    return (n - 1) // 2 if n % 2 else n // 2 - 1


def axis_table(n: int, m: int):
    """``(q, t, r)`` of the fine points ``i = 1 .. n`` (entry ``i - 1``): int64, float64, int64."""
    n, m = int(n), int(m)
    a = np.arange(1, n + 1, dtype=np.int64) * np.int64(m + 1)
    q, r = np.divmod(a, np.int64(n + 1))
    t = r.astype(np.float64) / np.float64(n + 1)
    return q, t, r


def axis_taps(n: int, m: int):
    """``(first, count, w)`` of the coarse points ``J = 1 .. m`` (entry
    ``J - 1``): the first fine tap, the tap count and the weights
    ``w[J-1, k]`` of tap ``first + k`` (0 beyond the count)."""
    n, m = int(n), int(m)
    q, t, _ = axis_table(n, m)
    J = np.arange(1, m + 1, dtype=np.int64)
    first = (J - 1) * (n + 1) // (m + 1) + 1
    last = ((J + 1) * (n + 1) + m) // (m + 1) - 1
    count = last - first + 1
    w = np.zeros((m, int(count.max()) if m else 0))
    for k in range(w.shape[1]):
        i = np.minimum(first + k, n)
        wk = np.where(q[i - 1] == J, 1.0 - t[i - 1], t[i - 1])
        w[:, k] = np.where(k < count, wk, 0.0)
    return first, count, w


def coarse_bound(n: int, m: int, b):
    """Coarse points owned by the ranks that own fine cells ``1 .. b``: the ``J``
    with ``J*(n+1) // (m+1) <= b``; ``b // 2`` on an odd axis under the nested rule."""
    return np.minimum(((np.asarray(b, dtype=np.int64) + 1) * (int(m) + 1) - 1) // (int(n) + 1), int(m))


def region_tables(n: int, m: int, fo: int, fn: int, co: int, cn: int) -> dict:
    """The tables of one axis of one region (fine cells ``fo+1 .. fo+fn``, coarse
    cells ``co+1 .. co+cn``), region-relative as the kernels take them:
    ``pq`` (the coarse cell below each fine cell, -1 .. cn-1), ``pt``; ``rf``
    (first tap, >= -2), ``rc`` (count), ``rw`` (cn x 4); the halo needs
    ``lo``, ``hi`` (fine) and ``ring_lo``, ``ring_hi`` (coarse).  ValueError
    where gmt_mg_xfer_plan_create refuses."""
    n, m, fo, fn, co, cn = (int(v) for v in (n, m, fo, fn, co, cn))
    if n < 1 or m < 1 or m > n or min(fo, fn, co, cn) < 0 or fo + fn > n or co + cn > m:
        raise ValueError("mg transfer tables: a bad description")
    q, t, _ = axis_table(n, m)
    pq = q[fo:fo + fn] - (co + 1)
    pt = t[fo:fo + fn].copy()
    if fn and (pq.min() < -RING_HALO or pq.max() + 1 > cn - 1 + RING_HALO):
        raise ValueError("mg transfer tables: a coarse cell more than 1 outside the coarse region")
    first, count, w = axis_taps(n, m)
    first, count, w = first[co:co + cn], count[co:co + cn], w[co:co + cn]
    if cn and (count.min() < MIN_TAPS or count.max() > MAX_TAPS):
        raise ValueError("mg transfer tables: a coarse point without 3 or 4 taps")
    rf = first - (fo + 1)
    lo = int(max(0, -rf.min())) if cn else 0
    hi = int(max(0, (rf + count - 1).max() - (fn - 1))) if cn else 0
    if lo > TAP_HALO or hi > TAP_HALO:
        raise ValueError("mg transfer tables: a tap more than 2 cells outside the region")
    rw = np.zeros((cn, 4))
    rw[:, :w.shape[1]] = w[:, :4]
    return dict(pq=pq, pt=pt, rf=rf, rc=count, rw=rw, lo=lo, hi=hi,
                ring_lo=int(fn > 0 and pq.min() < 0), ring_hi=int(fn > 0 and pq.max() + 1 > cn - 1))
