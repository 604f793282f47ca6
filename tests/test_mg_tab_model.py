"""The table model of the table-driven multigrid transfers (engine.mg_axis_table,
gpu_mpi_tests_amd/mg_tab.py), on the CPU without an engine: for a few hundred
even and odd n and for 8192, 32768 and 65536, with m = engine.mg_coarse_extent(n):
R assembled from the restriction taps is bitwise the transpose of P; tap counts
are 3 or 4; with even splits over 1-8 ranks the taps reach at most 1 fine cell
below and 2 above a rank's share and interpolation at most 1 coarse cell
outside it; ownership by the anchor rule partitions the coarse points; an odd n
reproduces the nested rule [ox/2, (ox+nx)/2) and the weights 0.5 / 1 / 0.5."""
import numpy as np
import pytest

from gpu_mpi_tests_amd import engine, mg_tab

SMALL = list(range(3, 260)) + list(range(1000, 1040)) + [5999, 6000]
BIG = [8192, 32768, 65536]


def bounds(n, p):
    base, rem = divmod(n, p)
    return [i * base + min(i, rem) for i in range(p)] + [n]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_axis(n):
    m = engine.mg_coarse_extent(n)
    assert m == ((n - 1) // 2 if n % 2 else n // 2 - 1) and m >= 1
    q, t, r = engine.mg_axis_table(n, m)
    i = np.arange(1, n + 1, dtype=np.int64)
    assert q.dtype == np.int64 and r.dtype == np.int64 and t.dtype == np.float64
    # 64-bit products: exact against Python integers at the ends and where 32 bits overflow
    for k in {1, 2, n // 2, n - 1, n}:
        assert (int(q[k - 1]), int(r[k - 1])) == divmod(k * (m + 1), n + 1) and t[k - 1] == int(r[k - 1]) / (n + 1)
    assert q.min() >= 0 and q.max() <= m and (np.diff(q) >= 0).all() and ((0 <= t) & (t < 1)).all()
    # P^T from the fine side, entries (J, i, weight) sorted by (J, i)
    lo = q >= 1
    hi = (r != 0) & (q + 1 <= m)
    PJ = np.concatenate([q[lo], q[hi] + 1])
    Pi = np.concatenate([i[lo], i[hi]])
    Pw = np.concatenate([1.0 - t[lo], t[hi]])
    order = np.lexsort((Pi, PJ))
    # R from the coarse side
    first, count, w = mg_tab.axis_taps(n, m)
    assert set(np.unique(count).tolist()) <= {3, 4}, (n, np.unique(count))
    assert w.shape[1] <= 4
    k = np.arange(w.shape[1])[None, :]
    live = k < count[:, None]
    RJ = np.broadcast_to(np.arange(1, m + 1)[:, None], w.shape)[live]
    Ri = (first[:, None] + k)[live]
    Rw = w[live]
    assert np.array_equal(RJ, PJ[order]) and np.array_equal(Ri, Pi[order]), n
    assert np.array_equal(_bits(Rw), _bits(Pw[order])), n  # R is bitwise P^T
    assert (w[~live] == 0).all() and (Rw > 0).all()
    # ownership and halo needs on even splits
    anchor = np.arange(1, m + 1, dtype=np.int64) * (n + 1) // (m + 1)
    assert (np.diff(anchor) >= 2).all() and anchor[0] >= 2 and anchor[-1] <= n
    for p in range(1, 9):
        if n // p < 2:
            break
        b = bounds(n, p)
        cb = [int(v) for v in mg_tab.coarse_bound(n, m, b)]
        assert cb[0] == 0 and cb[-1] == m and all(c1 >= c0 for c0, c1 in zip(cb, cb[1:])), (n, p, cb)
        owner = np.searchsorted(np.array(b[1:]), anchor, side="left")  # the rank whose cells b[k]+1 .. b[k+1] hold the anchor
        assert np.array_equal(owner, np.searchsorted(np.array(cb[1:]), np.arange(1, m + 1), side="left")), (n, p)
        if n % 2:
            assert cb == [v // 2 for v in b], (n, p)  # the nested rule [ox/2, (ox+nx)/2)
        for kk in range(p):
            tab = mg_tab.region_tables(n, m, b[kk], b[kk + 1] - b[kk], cb[kk], cb[kk + 1] - cb[kk])
            assert tab["lo"] <= 1 and tab["hi"] <= 2, (n, p, kk, tab["lo"], tab["hi"])
            assert tab["pq"].min() >= -1 and tab["pq"].max() + 1 <= cb[kk + 1] - cb[kk], (n, p, kk)
            if n % 2:
                assert tab["lo"] <= 1 and tab["hi"] <= 1
    if n % 2:
        assert (count == 3).all() and np.array_equal(first, 2 * np.arange(1, m + 1) - 1)
        assert np.array_equal(w, np.tile([0.5, 1.0, 0.5], (m, 1)))
        assert np.array_equal(t, np.where(i % 2 == 0, 0.0, 0.5)) and np.array_equal(q, i // 2)
    else:
        assert (r != 0).all()  # no fine point of an even axis sits on a coarse point


@pytest.mark.parametrize("chunk", range(4))
def test_small_axes(chunk):
    for n in SMALL[chunk::4]:
        check_axis(n)


@pytest.mark.parametrize("n", BIG)
def test_headline_axes(n):
    check_axis(n)
    assert engine.mg_coarse_extent(n) == n // 2 - 1


def test_chains_and_refusals():
    def chain(n):
        out = [n]
        while engine.mg_coarse_extent(out[-1]) >= 1:
            out.append(engine.mg_coarse_extent(out[-1]))
        return out

    assert chain(8192) == [8192, 4095, 2047, 1023, 511, 255, 127, 63, 31, 15, 7, 3, 1]
    assert chain(32768)[:3] == [32768, 16383, 8191] and chain(32768)[-1] == 1
    assert chain(766) == [766, 382, 190, 94, 46, 22, 10, 4, 1] and chain(256) == [256, 127, 63, 31, 15, 7, 3, 1]
    assert [engine.mg_coarse_extent(n) for n in (1, 2, 3, 4)] == [0, 0, 1, 1]
    for bad in ((22, 10, 4, 4, 1, 4), (22, 10, 4, 8, 1, 2), (22, 21, 0, 22, 0, 21), (22, 4, 0, 22, 0, 4),
                (22, 0, 0, 22, 0, 0), (22, 10, 20, 4, 0, 10), (22, 10, -1, 4, 0, 2)):
        with pytest.raises(ValueError):
            mg_tab.region_tables(*bad)
