"""The other communication entry points, driven through gmt_rt memory like
tests/ipc_cases.py (whose Rt this uses), so one set of checks runs on the
gfx950 kernels (tests/test_comm_kernels_gpu.py) and on the CPU backend (from
ipc_cases.main, in tests/test_ipc_cpu.py's child process):

* gmt_slices_reduce — the reduction half of the ipc all-reduce — against the
  NumPy loop in rank order, bitwise (IEEE adds, nothing to contract; fmax);
* gmt_stage_copy / gmt_stage_scatter with rows == 0: the aligned loop with its
  one-piece remainder, the byte tail and the unaligned byte loop;
* gmt_signal_wait on a signal the host raised first;
* gmt_fill_poly modes 3, 4 and 5.

NaN results are compared as "NaN on both sides": the sign and payload of a
generated NaN (inf - inf) are the processor's choice, everything else bitwise."""
import ctypes
from fractions import Fraction

import numpy as np

from gpu_mpi_tests_amd import _native as nat

SLICE_NS = (1, 255, 256, 257, 4099)
SLICE_COUNTS = (1, 2, 3, 8, 63)
STAGE_BYTES = (0, 8, 16, 24, 4096, 4104, (1 << 20) + 40)
STAGE_WGS = (1, 4, 300)
STAGE_SHIFTS = (0, 8, 1)  # device side 16-B aligned | 8-B aligned | unaligned
SENTINEL = -12345.0


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------ gmt_slices_reduce
def slices_data(n, ns, kind, shift=0):
    """Signed values over 30 decades (the order of the additions matters); kind
    "special" adds, by element, NaN / +-inf in slice 0, a middle slice, the last slice, or NaN in every slice."""
    g = np.random.default_rng(1000 * n + ns)
    x = np.where(g.random((ns, n)) < 0.5, -1.0, 1.0) * 10.0 ** g.uniform(-15.0, 15.0, (ns, n))
    if kind == "special":
        mid, last = ns // 2, ns - 1
        for i in range(n):
            p = (i + n + shift) % 8
            if p == 1:
                x[0, i] = np.nan
            elif p == 2:
                x[mid, i] = np.nan
            elif p == 3:
                x[last, i] = np.nan
            elif p == 4:
                x[mid, i] = np.inf
            elif p == 5:
                x[0, i] = -np.inf
            elif p == 6:
                x[:, i] = np.nan
            elif p == 7:
                x[0, i], x[last, i] = np.inf, -np.inf  # the sum is NaN when ns > 1
    return x


def slices_reference(op, x):
    acc = x[0].copy()
    with np.errstate(invalid="ignore"):
        for r in range(1, x.shape[0]):
            acc = acc + x[r] if op == 0 else np.fmax(acc, x[r])
    return acc


def run_slices(rt, ns_list=SLICE_COUNTS, n_list=SLICE_NS):
    L = rt.L
    checked = 0
    try:
        cap = max(n_list) * max(ns_list)
        inp = rt.malloc(8 * cap, nat.SPACE_DEVICE)
        pad = 8
        outb = rt.malloc(8 * (max(n_list) + 2 * pad), nat.SPACE_DEVICE)
        for n in n_list:
            for ns in ns_list:
                for op, kind, shift in ((0, "plain", 0), (0, "special", 0), (1, "special", 0), (1, "plain", 0)) + \
                        (tuple((1, "special", s) for s in range(1, 8)) if n == 1 else ()):
                    x = slices_data(n, ns, kind, shift)
                    want = slices_reference(op, x)
                    what = f"gmt_slices_reduce op {op} n {n} nslices {ns} {kind} shift {shift}"
                    rt.put(inp, x)
                    rt.put(outb, np.full(n + 2 * pad, SENTINEL))
                    rt.ok(L.gmt_slices_reduce(op, n, ns, inp, outb + 8 * pad, rt.stream), what)
                    rt.sync()
                    got = rt.get(outb, n + 2 * pad, np.float64)
                    assert (got[:pad] == SENTINEL).all() and (got[pad + n:] == SENTINEL).all(), what + ": guard"
                    bad = np.flatnonzero(~((got[pad:pad + n].view(np.uint64) == want.view(np.uint64)) |
                                           (np.isnan(got[pad:pad + n]) & np.isnan(want))))
                    assert bad.size == 0, f"{what}: element {bad[0]}: got {got[pad + bad[0]]!r}, expected " \
                                          f"{want[bad[0]]!r}, slices {x[:, bad[0]].tolist()[:8]}"
                    assert same_bits(rt.get(inp, n * ns, np.float64), x.ravel()), what + ": input changed"
                    # in place: out is in[0..n); the other slices stay
                    rt.ok(L.gmt_slices_reduce(op, n, ns, inp, inp, rt.stream), what + " in place")
                    rt.sync()
                    after = rt.get(inp, n * ns, np.float64).reshape(ns, n)
                    assert same_bits(after[0], want), what + " in place"
                    assert same_bits(after[1:], x[1:]), what + " in place: another slice changed"
                    checked += 1
        # n == 0: success, nothing touched; op 2 and nslices 0: refused, nothing touched
        x = slices_data(8, 3, "plain")
        rt.put(inp, x)
        rt.put(outb, np.full(16, SENTINEL))
        assert L.gmt_slices_reduce(0, 0, 3, inp, outb, rt.stream) == 0, "n == 0"
        assert L.gmt_slices_reduce(1, 0, 1, inp, outb, rt.stream) == 0, "n == 0"
        assert L.gmt_slices_reduce(2, 8, 3, inp, outb, rt.stream) != 0, "op 2 not refused"
        assert L.gmt_slices_reduce(-1, 8, 3, inp, outb, rt.stream) != 0, "op -1 not refused"
        assert L.gmt_slices_reduce(0, 8, 0, inp, outb, rt.stream) != 0, "nslices 0 not refused"
        assert L.gmt_slices_reduce(0, -1, 3, inp, outb, rt.stream) != 0, "n < 0 not refused"
        rt.sync()
        assert (rt.get(outb, 16, np.float64) == SENTINEL).all() and same_bits(rt.get(inp, 24, np.float64), x.ravel())
    finally:
        rt.free_all()
    return checked


# ------------------------------------------------------------------ gmt_stage_copy / gmt_stage_scatter, rows == 0
def run_stage(rt, shifts=STAGE_SHIFTS, wgs_list=STAGE_WGS, scatter_wgs=(1, 3)):
    L = rt.L
    nchunk = len(STAGE_BYTES)
    launches = 0
    try:
        # chunk k at a 256-byte boundary (+ shift on the device side), 64 guard bytes or more around it
        offs, cur = [], 0
        for b in STAGE_BYTES:
            cur = (cur + 64 + 255) // 256 * 256
            offs.append(cur)
            cur += b + 16  # room for the largest shift
        total = cur + 64
        dev_src = rt.malloc(total, nat.SPACE_DEVICE)
        dev_dst = rt.malloc(total, nat.SPACE_DEVICE)
        host = rt.malloc(total, nat.SPACE_PINNED)
        flags = rt.malloc(8 * nchunk, nat.SPACE_PINNED_COHERENT)
        counters = rt.malloc(4 * nchunk, nat.SPACE_DEVICE)
        table = rt.malloc(ctypes.sizeof(nat.StageChunk) * nchunk, nat.SPACE_DEVICE)
        rt.put(counters, np.zeros(nchunk, np.uint32))
        g = np.random.default_rng(7)
        value = 40
        for shift in shifts:
            src_img = g.integers(0, 256, total, dtype=np.uint8)
            rt.put(dev_src, src_img)
            blank = ((np.arange(total) * 29 + 3) & 0xFF).astype(np.uint8)
            want = blank.copy()
            for k, b in enumerate(STAGE_BYTES):
                want[offs[k]:offs[k] + b] = src_img[offs[k] + shift:offs[k] + shift + b]
            descs = (nat.StageChunk * nchunk)(*[
                nat.StageChunk(dev_src + offs[k] + shift, host + offs[k], b, 0, 0, 0, None)
                for k, b in enumerate(STAGE_BYTES)])
            rt.put(table, np.frombuffer(bytes(descs), np.uint8))
            for wgs in wgs_list:
                value += 1
                what = f"gmt_stage_copy device side +{shift} B, {wgs} workgroups"
                rt.put(host, blank)
                rt.ok(L.gmt_stage_copy(nchunk, table, counters, flags, value, wgs, rt.stream), what)
                rt.sync()
                got = rt.get(host, total)
                if not np.array_equal(got, want):
                    o = int(np.flatnonzero(got != want)[0])
                    k = max(i for i in range(nchunk) if offs[i] <= o) if o >= offs[0] else -1
                    raise AssertionError(f"{what}: host byte {o} (chunk {k} of {STAGE_BYTES[k]} bytes, offset "
                                         f"{o - offs[k]}): got {int(got[o])}, expected {int(want[o])}")
                assert rt.get(flags, nchunk, np.uint64).tolist() == [value] * nchunk, what + ": flags"
                assert rt.get(counters, nchunk, np.uint32).tolist() == [0] * nchunk, what + ": counters"
                launches += 1
            # the same chunks back out of page-locked memory into another device buffer
            descs = (nat.StageChunk * nchunk)(*[
                nat.StageChunk(host + offs[k], dev_dst + offs[k] + shift, b, 0, 0, 0, None)
                for k, b in enumerate(STAGE_BYTES)])
            rt.put(table, np.frombuffer(bytes(descs), np.uint8))
            back = blank.copy()
            for k, b in enumerate(STAGE_BYTES):
                back[offs[k] + shift:offs[k] + shift + b] = want[offs[k]:offs[k] + b]
            for wpc in scatter_wgs:
                what = f"gmt_stage_scatter device side +{shift} B, {wpc} workgroups per chunk"
                rt.put(dev_dst, blank)
                rt.ok(L.gmt_stage_scatter(nchunk, table, wpc, rt.stream), what)
                rt.sync()
                got = rt.get(dev_dst, total)
                if not np.array_equal(got, back):
                    o = int(np.flatnonzero(got != back)[0])
                    raise AssertionError(f"{what}: device byte {o}: got {int(got[o])}, expected {int(back[o])}")
                launches += 1
    finally:
        rt.free_all()
    return launches


# ------------------------------------------------------------------ gmt_signal_wait
def run_signal_wait(rt):
    """Every wait finds its signal already raised: three eager waits on a signal
    of 3, then (where the backend captures) the wait replayed from a graph after
    the host raised the signal to 4."""
    L = rt.L
    graph = ctypes.c_void_p()
    try:
        w = rt.malloc(24, nat.SPACE_FLAGS)  # signal | seen | err
        signal, seen, err = w, w + 8, w + 16
        rt.put(w, np.array([3, 0, 0], np.uint64))

        def state():
            rt.sync()
            v = rt.get(w, 3, np.uint64)
            return int(v[0]), int(v[1]), int(v[2]) & 0xFFFFFFFF

        for k in (1, 2, 3):
            rt.ok(L.gmt_signal_wait(signal, seen, err, rt.stream), "gmt_signal_wait")
            assert state() == (3, k, 0), (k, state())
        for args in ((None, seen, err), (signal, None, err), (signal, seen, None)):
            assert L.gmt_signal_wait(*args, rt.stream) != 0, args
        assert state() == (3, 3, 0), state()  # refused: nothing launched
        rt.put(signal, np.array([4], np.uint64))
        rc = L.gmt_rt_stream_begin_capture(rt.stream)
        if rc != 0 and not rt.hip:  # no capture on this backend: the fourth wait eagerly
            rt.ok(L.gmt_signal_wait(signal, seen, err, rt.stream), "gmt_signal_wait")
            assert state() == (4, 4, 0), state()
            return "eager"
        rt.ok(rc, "begin capture")
        rt.ok(L.gmt_signal_wait(signal, seen, err, rt.stream), "captured gmt_signal_wait")
        rt.ok(L.gmt_rt_stream_end_capture(rt.stream, ctypes.byref(graph)), "end capture")
        assert state() == (4, 3, 0), state()  # recorded, not run
        rt.ok(L.gmt_rt_graph_launch(graph, rt.stream), "graph launch")
        assert state() == (4, 4, 0), state()
        return "graph"
    finally:
        rt.L.gmt_rt_stream_synchronize(rt.stream)
        if graph.value:
            L.gmt_rt_graph_destroy(graph)
        rt.free_all()


# ------------------------------------------------------------------ gmt_fill_poly modes 3, 4, 5
FILL_NY, FILL_NX, FILL_LD = 37, 129, 140  # a 37 x 129 block inside a pitch of 140
FILL_SEEDS = (0, 12345, (1 << 32) + 7)


def run_fill(rt):
    from gpu_mpi_tests_amd import engine

    L = rt.L
    ny, nx, ld = FILL_NY, FILL_NX, FILL_LD
    rows, r0, c0 = ny + 2, 1, 5
    try:
        z = rt.malloc(8 * rows * ld, nat.SPACE_DEVICE)
        at = z + 8 * (r0 * ld + c0)

        def fill(calls):
            rt.put(z, np.full(rows * ld, SENTINEL))
            for (mode, cnx, cny, x0, dx, y0, dy, p) in calls:
                rt.ok(L.gmt_fill_poly(mode, cnx, cny, x0, dx, y0, dy, p, ld, rt.stream), f"gmt_fill_poly mode {mode}")
            rt.sync()
            got = rt.get(z, rows * ld, np.float64).reshape(rows, ld)
            outside = np.ones((rows, ld), bool)
            outside[r0:r0 + ny, c0:c0 + nx] = False
            assert (got[outside] == SENTINEL).all(), "a cell outside the block was written"
            return got[r0:r0 + ny, c0:c0 + nx]

        i, j = np.arange(nx, dtype=np.float64)[None, :], np.arange(ny, dtype=np.float64)[:, None]
        # mode 4: integer lattice with a negative origin, no contraction: NumPy's own roundings
        x0, dx, y0, dy = -7.0, 0.013, -3.0, 0.007
        x, y = (x0 + i) * dx, (y0 + j) * dy
        want = x * x * x + y * y
        got = fill([(4, nx, ny, x0, dx, y0, dy, at)])
        assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist(), "mode 4 differs from x*x*x + y*y"
        # mode 5: the lattice hash, whole and as two halves with shifted origins
        gx0, gy0, half = -11, -5, 64
        for seed in FILL_SEEDS:
            gx = np.broadcast_to(gx0 + np.arange(nx, dtype=np.int64)[None, :], (ny, nx))
            gy = np.broadcast_to(gy0 + np.arange(ny, dtype=np.int64)[:, None], (ny, nx))
            want = engine.lattice_uniform(gx, gy, seed)
            assert 0.0 <= want.min() and want.max() < 1.0 and np.unique(want).size > 0.99 * want.size
            whole = fill([(5, nx, ny, float(gx0), float(seed), float(gy0), 0.0, at)])
            assert whole.view(np.uint64).tolist() == want.view(np.uint64).tolist(), f"mode 5 seed {seed}"
            halves = fill([(5, half, ny, float(gx0), float(seed), float(gy0), 0.0, at),
                           (5, nx - half, ny, float(gx0 + half), float(seed), float(gy0), 0.0, at + 8 * half)])
            assert halves.view(np.uint64).tolist() == want.view(np.uint64).tolist(), f"mode 5 seed {seed}, two halves"
        # mode 3: x0 + i*dx, possibly one fma: within the two roundings of the uncontracted form of the exact value
        x0, dx = -0.3, 0.1
        got = fill([(3, nx, ny, x0, dx, 99.0, 99.0, at)])
        for k in range(nx):
            exact = Fraction(x0) + k * Fraction(dx)
            tol = 2.5 * 2.0 ** -53 * (abs(x0) + abs(k * dx))
            col = got[:, k]
            assert (col == col[0]).all(), f"mode 3 column {k} varies with the row"
            assert abs(Fraction(float(col[0])) - exact) <= Fraction(tol), \
                f"mode 3 column {k}: got {col[0]!r}, exact {float(exact)!r}, tolerance {tol:.3e}"
    finally:
        rt.free_all()
    return len(FILL_SEEDS)


def run_all(rt):
    return dict(slices=run_slices(rt), stage=run_stage(rt), signal_wait=run_signal_wait(rt), fill_seeds=run_fill(rt))
