"""Inline halo (push) passes replayed from hipGraphs on the GPU.

The hand-over between two push passes reads its epoch from device memory
(gmt_push_sync_dev, csrc/kernels/ipc.hip), so the engine captures a full pass
and its hand-over once per parity and replays them (JacobiSolver::
capture_graphs / step_block): NativeJacobi(push=True, graph=True).graph_fused.

* the hand-over kernel alone, eager and replayed from a captured launch;
* one rank, periodic (no hand-over at all: the graph is the pass alone);
* two / four ranks sharing cuda:0 over IPC mappings, per-strip and
  shared-group passes;
* mpi_jacobi2d --push --graph.

Every field is compared bitwise with the serial NumPy solve, over several
run() calls whose step counts make the replays start from both parities and
alternate with eager partial passes."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import free_port
from gpu_mpi_tests_amd import _native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
MPIRUN = "/opt/conda/bin/mpirun"
SPACE_DEVICE, SPACE_PINNED, SPACE_FLAGS = 1, 2, 4  # gmt/rt.h
RUNS = (60, 45, 27)


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _rt():
    return _native.lib()  # the gmt_rt_* prototypes are declared with the kernels' (_native._SIGS)


def test_push_sync_dev_kernel_eager_and_replayed():
    """Self-loop (remote[d] = local + d, all 8 directions): every launch
    releases *epoch + 1 into its own wait words and the last of its 8
    workgroups advances the epoch.  5 eager launches, then ONE captured launch
    replayed 4 times: a replay hands over the epoch of its own turn."""
    L = _rt()
    ok = lambda e, what: _native.check(e, what)  # noqa: E731
    flags, ctl, err, stream, graph = (ctypes.c_void_p() for _ in range(5))
    ok(L.gmt_rt_malloc(ctypes.byref(flags), 64, SPACE_FLAGS), "malloc flags")
    ok(L.gmt_rt_malloc(ctypes.byref(ctl), 16, SPACE_DEVICE), "malloc ctl")  # epoch | arrivals
    ok(L.gmt_rt_malloc(ctypes.byref(err), 4, SPACE_PINNED), "malloc err")
    ok(L.gmt_rt_stream_create(ctypes.byref(stream), 0), "stream")
    try:
        ok(L.gmt_rt_memset_async(ctl, 0, 16, stream), "memset")
        ok(L.gmt_rt_memset_async(flags, 0, 64, stream), "memset")
        ctypes.memset(err.value, 0, 4)
        remote = (ctypes.c_void_p * 8)(*[flags.value + 8 * d for d in range(8)])

        def launch():
            ok(L.gmt_push_sync_dev(flags, remote, 0xFF, ctl, ctl.value + 8, err, None, stream), "gmt_push_sync_dev")

        def state():
            ok(L.gmt_rt_stream_synchronize(stream), "sync")
            f, c = np.zeros(8, np.uint64), np.zeros(4, np.uint32)
            ok(L.gmt_rt_memcpy(f.ctypes.data, flags, 64), "D2H")
            ok(L.gmt_rt_memcpy(c.ctypes.data, ctl, 16), "D2H")
            return f.tolist(), int(c[0]) | int(c[1]) << 32, int(c[2]), ctypes.c_uint32.from_address(err.value).value

        for _ in range(5):
            launch()
        assert state() == ([5] * 8, 5, 0, 0)
        # mask 0: nothing is launched, the epoch stays
        ok(L.gmt_push_sync_dev(flags, remote, 0, ctl, ctl.value + 8, err, None, stream), "mask 0")
        assert state() == ([5] * 8, 5, 0, 0)
        ok(L.gmt_rt_stream_begin_capture(stream), "begin capture")
        launch()
        ok(L.gmt_rt_stream_end_capture(stream, ctypes.byref(graph)), "end capture")
        assert graph.value
        assert state() == ([5] * 8, 5, 0, 0)  # recorded, not run
        for _ in range(4):
            ok(L.gmt_rt_graph_launch(graph, stream), "graph launch")
        assert state() == ([9] * 8, 9, 0, 0)
        launch()  # eager hand-overs and replays mix
        ok(L.gmt_rt_graph_launch(graph, stream), "graph launch")
        assert state() == ([11] * 8, 11, 0, 0)
    finally:
        L.gmt_rt_stream_synchronize(stream)
        if graph.value:
            L.gmt_rt_graph_destroy(graph)
        L.gmt_rt_stream_destroy(stream)
        L.gmt_rt_free(flags, SPACE_FLAGS)
        L.gmt_rt_free(ctl, SPACE_DEVICE)
        L.gmt_rt_free(err, SPACE_PINNED)


@pytest.fixture(scope="module")
def env():
    from gpu_mpi_tests_amd.parallel import dist as gd

    return gd.init(device="cuda")


@pytest.mark.parametrize("ny,nx,k", [(300, 700, 20), (257, 1031, 12), (520, 600, 4)])
def test_push_graph_one_rank_periodic(env, ny, nx, k):
    """Every neighbour is this rank: no hand-over, the graph is the pass
    alone.  RUNS = 60, 45, 27 sweeps: at K = 20 the planner makes that
    20 20 20 | 20 20 5 | 12 12 3, i.e. 3 + 2 replays with eager partial passes
    after them, so replays start from both parities (K = 12: 5 + 3 + 2
    replays, K = 4: 15 + 9 + 6); the plan's shape is asserted below."""
    from gpu_mpi_tests_amd import engine

    e = engine.NativeJacobi(ny, nx, env, periodic=True, overlap=False, graph=True, tblock=k, push=True,
                            transport="local", init="random", seed=5)
    try:
        assert e.push_active and e.graph
        assert e.graph_fused
        assert e.lib.gmt_engine_jacobi_graphs(e.h) == 3
        assert any(p.count(k) % 2 == 1 for p in map(e.plan, RUNS)) and any(set(p) - {k} for p in map(e.plan, RUNS))
        for steps in RUNS:
            e.run(steps)
            e.synchronize()
        got = e.interior()
    finally:
        e.close()
    want = engine.serial_jacobi(ny, nx, sum(RUNS), True, init="random", seed=5)
    assert np.array_equal(got, want), float(np.abs(got - want).max())


def test_graph_fused_is_false_without_graph(env):
    from gpu_mpi_tests_amd import engine

    e = engine.NativeJacobi(300, 700, env, periodic=True, overlap=False, graph=False, tblock=20, push=True,
                            transport="local")
    try:
        assert e.push_active and not e.graph and not e.graph_fused
        assert e.lib.gmt_engine_jacobi_graphs(e.h) == 0
    finally:
        e.close()


@pytest.mark.parametrize("np_,ny,nx,k,dims,periodic,shared", [
    (2, 400, 900, 20, "2x1", True, 0),
    (2, 300, 1200, 12, "1x2", False, 0),
    (4, 600, 1100, 20, "2x2", True, 0),
    (2, 400, 900, 20, "2x1", True, 2),
])
def test_push_graph_ranks_sharing_the_gpu(np_, ny, nx, k, dims, periodic, shared):
    """np_ ranks on cuda:0 over IPC mappings: each rank replays pass +
    hand-over from its own graph; the device epochs of the ranks stay in step
    through replays and eager partial passes alike.  The smallest shares the
    push rules allow (more than 256 columns, at least 2K + 2 rows, two strips
    where both x faces are pushed).  shared = 2: the pass inside the graph
    runs in shared hand-off groups."""
    cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(np_), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "push_graph_worker.py"), str(ny), str(nx), str(k), dims,
           "1" if periodic else "0", "1", "1", str(shared), ",".join(map(str, RUNS))]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd=ROOT,
                       env=dict(os.environ, OMP_NUM_THREADS="1", GMT_TRANSPORT="ipc", GMT_TEST_DEVICE="cuda"))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["push"] == [True] * np_, r
    assert r["graph_fused"] == [True] * np_ and r["graphs"] == [3] * np_, r
    assert r["equal"] and r["nbad"] == 0, r
    assert r["resid_same"], r
    if shared:
        assert r["shared_strips"] == [shared] * np_, r
    assert any(pl.count(k) % 2 == 1 for pl in r["plans"]) and any(set(pl) - {k} for pl in r["plans"]), r


def test_app_push_graph():
    """mpi_jacobi2d --push --graph at 2 ranks: 301 x 301 splits 2x1 into
    shares of 150 / 151 rows x 301 columns, enough for push at K = 4."""
    exe = os.path.join(BIN, "mpi_jacobi2d")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} not built (run make all / __graft_entry__.build())")
    cmd = [MPIRUN, "-np", "2", exe, "301", "23", "--check", "--tblock", "--tsteps=4", "--warmup=3", "--graph",
           "--push", "--transport=ipc"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd="/tmp")
    out = p.stdout
    assert p.returncode == 0, f"{' '.join(cmd)} rc={p.returncode}\n{out[-3000:]}\n{p.stderr[-3000:]}"
    assert re.search(r"transport = ipc overlap=1 \(inline halo\) graph=1", out), out
    assert "graphs    = sweep:1 fused:1" in out, out
    m = re.search(r"check\s*: max\|diff\| vs serial = ([0-9.eE+-]+) OK", out)
    assert m and float(m.group(1)) == 0.0, out
