"""Inline halo (push) together with graph=True on the CPU backend: the
hand-over whose epoch lives in memory (gmt_push_sync_dev, csrc/host/
kernels_host.cpp) and the engine's eager path through it.  The CPU backend
has no graphs, so graph_fused stays False there; the replay path itself is
tests/test_push_graph_gpu.py.

Each case runs in a fresh interpreter: the HIP and host libraries share the
libgmt.so SONAME, so one process may only ever bind one backend."""
import json
import os
import subprocess
import sys

from conftest import free_port
from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")

SYNC = r"""
import ctypes, json
L = ctypes.CDLL({lib!r})
u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
L.gmt_push_sync_dev.argtypes = [u64p, ctypes.POINTER(u64p), ctypes.c_int, u64p, u32p, u32p, u32p, ctypes.c_void_p]
L.gmt_push_sync_dev.restype = ctypes.c_int
local = (ctypes.c_uint64 * 8)()
scratch = (ctypes.c_uint64 * 8)()
epoch, arrivals = ctypes.c_uint64(0), ctypes.c_uint32(0)
err, stop = ctypes.c_uint32(0), ctypes.c_uint32(0)
def at(arr, d):
    return ctypes.cast(ctypes.addressof(arr) + 8 * d, u64p)
def call(mask, target):
    remote = (u64p * 8)(*[at(target, d) for d in range(8)])
    return L.gmt_push_sync_dev(local, remote, mask, ctypes.byref(epoch), ctypes.byref(arrivals),
                               ctypes.byref(err), ctypes.byref(stop), None)
def state():
    return dict(epoch=epoch.value, local=list(local), arrivals=arrivals.value, err=err.value, stop=stop.value)
out = dict(rc=[], states=[])
{body}
print(json.dumps(out))
"""


def _sync(body, **env):
    ensure_host_build()
    p = subprocess.run([sys.executable, "-c", SYNC.format(lib=HOST_LIB, body=body)], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", **env))
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


MASK = 0b10101101  # directions 0, 2, 3, 5, 7


def test_push_sync_dev_self_loop_counts_its_own_epoch():
    """remote[d] = local + d: each call releases *epoch + 1 into its own wait
    words, so it returns at once and advances the epoch; a set stop word makes
    the call touch nothing; mask 0 is a no-op."""
    r = _sync(f"""
for i in range(3):
    out["rc"].append(call({MASK}, local)); out["states"].append(state())
out["rc"].append(call(0, local)); out["states"].append(state())
stop.value = 1
out["rc"].append(call({MASK}, local)); out["states"].append(state())
""")
    assert r["rc"] == [0] * 5, r
    for i in range(3):
        assert r["states"][i] == dict(epoch=i + 1, local=[i + 1 if (MASK >> d) & 1 else 0 for d in range(8)],
                                      arrivals=0, err=0, stop=0), (i, r)
    assert r["states"][3] == r["states"][2], r  # mask 0: nothing happens
    assert r["states"][4] == dict(r["states"][2], stop=1), r  # stopped: neither flags nor epoch nor arrivals move


def test_push_sync_dev_refuses_missing_words():
    r = _sync("""
remote = (u64p * 8)(*[at(local, d) for d in range(8)])
out["rc"].append(L.gmt_push_sync_dev(local, remote, 1, None, ctypes.byref(arrivals), ctypes.byref(err), None, None))
out["rc"].append(L.gmt_push_sync_dev(local, remote, 1, ctypes.byref(epoch), None, ctypes.byref(err), None, None))
out["rc"].append(L.gmt_push_sync_dev(local, None, 1, ctypes.byref(epoch), ctypes.byref(arrivals), ctypes.byref(err), None, None))
out["states"].append(state())
""")
    assert all(rc != 0 for rc in r["rc"]), r
    assert r["states"][0] == dict(epoch=0, local=[0] * 8, arrivals=0, err=0, stop=0), r


def test_push_sync_dev_wait_is_bounded():
    """The neighbour never answers (remote points at a scratch word): after
    GMT_WAIT_TIMEOUT_MS the call sets bit d of err and of stop and returns.
    CPU only: nothing is made to wait on a GPU."""
    r = _sync("""
out["rc"].append(call(1 << 3, scratch)); out["states"].append(state())
out["scratch"] = list(scratch)
""", GMT_WAIT_TIMEOUT_MS="50")
    assert r["rc"] == [0], r
    s = r["states"][0]
    assert s["err"] == 1 << 3 and s["stop"] == 1 << 3 and s["arrivals"] == 0, r
    assert s["local"] == [0] * 8 and r["scratch"][3] == 1, r  # the release went out; the answer never came


def test_engine_push_with_graph_on_the_host_backend():
    """NativeJacobi(push=True, graph=True) at 2 ranks over memfd IPC: every
    pass hands over through gmt_push_sync_dev (eagerly: no graphs here);
    bitwise equal to the serial solve across three run() calls."""
    ensure_host_build()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "push_graph_worker.py"), "140", "300", "20", "2x1", "1", "1", "1", "0",
           "60,45,27"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1",
                                GMT_TRANSPORT="ipc"))
    assert p.returncode == 0, p.stdout + p.stderr
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["push"] == [True, True], r
    assert r["equal"] and r["nbad"] == 0 and r["resid_same"], r
    assert r["graph_fused"] == [False, False] and r["graphs"] == [0, 0], r  # the CPU backend has no graphs
