"""The CPU backend's IPC exchange (gmt_ipc_plan_init / gmt_ipc_exchange),
gmt_slices_reduce, the contiguous staging copies, gmt_signal_wait and
gmt_fill_poly modes 3 - 5 against the byte-exact models of tests/ipc_cases.py
and tests/comm_cases.py — the same cases tests/test_ipc_gpu.py and
tests/test_comm_kernels_gpu.py run on the gfx950 kernels.  In a child process
with the GPUs hidden: build/lib-host/libgmt.so shares its SONAME with the GPU
library."""
import json
import os
import subprocess
import sys

import ipc_cases
from native_util import ROOT, ensure_host_build

HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")


def test_host_comm_kernels_match_the_models():
    ensure_host_build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ipc_cases.py"), HOST_LIB], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["ok"] and r["backend"] == 0
    assert r["cases"] == len(ipc_cases.CASES) == 21  # no case left out silently
    assert r["skipped"] == ["graph_replay"]          # the CPU backend has no stream capture
    assert r["refusals"] == ipc_cases.N_REFUSALS
    assert r["comm"] == dict(slices=25 * 4 + 5 * 7, stage=15, signal_wait="eager", fill_seeds=3)


def test_case_table_reaches_every_branch():
    """The table itself: the sizes, alignments and chunk counts the cases are there for."""
    by = {c["name"]: c for c in ipc_cases.CASES}
    assert len(by) == len(ipc_cases.CASES)
    chunks = lambda cs: sum(max(1, -(-c["bytes"] // ipc_cases.CHUNK)) for c in cs)  # noqa: E731
    assert by["contig_2049d"]["sends"][0]["bytes"] % 16 == 8            # slot 1 misaligned
    assert chunks(by["over_128_chunks"]["sends"]) == 131 + 1 + 5 > 128  # the walk wraps inside channel 0
    t = by["table_8+8"]
    assert len(t["sends"]) == len(t["recvs"]) == 8 and t["sends"][3]["bytes"] == 0
    assert chunks(t["sends"][1:2]) == 3
    assert any(not c["wait"] for c in t["sends"] + t["recvs"]) and any(not c["signal"] for c in t["sends"] + t["recvs"])
    assert by["send_only"]["recvs"] == [] and by["recv_only"]["sends"] == []
    assert ipc_cases.GRAPH_TURNS.count("graph") == 4 and by["graph_replay"]["graph"]
    for c in ipc_cases.CASES:  # every strided side keeps the plan rules
        for ch in c["sends"] + c["recvs"]:
            assert ch["run"] == 0 or (ch["ld"] >= ch["run"] and ch["bytes"] % ch["run"] == 0), c["name"]
