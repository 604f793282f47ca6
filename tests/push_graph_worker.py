"""torchrun worker: the native Jacobi engine with inline halo (push) and
hipGraphs together, several run() calls, vs the serial NumPy reference.
Rank 0 prints one JSON line.  Used by tests/test_push_graph_cpu.py and
tests/test_push_graph_gpu.py.

argv: ny nx tblock dims(PYxPX) periodic(0|1) push(0|1) graph(0|1) shared steps[,steps...]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

from gpu_mpi_tests_amd import engine  # noqa: E402
from gpu_mpi_tests_amd.parallel import dist as gd  # noqa: E402


def main():
    ny, nx, k = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    dims = tuple(int(v) for v in sys.argv[4].split("x"))
    periodic, push, graph = (sys.argv[i] == "1" for i in (5, 6, 7))
    shared = int(sys.argv[8])
    runs = [int(v) for v in sys.argv[9].split(",")]
    env = gd.init(device=os.environ.get("GMT_TEST_DEVICE", "cpu"))
    e = engine.NativeJacobi(ny, nx, env, dims=dims, periodic=periodic, overlap=False, graph=graph, tblock=k,
                            push=push, shared=shared, init="random", seed=11)
    plans = []
    for steps in runs:  # replays from both parities, eager partial passes in between
        plans.append(e.plan(steps))
        e.run(steps)
        e.synchronize()
    part = (e.off_y, e.off_x, e.interior())
    parts = [None] * env.world_size
    dist.all_gather_object(parts, part, group=env.host_group)
    mine = dict(graph_fused=e.graph_fused, graph=e.graph, push=e.push_active,
                graphs=int(e.lib.gmt_engine_jacobi_graphs(e.h)), shared_strips=e.tb_launch(k)["shared_strips"],
                resid=e.residual())  # one more sweep + all-reduce: identical on every rank
    every = [None] * env.world_size
    dist.all_gather_object(every, mine, group=env.host_group)
    if env.rank == 0:
        full = np.full((ny, nx), np.nan)
        for oy, ox, a in parts:
            full[oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
        ref = engine.serial_jacobi(ny, nx, sum(runs), periodic, init="random", seed=11)
        print(json.dumps(dict(equal=bool(np.array_equal(full, ref)), nbad=int((full != ref).sum()),
                              graph_fused=[r["graph_fused"] for r in every], graph=[r["graph"] for r in every],
                              graphs=[r["graphs"] for r in every], push=[r["push"] for r in every],
                              shared_strips=[r["shared_strips"] for r in every],
                              resid_same=len({r["resid"] for r in every}) == 1, plans=plans,
                              transport=e.transport, tsteps=e.tsteps)), flush=True)
    e.close()
    gd.shutdown()


if __name__ == "__main__":
    main()
