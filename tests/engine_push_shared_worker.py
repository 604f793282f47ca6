"""torchrun worker: the native Jacobi engine with the inline halo exchange in
shared hand-off group launches (NativeJacobi(push=True, shared=N)) at
world_size ranks vs the serial NumPy reference.  Rank 0 prints one JSON line
with every rank's ``shared_strips``.  Used by tests/test_push_shared_gpu.py.

argv: ny nx steps periodic(0/1) tblock dims(PYxPX) shared"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

from gpu_mpi_tests_amd import engine  # noqa: E402
from gpu_mpi_tests_amd.parallel import dist as gd  # noqa: E402


def main():
    ny, nx, steps, periodic, tblock = (int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] == "1",
                                       int(sys.argv[5]))
    dims = tuple(int(v) for v in sys.argv[6].split("x"))
    shared = int(sys.argv[7])
    env = gd.init(device=os.environ.get("GMT_TEST_DEVICE", "cpu"))
    e = engine.NativeJacobi(ny, nx, env, dims=dims, periodic=periodic, overlap=False, graph=False, tblock=tblock,
                            push=True, shared=shared)
    strips = e.tb_launch(tblock)["shared_strips"]
    e.run(steps)
    e.synchronize()
    part = (e.off_y, e.off_x, e.interior(), strips)
    parts = [None] * env.world_size
    dist.all_gather_object(parts, part, group=env.host_group)
    resid = e.residual()  # one more sweep + all-reduce: identical on every rank
    resids = [None] * env.world_size
    dist.all_gather_object(resids, resid, group=env.host_group)
    if env.rank == 0:
        full = np.full((ny, nx), np.nan)
        for oy, ox, a, _ in parts:
            full[oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
        ref = engine.serial_jacobi(ny, nx, steps, periodic)
        bad = np.argwhere(np.abs(full - ref) > 0)
        print(json.dumps(dict(diff=float(np.abs(full - ref).max()), transport=e.transport, nbad=int(len(bad)),
                              first_bad=bad[:4].tolist(), dims=[e.py, e.px], tsteps=e.tsteps, push=e.push_active,
                              shared_strips=[int(p[3]) for p in parts], resid_same=len(set(resids)) == 1)),
              flush=True)
    e.close()
    gd.shutdown()


if __name__ == "__main__":
    main()
