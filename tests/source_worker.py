"""Worker of the Poisson source tests (tests/test_source_cpu.py,
tests/test_source_gpu.py).

``source_worker.py '<json list of jobs>'``, on its own or under
torch.distributed.run, on GMT_TEST_DEVICE (default cpu): every job builds one
NativeJacobi with a source, runs it, and rank 0 gathers the field.  Fields go
to ``<job["save"]>.npy`` for the test to judge against its references; rank 0
prints one JSON line with a result per job.  Jobs:

  run    source engine (host source unless job["source"]), run(job["sweeps"]);
         job["zero"]: the same with the source zeroed -> "<save>_zero.npy"
  resid  residual_norm twice, run(n1), residual_norm, run(n2): read-only,
         repeatable, the later sweeps unchanged
  solve  prepare(), solve(**job["solve"]) from the initial field
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import source_cases as sc  # noqa: E402


def run_jobs(jobs, env):
    import torch.distributed as dist
    from gpu_mpi_tests_amd import engine

    def gather(v):
        if env.world_size == 1:
            return [v]
        out = [None] * env.world_size
        dist.all_gather_object(out, v, group=env.host_group)
        return out

    def field(e, ny, nx):
        parts = gather((e.off_y, e.off_x, e.interior()))
        full = np.full((ny, nx), np.nan)
        for oy, ox, a in parts:
            full[oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
        return full

    def make(job, source):
        return engine.NativeJacobi(
            job["ny"], job["nx"], env, dims=tuple(job["dims"]) if job.get("dims") else None,
            periodic=bool(job.get("periodic", False)), overlap=bool(job.get("overlap", False)),
            graph=bool(job.get("graph", False)), tblock=job.get("tsteps", 1), push=bool(job.get("push", False)),
            transport=job.get("transport", "auto"), init=job.get("init", "random"), seed=sc.SEED, source=source,
            source_amp=job.get("source_amp", 1.0), src_every=job.get("src_every", 0))

    results = []
    for job in jobs:
        ny, nx = job["ny"], job["nx"]
        src = job.get("source") or sc.host_source(ny, nx)
        e = make(job, src)
        res = dict(push=e.push_active, graph=e.graph, graph_fused=e.graph_fused, band_first=e.band_first,
                   transport=e.transport, tsteps=e.tsteps, src_every=e.src_every, setup=e.source_setup())
        try:
            if job["kind"] == "run":
                n = job["sweeps"]
                res["source_plan"] = e.source_plan(n)
                res["plan"] = e.plan(e.src_every) if e.src_every else []
                if job.get("resid0"):
                    res["rn0"] = e.residual_norm()
                e.run(n)
                e.synchronize()
                full = field(e, ny, nx)
                if env.rank == 0 and job.get("save"):
                    np.save(job["save"] + ".npy", full)
                if job.get("late"):  # set_source after a sweep is refused
                    try:
                        e.set_source(np.zeros((e.ny, e.nx)))
                        res["late"] = "accepted"
                    except engine.EngineError as err:
                        res["late"] = str(err)
                if job.get("zero"):
                    z = make(job, np.zeros((ny, nx)))
                    try:
                        z.run(n)
                        z.synchronize()
                        zf = field(z, ny, nx)
                        if env.rank == 0:
                            np.save(job["save"] + "_zero.npy", zf)
                    finally:
                        z.close()
            elif job["kind"] == "resid":
                n1, n2 = job["pre"]
                before = e.interior()
                rn = [e.residual_norm(), e.residual_norm()]
                res["unchanged"] = all(gather(bool(np.array_equal(before, e.interior()))))
                e.run(n1)
                rn.append(e.residual_norm())
                e.run(n2)
                e.synchronize()
                full = field(e, ny, nx)
                if env.rank == 0 and job.get("save"):
                    np.save(job["save"] + ".npy", full)
                res["rn"] = rn
                res["rn_same"] = len({json.dumps(v) for v in gather(rn)}) == 1
            elif job["kind"] == "solve":
                s = dict(job["solve"])
                e.prepare(s.get("check_every", 0) or e.tsteps)
                r = e.solve(**s)
                res["res"] = r
                res["same"] = len({json.dumps(v, sort_keys=True) for v in gather(r)}) == 1
                full = field(e, ny, nx)
                if env.rank == 0 and job.get("save"):
                    np.save(job["save"] + ".npy", full)
        finally:
            e.close()
        results.append(res)
    return results


def main():
    from gpu_mpi_tests_amd.parallel import dist as gd

    jobs = json.loads(sys.argv[1])
    env = gd.init(device=os.environ.get("GMT_TEST_DEVICE", "cpu"))
    res = run_jobs(jobs, env)
    if env.rank == 0:
        print(json.dumps(res), flush=True)
    gd.shutdown()


if __name__ == "__main__":
    main()
