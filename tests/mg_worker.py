"""Worker and reference helpers of the multigrid tests (tests/test_mg_cpu.py,
tests/test_mg_gpu.py).

As a program (one rank on its own, or under torch.distributed.run):
``mg_worker.py '<json config>'`` builds one NativeJacobi on GMT_TEST_DEVICE
(default cpu) and runs the config's ``ops`` on it in order; rank 0 prints one
JSON line with a result per op and saves the gathered fields the ops asked for
into the ``.npz`` file ``out``.  The test judges everything against
``engine.serial_mg`` (helper below)."""
import functools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

SEED = 11


@functools.lru_cache(maxsize=None)
def reference(ny, nx, cycles, source=None, nu=(2, 2), max_levels=0, init="random"):
    """engine.serial_mg of the workers' problem, once per argument set and never modified:
    ({k: field after k cycles}, [(L2, max) fsum residual after k cycles])."""
    from gpu_mpi_tests_amd import engine

    return engine.serial_mg(ny, nx, cycles, init=init, seed=SEED, source=source, nu=nu, max_levels=max_levels,
                            keep=tuple(range(cycles + 1)))


def run(cfg, env):
    import torch.distributed as dist
    from gpu_mpi_tests_amd import engine

    ny, nx = cfg["ny"], cfg["nx"]
    dims = tuple(cfg["dims"]) if cfg.get("dims") else None

    def make(ny=ny, nx=nx, **over):
        kw = dict(dims=dims, periodic=False, overlap=bool(cfg.get("overlap", False)), graph=bool(cfg.get("graph", False)),
                  tblock=cfg.get("tsteps", 1), push=bool(cfg.get("push", False)), transport=cfg.get("transport", "auto"),
                  init=cfg.get("init", "random"), seed=SEED, source=cfg.get("source"))
        kw.update(over)
        return engine.NativeJacobi(ny, nx, env, **kw)

    def gather(v):
        if env.world_size == 1:
            return [v]
        out = [None] * env.world_size
        dist.all_gather_object(out, v, group=env.host_group)
        return out

    def same(v):
        return len({json.dumps(x, sort_keys=True) for x in gather(v)}) == 1

    fields = {}

    def keep_field(e, tag):
        if not tag:
            return
        parts = gather((e.off_y, e.off_x, e.interior()))  # every rank's share
        if env.rank == 0:
            full = np.full((ny, nx), np.nan)
            for oy, ox, a in parts:
                full[oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
            fields[tag] = full

    def refused(e, kw):
        try:
            e.mg(**kw)
            return None
        except ValueError as err:
            return str(err)

    e = make()
    results = [dict(push=e.push_active, graph=e.graph, graph_fused=e.graph_fused, transport=e.transport,
                    tsteps=e.tsteps, umax=float(e.max_abs_u0))]
    try:
        for op in cfg["ops"]:
            kind = op["op"]
            if kind == "reset":
                e.prepare(1)  # the initial field again
                results.append(None)
            elif kind == "rn":
                rn = e.residual_norm()
                results.append(dict(rn=rn, same=same(rn)))
            elif kind == "mg":
                kw = dict(op["kw"])
                if "nu" in kw:
                    kw["nu"] = tuple(kw["nu"])
                r = e.mg(**kw)
                results.append(dict(res=r, same=same(r)))
                keep_field(e, op.get("tag"))
            elif kind == "run":
                e.run(op["k"])
                e.synchronize()
                results.append(None)
                keep_field(e, op.get("tag"))
            elif kind == "bad":
                results.append([refused(e, kw) is not None for kw in op["kws"]])
            elif kind in ("periodic", "nocoarse"):
                # the refusal comes before any collective: no rank may free its engine while
                # another is still opening its IPC handles in the constructor
                other = make(periodic=True, push=False, graph=False) if kind == "periodic" else make(*op["shape"])
                try:
                    results.append(refused(other, dict(max_cycles=2)))
                finally:
                    gather(True)
                    other.close()
            else:
                raise ValueError(kind)
    finally:
        e.close()
    if env.rank == 0 and cfg.get("out"):
        np.savez(cfg["out"], **fields)
    return results


def main():
    from gpu_mpi_tests_amd.parallel import dist as gd

    cfg = json.loads(sys.argv[1])
    env = gd.init(device=os.environ.get("GMT_TEST_DEVICE", "cpu"))
    res = run(cfg, env)
    if env.rank == 0:
        print(json.dumps(res), flush=True)
    gd.shutdown()


if __name__ == "__main__":
    main()
