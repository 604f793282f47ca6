"""Worker of the red-black multigrid tests (tests/test_mg_rb_cpu.py,
tests/test_mg_rb_gpu.py).

As a program (one rank on its own, or under torch.distributed.run):
``mg_rb_worker.py '<json config>'`` builds, one after another, a NativeJacobi on
GMT_TEST_DEVICE (default cpu) for every entry of the config's ``engines``
(``ny``, ``nx``, ``tsteps``, ``source``, ``init``, ``ops``) on the process grid
``dims``, and runs the entry's ops on it in order.  Unlike tests/mg_worker.py
one process group serves several engines, so a test that needs many small
problems starts its ranks once.  Ops: ``mg`` (the initial field again, then
``NativeJacobi.mg(**kw)``; the gathered field is kept under ``tag``), ``bad``
(every ``kws`` entry must raise ValueError) and ``capi`` (gmt_engine_jacobi_mg
itself with the given ``smoother`` number: its return code).  Rank 0 prints
one JSON line — per engine every rank's offsets and one result per op — and
saves the fields into the ``.npz`` file ``out``."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from mg_worker import SEED  # noqa: E402


def run(cfg, env):
    import torch.distributed as dist
    from gpu_mpi_tests_amd import engine

    dims = tuple(cfg["dims"]) if cfg.get("dims") else None

    def gather(v):
        if env.world_size == 1:
            return [v]
        out = [None] * env.world_size
        dist.all_gather_object(out, v, group=env.host_group)
        return out

    def same(v):
        return len({json.dumps(x, sort_keys=True) for x in gather(v)}) == 1

    fields, results = {}, []
    for ec in cfg["engines"]:
        ny, nx = ec["ny"], ec["nx"]
        e = engine.NativeJacobi(ny, nx, env, dims=dims, periodic=False, overlap=False, graph=False, tblock=ec.get("tsteps", 1),
                                transport=cfg.get("transport", "auto"), init=ec.get("init", "random"), seed=SEED,
                                source=ec.get("source"))
        res = []
        offsets = gather((int(e.off_y), int(e.off_x)))
        try:
            for op in ec["ops"]:
                kind = op["op"]
                if kind == "mg":
                    kw = dict(op["kw"])
                    if "nu" in kw:
                        kw["nu"] = tuple(kw["nu"])
                    e.prepare(1)  # the initial field again
                    r = e.mg(**kw)
                    res.append(dict(res=r, same=same(r)))
                    if op.get("tag"):
                        parts = gather((e.off_y, e.off_x, e.interior()))  # every rank's share
                        if env.rank == 0:
                            full = np.full((ny, nx), np.nan)
                            for oy, ox, a in parts:
                                full[oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
                            fields[op["tag"]] = full
                elif kind == "bad":
                    out = []
                    for kw in op["kws"]:
                        try:
                            e.mg(**kw)
                            out.append(False)
                        except ValueError:
                            out.append(True)
                    res.append(out)
                elif kind == "capi":
                    o = engine.MgOpts(max_cycles=2, check_every=1, lag=1, nu1=1, nu2=1, omega=1.0,
                                      smoother=int(op["smoother"]))
                    r = engine.MgResult()
                    res.append(int(e.lib.gmt_engine_jacobi_mg(e.h, ctypes.byref(o), ctypes.byref(r))))
                else:
                    raise ValueError(kind)
        finally:
            gather(True)  # no rank frees its engine while another still uses it
            e.close()
        results.append(dict(offsets=offsets, ops=res))
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
