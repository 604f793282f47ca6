"""Worker and reference helpers of the conjugate-gradient tests
(tests/test_cg_cpu.py, tests/test_cg_gpu.py).

As a program (one rank on its own, or under torch.distributed.run):
``cg_worker.py '<json config>'`` builds one NativeJacobi on GMT_TEST_DEVICE
(default cpu) and runs the config's ``ops`` on it in order; rank 0 prints one
JSON line with a result per op and saves the gathered fields the ops asked for
into the ``.npz`` file ``out``.  The test judges everything against
``engine.serial_cg`` (helpers below)."""
import functools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

SEED = 11


@functools.lru_cache(maxsize=None)
def reference(ny, nx, iters, init="random", source=None, keep=()):
    """engine.serial_cg of the workers' problem: ({k: field} for k in keep, series)."""
    from gpu_mpi_tests_amd import engine

    return engine.serial_cg(ny, nx, iters, init=init, seed=SEED, source=source, keep=tuple(keep))


def pick_rtol(series, every, lo, norm="l2"):
    """(c, rtol): the first check c >= lo (check i = iteration i * every) that the
    reference series can decide — CG's residual is not monotone, so c must be the
    first check at or below the threshold and every checked value up to c at
    least 2.5% away from it.  The threshold is the geometric mean of r[c] and
    the smallest earlier check."""
    k = 0 if norm == "l2" else 1
    r = [series[i * every][k] for i in range((len(series) - 1) // every + 1)]
    for c in range(max(lo, 1), len(r)):
        prev = min(r[:c])
        if prev / r[c] >= 1.025 ** 2 * 1.01:
            thr = (prev * r[c]) ** 0.5
            assert all(v >= 1.025 * thr for v in r[:c]) and r[c] * 1.025 <= thr
            return c, thr / r[0]
    raise AssertionError(("no decidable check", lo, r))


def run(cfg, env):
    import torch.distributed as dist
    from gpu_mpi_tests_amd import engine

    ny, nx = cfg["ny"], cfg["nx"]
    dims = tuple(cfg["dims"]) if cfg.get("dims") else None

    def make(**over):
        kw = dict(dims=dims, periodic=False, overlap=bool(cfg.get("overlap", False)), graph=bool(cfg.get("graph", False)),
                  tblock=cfg.get("tsteps", 1), push=bool(cfg.get("push", False)), transport=cfg.get("transport", "auto"),
                  init=cfg.get("init", "random"), seed=SEED, source=cfg.get("source"),
                  source_amp=cfg.get("source_amp", 1.0))
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
        parts = gather((e.off_y, e.off_x, e.interior()))
        if env.rank == 0 and tag:
            full = np.full((ny, nx), np.nan)
            for oy, ox, a in parts:
                full[oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
            fields[tag] = full

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
            elif kind == "cg":
                r = e.cg(**op["kw"])
                results.append(dict(res=r, same=same(r)))
                keep_field(e, op.get("tag"))
            elif kind == "run":
                e.run(op["k"])
                e.synchronize()
                results.append(None)
                keep_field(e, op.get("tag"))
            elif kind == "series":
                out = []
                for c in range(1, op["upto"] // op["every"] + 1):
                    e.prepare(1)
                    r = e.cg(max_iters=c * op["every"], check_every=op["every"], lag=0)
                    assert r["iters"] == c * op["every"] and r["checks"] == c + 1 and not r["converged"], r
                    out.append((r["residual"], r["residual_max"], r["r0"]))
                results.append(dict(series=out, same=same(out)))
            elif kind == "bad":
                errors = []
                for kw in op["kws"]:
                    try:
                        e.cg(**kw)
                        errors.append(False)
                    except ValueError:
                        errors.append(True)
                results.append(errors)
            elif kind == "periodic":
                ep = make(periodic=True, push=False, graph=False)
                try:
                    ep.cg(rtol=1e-3, max_iters=10)
                    results.append(False)
                except ValueError:
                    results.append(True)
                finally:
                    # the refusal comes before any collective: no rank may free its engine while
                    # another is still opening its IPC handles in the constructor
                    gather(True)
                    ep.close()
            elif kind == "solve":
                es = make()
                try:
                    r = es.solve(**op["kw"])
                finally:
                    gather(True)
                    es.close()
                results.append(dict(res=r, same=same(r)))
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
