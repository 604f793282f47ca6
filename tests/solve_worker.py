"""Worker and NumPy references of the residual_norm / solve tests
(tests/test_solve_cpu.py, tests/test_solve_gpu.py).

As a program (one rank on its own, or under torch.distributed.run):
``solve_worker.py '<json config>'`` builds one NativeJacobi on GMT_TEST_DEVICE
(default cpu), runs the residual_norm sequence and every solve case of the
config, and rank 0 prints one JSON line.  Every solve case starts from the
initial field (prepare() restores it).  The fields are compared bitwise with
the serial NumPy solve here; the residuals and the solve results are judged
by the test against the references below."""
import functools
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

SEED = 11


def _resid(u, periodic):
    """(L2, max) of d = J(u) - u over the interior of the ghosted field u."""
    if periodic:
        u[1:-1, 0] = u[1:-1, -2]
        u[1:-1, -1] = u[1:-1, 1]
        u[0, 1:-1] = u[-2, 1:-1]
        u[-1, 1:-1] = u[1, 1:-1]
    d = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1])) - u[1:-1, 1:-1]
    return math.sqrt(math.fsum((d * d).ravel().tolist())), float(np.abs(d).max())


@functools.lru_cache(maxsize=None)
def ref_residuals(ny, nx, periodic, sweeps):
    """{s: (L2, max)} of the serial solve (random init, seed SEED) at every sweep count in `sweeps`."""
    from gpu_mpi_tests_amd import engine

    u = engine.initial_field(ny, nx, "random", SEED)
    un = u.copy()
    out = {}
    for s in range(max(sweeps) + 1):
        if s in sweeps:
            out[s] = _resid(u, periodic)
        if periodic:
            u[1:-1, 0] = u[1:-1, -2]
            u[1:-1, -1] = u[1:-1, 1]
            u[0, 1:-1] = u[-2, 1:-1]
            u[-1, 1:-1] = u[1, 1:-1]
        un[1:-1, 1:-1] = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1]))
        u, un = un, u
    return out


def pick_rtol(ny, nx, periodic, every, c, norm="l2"):
    """rtol that the reference series r[i] (residual after i * every sweeps)
    first meets at check c: the geometric mean of r[c-1] and r[c] over r[0].
    The reference's own r[c] / r[c-1] must be <= 0.95, so the crossing sits at
    least 2.5% from either neighbour (summation order moves a value by 1e-11)."""
    k = 0 if norm == "l2" else 1
    ser = ref_residuals(ny, nx, periodic, tuple(i * every for i in range(c + 1)))
    r = [ser[i * every][k] for i in range(c + 1)]
    assert r[c] / r[c - 1] <= 0.95, (ny, nx, periodic, every, c, r)
    assert all(r[i] > r[c - 1] for i in range(c - 1)), r  # no earlier check meets it
    return math.sqrt(r[c - 1] * r[c]) / r[0], r


def run(cfg, env):
    """The residual_norm sequence and the solve cases of cfg on one engine; every rank calls it."""
    import torch.distributed as dist
    from gpu_mpi_tests_amd import engine

    ny, nx, periodic = cfg["ny"], cfg["nx"], bool(cfg.get("periodic", False))
    dims = tuple(cfg["dims"]) if cfg.get("dims") else None
    e = engine.NativeJacobi(ny, nx, env, dims=dims, periodic=periodic, overlap=bool(cfg.get("overlap", False)),
                            graph=bool(cfg.get("graph", False)), tblock=cfg.get("tsteps", 1),
                            push=bool(cfg.get("push", False)), transport=cfg.get("transport", "auto"),
                            init="random", seed=SEED)

    def gather(v):
        if env.world_size == 1:
            return [v]
        out = [None] * env.world_size
        dist.all_gather_object(out, v, group=env.host_group)
        return out

    def field_equal(sweeps):
        parts = gather((e.off_y, e.off_x, e.interior()))
        if env.rank != 0:
            return None
        full = np.full((ny, nx), np.nan)
        for oy, ox, a in parts:
            full[oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
        return bool(np.array_equal(full, engine.serial_jacobi(ny, nx, sweeps, periodic, init="random", seed=SEED)))

    res = dict(push=e.push_active, graph_fused=e.graph_fused, band_first=e.band_first, transport=e.transport,
               tsteps=e.tsteps)
    try:
        # residual_norm: read-only, repeatable, at sweep counts that are and are not multiples of tsteps
        n1, n2 = cfg.get("pre", (0, 0))
        before = e.interior()
        rn = [e.residual_norm(), e.residual_norm()]
        res["unchanged"] = all(gather(bool(np.array_equal(before, e.interior()))))
        e.run(n1)
        rn.append(e.residual_norm())
        e.run(n2)
        e.synchronize()
        res["run_equal"] = field_equal(n1 + n2)
        res["rn"] = rn
        res["rn_same"] = len({json.dumps(v) for v in gather(rn)}) == 1
        cases = []
        for c in cfg.get("cases", ()):
            every = c.get("check_every", 0) or e.tsteps
            e.prepare(every)  # the initial field again
            r = e.solve(tol=c.get("tol", 0.0), rtol=c.get("rtol", 0.0), norm=c.get("norm", "l2"),
                        max_sweeps=c["max_sweeps"], check_every=c.get("check_every", 0), lag=c.get("lag", 1))
            same = len({json.dumps(v, sort_keys=True) for v in gather(r)}) == 1
            cases.append(dict(res=r, same=same, equal=field_equal(r["sweeps"])))
        res["cases"] = cases
        errors = []
        for kw in cfg.get("bad", ()):
            try:
                e.solve(**kw)
                errors.append(False)
            except ValueError:
                errors.append(True)
        res["bad"] = errors
    finally:
        e.close()
    return res


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
