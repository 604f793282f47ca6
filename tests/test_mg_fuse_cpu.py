"""Fused smoothing of the multigrid cycle (NativeJacobi.mg(fuse=...)) on the CPU
backend: tests/mg_worker.py under torch.distributed.run at 255 x 767 on 1, 2, 4
and 6 ranks over the host emulations of RCCL and IPC, on a plain engine
(tsteps = 1: ghost depth 1, so on several ranks the fine level stays unfused
and the coarse levels fuse) and on a tsteps = 4 engine (the fine level fuses).

Every cell's arithmetic is unchanged, so every comparison is bitwise: after 3
cycles interior() is engine.serial_mg and the same engine's fuse = 0 field, r0
and the residual are the fuse = 0 call's bit for bit — for fuse = 2 with
nu = (2, 2), fuse = 4 with nu = (4, 4) (the 7-row level of a grid with two
process rows has depth 3: chunks 3 + 1), fuse = 2 with nu = (3, 2) (chunks
2 + 1, an odd sweep count: the parity flips), max_levels = 3, a random source,
and coarsen = "any" at 256 x 768.  With rtol = 1e-6 the fused call stops at the
fuse = 0 call's cycle for lag 0 and 1 (tests/test_mg_cpu.py establishes the
condition on the reference).  A second mg() call, run(k) after mg() and a
fuse = 0 call after a fused one are what they are without fusing.  The reported
depths are engine.mg_fuse_depths'."""
import numpy as np
import pytest

from mg_worker import SEED, reference
from test_mg_cpu import CAP, RTOL, launch_cpu, same_bits

NY, NX = 255, 767
CYCLES = 3
GRIDS = [(1, None, "rccl"), (2, (1, 2), "rccl"), (2, (2, 1), "rccl"), (4, (2, 2), "rccl"), (6, (2, 3), "rccl"),
         (2, (1, 2), "ipc"), (4, (2, 2), "ipc")]
# tag -> mg() options, run once with fuse = 0 and once fused
VARIANTS = {"v22": (2, dict(max_cycles=CYCLES, nu=(2, 2))), "v44": (4, dict(max_cycles=CYCLES, nu=(4, 4))),
            "v32": (2, dict(max_cycles=CYCLES, nu=(3, 2))), "l3": (2, dict(max_cycles=2, max_levels=3)),
            "d0": (2, dict(rtol=RTOL, max_cycles=CAP, lag=0)), "d1": (2, dict(rtol=RTOL, max_cycles=CAP, lag=1))}
RESULT_KEYS = ("converged", "iters", "checks", "residual_iters", "residual", "residual_max", "r0", "failed", "levels")


def pair_ops(variants):
    ops = []
    for tag, (fuse, kw) in variants.items():
        for f in (0, fuse):
            ops += [dict(op="reset"), dict(op="mg", tag=f"{tag}_{f}", kw=dict(kw, fuse=f))]
    return ops


def sequence_ops(tsteps, fuse):
    """mg, run, mg with the other setting, mg again: the same fields whatever `fuse` is."""
    return [dict(op="reset"), dict(op="mg", tag=f"s1_{fuse}", kw=dict(max_cycles=2, fuse=fuse)),
            dict(op="run", k=3 * tsteps, tag=f"s2_{fuse}"),
            dict(op="mg", tag=f"s3_{fuse}", kw=dict(max_cycles=2, fuse=0)),
            dict(op="mg", tag=f"s4_{fuse}", kw=dict(max_cycles=1, nu=(1, 2), fuse=fuse))]


def check_pairs(res, fields, variants, dims, tsteps, ny=NY, nx=NX, coarsen="nested"):
    from gpu_mpi_tests_amd import engine

    ops = pair_ops(variants)
    by_tag = {op["tag"]: r for op, r in zip(ops, res) if op["op"] == "mg"}
    for tag, (fuse, kw) in variants.items():
        plain, fused = by_tag[f"{tag}_0"], by_tag[f"{tag}_{fuse}"]
        assert plain["same"] and fused["same"], tag
        for k in RESULT_KEYS:  # r0 and the residuals bit for bit, the same cycle counts and decision
            assert plain["res"][k] == fused["res"][k], (tag, k, plain["res"], fused["res"])
        assert same_bits(fields[f"{tag}_0"], fields[f"{tag}_{fuse}"]), tag
        depths = engine.mg_fuse_depths(ny, nx, dims, fuse, tsteps, kw.get("max_levels", 0), coarsen)
        r = fused["res"]
        assert len(depths) == r["levels"] - 1, (tag, depths, r)
        assert (r["fuse"], r["fuse_fine"], r["fuse_levels"]) == (fuse, depths[0], sum(d >= 2 for d in depths)), (tag, r)
        assert (plain["res"]["fuse"], plain["res"]["fuse_fine"], plain["res"]["fuse_levels"]) == (0, 1, 0), plain


@pytest.mark.parametrize("tsteps", [1, 4])
@pytest.mark.parametrize("np_,dims,transport", GRIDS, ids=lambda v: None if isinstance(v, int) else str(v))
def test_fused_cycle_is_the_unfused_cycle(np_, dims, transport, tsteps, tmp_path):
    from gpu_mpi_tests_amd import engine

    out = str(tmp_path / "fields.npz")
    ops = pair_ops(VARIANTS) + sequence_ops(tsteps, 0) + sequence_ops(tsteps, 2)
    res = launch_cpu(dict(ny=NY, nx=NX, dims=dims, tsteps=tsteps, ops=ops, out=out), np_, transport)
    fields = dict(np.load(out))
    d = dims or (1, 1)
    check_pairs(res[1:], fields, VARIANTS, d, tsteps)
    # against the definition
    nlev = len(engine.mg_levels(NY, NX, d))
    for tag, nu, cycles, levels in (("v22", (2, 2), CYCLES, nlev), ("v44", (4, 4), CYCLES, nlev),
                                    ("v32", (3, 2), CYCLES, nlev), ("l3", (2, 2), 2, 3)):
        ref_f, _ = reference(NY, NX, cycles, None, nu, levels)
        assert same_bits(fields[f"{tag}_{VARIANTS[tag][0]}"], ref_f[cycles]), tag
    # the decision falls at the same cycle (compared key by key above) and has converged
    by_tag = {op["tag"]: r for op, r in zip(ops, res[1:]) if op["op"] == "mg"}
    for lag in (0, 1):
        r = by_tag[f"d{lag}_2"]["res"]
        assert r["converged"] == 1 and r["iters"] == min(r["residual_iters"] + lag, CAP), r
    # mg, run, mg(fuse = 0), mg: what they are without fusing
    for s in ("s1", "s2", "s3", "s4"):
        assert same_bits(fields[f"{s}_0"], fields[f"{s}_2"]), s
    # the depths the issue derives by hand: fine level capped by the ghost depth, the 7-row level by its shares
    r = by_tag["v44_4"]["res"]
    if np_ == 1:
        assert (r["fuse_fine"], r["fuse_levels"]) == (4, r["levels"] - 1), r
    else:
        assert r["fuse_fine"] == (1 if tsteps == 1 else 4), r
        # the 7-row level of two process rows has depth 3: still fused
        assert r["fuse_levels"] == r["levels"] - 1 - (1 if tsteps == 1 else 0), r


@pytest.mark.parametrize("tsteps", [1, 4])
@pytest.mark.parametrize("np_,dims,transport", GRIDS, ids=lambda v: None if isinstance(v, int) else str(v))
def test_fused_cycle_with_a_source(np_, dims, transport, tsteps, tmp_path):
    from gpu_mpi_tests_amd import engine

    out = str(tmp_path / "fields.npz")
    variants = {"v22": VARIANTS["v22"], "v32": VARIANTS["v32"]}
    ops = pair_ops(variants) + sequence_ops(tsteps, 0) + sequence_ops(tsteps, 2)
    res = launch_cpu(dict(ny=NY, nx=NX, dims=dims, tsteps=tsteps, source="random", ops=ops, out=out), np_, transport)
    fields = dict(np.load(out))
    d = dims or (1, 1)
    check_pairs(res[1:], fields, variants, d, tsteps)
    nlev = len(engine.mg_levels(NY, NX, d))
    for tag, nu in (("v22", (2, 2)), ("v32", (3, 2))):
        ref_f, _ = reference(NY, NX, CYCLES, "random", nu, nlev)
        assert same_bits(fields[f"{tag}_2"], ref_f[CYCLES]), tag
    for s in ("s1", "s2", "s3", "s4"):
        assert same_bits(fields[f"{s}_0"], fields[f"{s}_2"]), s


@pytest.mark.parametrize("np_,dims,transport,tsteps", [(1, None, "rccl", 1), (2, (2, 1), "rccl", 4), (4, (2, 2), "ipc", 1),
                                                       (6, (2, 3), "rccl", 4)],
                         ids=lambda v: None if isinstance(v, int) else str(v))
def test_fused_cycle_any_size(np_, dims, transport, tsteps, tmp_path):
    """coarsen = "any" at 256 x 768: table-driven transfers between fused levels."""
    from gpu_mpi_tests_amd import engine

    ny, nx = 256, 768
    out = str(tmp_path / "fields.npz")
    variants = {"a22": (2, dict(max_cycles=CYCLES, nu=(2, 2), coarsen="any")),
                "a43": (4, dict(max_cycles=2, nu=(4, 3), coarsen="any"))}
    ops = pair_ops(variants)
    res = launch_cpu(dict(ny=ny, nx=nx, dims=dims, tsteps=tsteps, ops=ops, out=out), np_, transport)
    fields = dict(np.load(out))
    d = dims or (1, 1)
    check_pairs(res[1:], fields, variants, d, tsteps, ny, nx, "any")
    nlev = len(engine.mg_levels(ny, nx, d, 0, "any"))
    want, _ = engine.serial_mg(ny, nx, CYCLES, init="random", seed=SEED, nu=(2, 2), max_levels=nlev, coarsen="any")
    assert same_bits(fields["a22_2"], want)


def test_refusals():
    bad = [dict(max_cycles=2, fuse=1), dict(max_cycles=2, fuse=5), dict(max_cycles=2, fuse=-1)]
    for np_, dims in ((1, None), (2, (1, 2))):
        res = launch_cpu(dict(ny=NY, nx=NX, dims=dims, ops=[dict(op="bad", kws=bad)]), np_)
        assert res[1] == [True] * len(bad), res[1]
