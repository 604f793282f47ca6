"""The fused residual + restriction of the multigrid cycle
(NativeJacobi.mg(fuse_resid=True)) on the CPU backend: tests/mg_worker.py under
torch.distributed.run at 63 x 127 on 1 x 1, 2 x 1, 2 x 2, 3 x 2 and 2 x 3
process grids with tsteps = 2.  The 2 x 3 grid is added to the four of the
issue because the first coarse column of a rank is at region index 0 only where
a rank starts on an odd column, which 127 columns over 1 or 2 process columns
never give; the test asserts that both values of px and of py occur.

Every cell's arithmetic is unchanged, so every comparison is bitwise: after 3
cycles interior() is engine.serial_mg and the same engine's fuse_resid = False
field, with r0 and the residuals the unfused call's bit for bit, crossed with
fuse in {0, 2, 4}, both smoothers and a source.  resid_levels is
engine.mg_resid_levels'.  tsteps = 1 on 2 x 2 keeps level 0 unfused and fuses
the coarse levels; 64 x 64 with coarsen = "any" keeps the table-driven level 0
unfused and fuses the rest; run(k) afterwards continues from the field."""
import numpy as np
import pytest

from mg_worker import SEED
from test_mg_cpu import launch_cpu, same_bits

NY, NX = 63, 127
CYCLES = 3
GRIDS = [(1, None), (2, (2, 1)), (4, (2, 2)), (6, (3, 2)), (6, (2, 3))]
RESULT_KEYS = ("converged", "iters", "checks", "residual_iters", "residual", "residual_max", "r0", "failed", "levels",
               "fuse", "fuse_fine", "fuse_levels")
COMBOS = [(fuse, sm) for fuse in (0, 2, 4) for sm in ("jacobi", "rb")]


def pair_ops(combos, **kw):
    ops = []
    for fuse, sm in combos:
        for fr in (False, True):
            ops += [dict(op="reset"), dict(op="mg", tag=f"{sm}{fuse}_{int(fr)}",
                                           kw=dict(kw, max_cycles=CYCLES, fuse=fuse, smoother=sm, fuse_resid=fr))]
    return ops


def check_pairs(ops, res, fields, combos, ny, nx, dims, tsteps, source=None, coarsen="nested"):
    from gpu_mpi_tests_amd import engine

    by_tag = {op["tag"]: r for op, r in zip(ops, res) if op["op"] == "mg"}
    want_levels = engine.mg_resid_levels(ny, nx, dims, tsteps, 0, coarsen)
    nlev = len(engine.mg_levels(ny, nx, dims, 0, coarsen))
    for fuse, sm in combos:
        tag = f"{sm}{fuse}"
        plain, fused = by_tag[f"{tag}_0"], by_tag[f"{tag}_1"]
        assert plain["same"] and fused["same"], tag
        for k in RESULT_KEYS:  # r0 and the residuals bit for bit, the same cycle counts
            assert plain["res"][k] == fused["res"][k], (tag, k, plain["res"], fused["res"])
        assert same_bits(fields[f"{tag}_0"], fields[f"{tag}_1"]), tag
        assert fused["res"]["fuse_resid"] is True and fused["res"]["resid_levels"] == want_levels, (tag, fused["res"])
        assert plain["res"]["fuse_resid"] is False and plain["res"]["resid_levels"] == [], plain["res"]
        want, _ = engine.serial_mg(ny, nx, CYCLES, init="random", seed=SEED, source=source, max_levels=nlev,
                                   coarsen=coarsen, smoother=sm)
        assert same_bits(fields[f"{tag}_1"], want), tag
    return want_levels


def parities(ny, nx, dims):
    """The (px, py) of every rank on every restricting level: 1 where its share starts on an even global cell."""
    from gpu_mpi_tests_amd import engine

    shares = []
    levels = engine.mg_levels(ny, nx, dims, 0, "nested", shares)
    px, py = set(), set()
    for by, bx in shares[:len(levels) - 1]:
        py |= {1 - b % 2 for b in by[:-1]}
        px |= {1 - b % 2 for b in bx[:-1]}
    return px, py


def test_both_parities_occur():
    px, py = set(), set()
    for _, dims in GRIDS:
        a, b = parities(NY, NX, dims or (1, 1))
        px |= a
        py |= b
    assert px == {0, 1} and py == {0, 1}, (px, py)
    four = [parities(NY, NX, d or (1, 1)) for _, d in GRIDS[:4]]  # the issue's four grids leave px = 0 out
    assert set().union(*(p for p, _ in four)) == {1}


@pytest.mark.parametrize("source", [None, "random"])
@pytest.mark.parametrize("np_,dims", GRIDS, ids=lambda v: None if isinstance(v, int) else str(v))
def test_fused_transfer_is_the_two_kernels(np_, dims, source, tmp_path):
    out = str(tmp_path / "fields.npz")
    ops = pair_ops(COMBOS) + [dict(op="run", k=4, tag="run_1"), dict(op="reset"),
                              dict(op="mg", tag="again_0", kw=dict(max_cycles=CYCLES, fuse=4, smoother="rb")),
                              dict(op="run", k=4, tag="run_0")]
    res = launch_cpu(dict(ny=NY, nx=NX, dims=dims, tsteps=2, source=source, ops=ops, out=out), np_, "ipc" if np_ == 4 else "rccl")
    fields = dict(np.load(out))
    d = dims or (1, 1)
    levels = check_pairs(ops, res[1:], fields, COMBOS, NY, NX, d, 2, source)
    assert levels and levels[0] == 0, levels  # the fine level fuses: ghost depth 2
    # run(k) after the fused call continues from its field; an unfused call after fused ones is what it was
    assert same_bits(fields["again_0"], fields["rb4_0"]) and same_bits(fields["run_0"], fields["run_1"])
    assert not same_bits(fields["run_1"], fields["rb4_1"])


def test_ghost_depth_one_keeps_level_0_unfused(tmp_path):
    from gpu_mpi_tests_amd import engine

    out = str(tmp_path / "fields.npz")
    combos = [(2, "jacobi"), (0, "rb")]
    ops = pair_ops(combos)
    res = launch_cpu(dict(ny=NY, nx=NX, dims=(2, 2), tsteps=1, ops=ops, out=out), 4)
    levels = check_pairs(ops, res[1:], dict(np.load(out)), combos, NY, NX, (2, 2), 1)
    nlev = len(engine.mg_levels(NY, NX, (2, 2)))
    assert levels == list(range(1, nlev - 1)) and len(levels) >= 2, levels


@pytest.mark.parametrize("np_,dims", [(1, None), (4, (2, 2))], ids=lambda v: None if isinstance(v, int) else str(v))
def test_any_size_fuses_the_nested_levels(np_, dims, tmp_path):
    from gpu_mpi_tests_amd import engine

    out = str(tmp_path / "fields.npz")
    combos = [(2, "rb"), (0, "jacobi")]
    ops = pair_ops(combos, coarsen="any")
    res = launch_cpu(dict(ny=64, nx=64, dims=dims, tsteps=2, ops=ops, out=out), np_)
    d = dims or (1, 1)
    levels = check_pairs(ops, res[1:], dict(np.load(out)), combos, 64, 64, d, 2, None, "any")
    table = engine.mg_levels(64, 64, d, 0, "any")
    assert table[0] == (64, 64) and table[1] == (31, 31), table
    if np_ == 1:
        assert levels == list(range(1, len(table) - 1)) and len(levels) >= 2, (levels, table)
    else:
        assert 0 not in levels and 1 in levels, (levels, table)


def test_refusals():
    bad = [dict(max_cycles=2, fuse_resid=True, fuse=1)]
    res = launch_cpu(dict(ny=NY, nx=NX, dims=None, ops=[dict(op="bad", kws=bad)]), 1)
    assert res[1] == [True], res[1]


def test_model_rule():
    from gpu_mpi_tests_amd import engine

    assert engine.mg_resid_levels(63, 127, (1, 1), 1) == [0, 1, 2, 3, 4]
    assert engine.mg_resid_levels(63, 127, (2, 2), 1) == [1, 2, 3]      # level 4 leaves a rank one row
    assert engine.mg_resid_levels(63, 127, (2, 2), 2) == [0, 1, 2, 3]
    assert engine.mg_resid_levels(64, 64, (1, 1), 2, 0, "any") == [1, 2, 3, 4]    # 64 -> 31: level 0 goes by tables
    assert engine.mg_resid_levels(63, 127, (1, 1), 1, 3) == [0, 1]
