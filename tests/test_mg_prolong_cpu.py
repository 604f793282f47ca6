"""The interpolation fused into the first post-smoothing pass of the multigrid
cycle (NativeJacobi.mg(fuse_prolong=True)) on the CPU backend: tests/mg_worker.py
under torch.distributed.run at 63 x 127 on 1 x 1, 1 x 2, 2 x 2 and 3 x 2 process
grids (the last has ranks that start on odd cells: asserted), and at 255 x 767
and 64 x 64 with coarsen = "any".

Every cell's arithmetic is unchanged, so every comparison is bitwise: after 3
cycles interior() is engine.serial_mg and the same engine's fuse_prolong = False
field, with r0 and the residuals the unfused call's bit for bit, crossed with
fuse in {0, 2, 4}, both smoothers, nu in {(2, 2), (2, 1), (1, 0)} (the last has
no post-smoothing: nothing fuses), fuse_resid on and off, a source and tsteps
1, 2 and 4.  prolong_levels is engine.mg_prolong_levels'; run(k) afterwards
continues from the field."""
import numpy as np
import pytest

from mg_worker import SEED
from test_mg_cpu import launch_cpu, same_bits
from test_mg_resid_cpu import RESULT_KEYS

NY, NX = 63, 127
CYCLES = 3
GRIDS = [(1, None), (2, (1, 2)), (4, (2, 2)), (6, (3, 2))]
NUS = ((2, 2), (2, 1), (1, 0))
COMBOS = [(fuse, sm, nu, fr) for fuse in (0, 2, 4) for sm in ("jacobi", "rb") for nu in NUS for fr in (False, True)]


def tag_of(fuse, sm, nu, fr):
    return f"{sm}{fuse}_{nu[0]}{nu[1]}_{int(fr)}"


def pair_ops(combos, **kw):
    ops = []
    for fuse, sm, nu, fr in combos:
        for fp in (False, True):
            ops += [dict(op="reset"),
                    dict(op="mg", tag=f"{tag_of(fuse, sm, nu, fr)}_{int(fp)}",
                         kw=dict(kw, max_cycles=CYCLES, fuse=fuse, smoother=sm, nu=nu, fuse_resid=fr, fuse_prolong=fp))]
    return ops


def check_pairs(ops, res, fields, combos, ny, nx, dims, tsteps, source=None, coarsen="nested"):
    from gpu_mpi_tests_amd import engine

    by_tag = {op["tag"]: r for op, r in zip(ops, res) if op["op"] == "mg"}
    nlev = len(engine.mg_levels(ny, nx, dims, 0, coarsen))
    refs, seen = {}, []
    for fuse, sm, nu, fr in combos:
        tag = tag_of(fuse, sm, nu, fr)
        plain, fused = by_tag[f"{tag}_0"], by_tag[f"{tag}_1"]
        assert plain["same"] and fused["same"], tag
        for k in RESULT_KEYS:  # r0 and the residuals bit for bit, the same cycle counts
            assert plain["res"][k] == fused["res"][k], (tag, k, plain["res"], fused["res"])
        assert plain["res"]["resid_levels"] == fused["res"]["resid_levels"], tag
        assert same_bits(fields[f"{tag}_0"], fields[f"{tag}_1"]), tag
        want_levels = engine.mg_prolong_levels(ny, nx, dims, tsteps, fuse, nu[1], sm, 0, coarsen)
        assert fused["res"]["fuse_prolong"] is True and fused["res"]["prolong_levels"] == want_levels, (tag, fused["res"])
        assert plain["res"]["fuse_prolong"] is False and plain["res"]["prolong_levels"] == [], plain["res"]
        if (sm, nu) not in refs:
            refs[sm, nu] = engine.serial_mg(ny, nx, CYCLES, init="random", seed=SEED, source=source, nu=nu,
                                            max_levels=nlev, coarsen=coarsen, smoother=sm)[0]
        assert same_bits(fields[f"{tag}_1"], refs[sm, nu]), tag
        seen.append(want_levels)
    return seen


def test_odd_offsets_occur():
    """3 x 2 ranks: a rank of some level starts on an odd global cell in x and in y (px = 0, py = 0 there)."""
    from test_mg_resid_cpu import parities

    px, py = parities(NY, NX, (3, 2))
    assert px == {0, 1} or py == {0, 1}, (px, py)
    assert 0 in py, py  # 63 rows over 3 ranks: rank 1 starts on row 21


# run(k) after the call: (fuse, smoother, nu, fuse_resid).  With tsteps = 2 level 0 has depth 2 on several ranks and
# 4 on one: in the first the fused launch is the whole post-smoothing run (c = n2 = 2), in the second a chunk
# follows it (c = 2 of n2 = 4), in the third a single sweep follows a launch with c = 1
RUN_COMBOS = [(4, "rb", (2, 1), True), (2, "rb", (2, 2), False), (0, "jacobi", (2, 2), True)]


def run_ops():
    ops = []
    for i, (fuse, sm, nu, fr) in enumerate(RUN_COMBOS):
        for fp in (True, False):
            ops += [dict(op="reset"),
                    dict(op="mg", tag=f"runmg{i}_{int(fp)}", kw=dict(max_cycles=CYCLES, fuse=fuse, smoother=sm, nu=nu,
                                                                     fuse_resid=fr, fuse_prolong=fp)),
                    dict(op="run", k=4, tag=f"run{i}_{int(fp)}")]
    return ops


def check_runs(ops, res, fields):
    """run(k) after a call whose level 0 really ran gmt_mg_prolong_smooth gives the field that run(k) gives after
    the unfused call, bit for bit: the fused path leaves the engine's parity and ring state as the pair does."""
    by_tag = {op["tag"]: r for op, r in zip(ops, res) if op["op"] == "mg"}
    for i in range(len(RUN_COMBOS)):
        levels = by_tag[f"runmg{i}_1"]["res"]["prolong_levels"]
        assert levels and levels[0] == 0, (i, levels)
        assert by_tag[f"runmg{i}_0"]["res"]["prolong_levels"] == [], i
        assert same_bits(fields[f"runmg{i}_1"], fields[f"runmg{i}_0"]), i
        assert same_bits(fields[f"run{i}_1"], fields[f"run{i}_0"]), i
        assert not same_bits(fields[f"run{i}_1"], fields[f"runmg{i}_1"]) and np.isfinite(fields[f"run{i}_1"]).all(), i


@pytest.mark.parametrize("np_,dims", GRIDS, ids=lambda v: None if isinstance(v, int) else str(v))
def test_fused_prolong_is_the_two_kernels(np_, dims, tmp_path):
    out = str(tmp_path / "fields.npz")
    ops = pair_ops(COMBOS) + run_ops()
    res = launch_cpu(dict(ny=NY, nx=NX, dims=dims, tsteps=2, ops=ops, out=out), np_, "ipc" if np_ == 4 else "rccl")
    fields = dict(np.load(out))
    d = dims or (1, 1)
    seen = check_pairs(ops, res[1:], fields, COMBOS, NY, NX, d, 2)
    assert any(lv and lv[0] == 0 for lv in seen) and [] in seen, seen  # the fine level fuses; nu2 = 0 fuses nothing
    check_runs(ops, res[1:], fields)
    # an unfused call after fused ones is what it was before them
    assert same_bits(fields["runmg0_0"], fields[f"{tag_of(*RUN_COMBOS[0])}_0"])


@pytest.mark.parametrize("np_,dims", [(1, None), (4, (2, 2))], ids=lambda v: None if isinstance(v, int) else str(v))
def test_with_a_source(np_, dims, tmp_path):
    out = str(tmp_path / "fields.npz")
    combos = [(fuse, sm, nu, fr) for fuse in (0, 4) for sm in ("jacobi", "rb") for nu in NUS[:2] for fr in (False, True)]
    ops = pair_ops(combos)
    res = launch_cpu(dict(ny=NY, nx=NX, dims=dims, tsteps=2, source="random", ops=ops, out=out), np_)
    check_pairs(ops, res[1:], dict(np.load(out)), combos, NY, NX, dims or (1, 1), 2, "random")


@pytest.mark.parametrize("tsteps", [1, 4])
def test_ghost_depths(tsteps, tmp_path):
    """tsteps = 1 keeps level 0 at depth 1 on several ranks (c = 1: no exchange of u at all); tsteps = 4 lets a
    4-deep chunk run on the fine level."""
    from gpu_mpi_tests_amd import engine

    out = str(tmp_path / "fields.npz")
    combos = [(fuse, sm, nu, fr) for fuse in (0, 4) for sm in ("jacobi", "rb") for nu in ((2, 2), (1, 2))
              for fr in (False, True)]
    ops = pair_ops(combos)
    res = launch_cpu(dict(ny=NY, nx=NX, dims=(2, 2), tsteps=tsteps, ops=ops, out=out), 4)
    check_pairs(ops, res[1:], dict(np.load(out)), combos, NY, NX, (2, 2), tsteps)
    assert engine.mg_fuse_depths(NY, NX, (2, 2), 4, tsteps)[0] == tsteps


@pytest.mark.parametrize("ny,nx,np_,dims", [(255, 767, 1, None), (255, 767, 4, (2, 2)), (64, 64, 1, None),
                                            (64, 64, 4, (2, 2))])
def test_any_size_fuses_the_nested_levels(ny, nx, np_, dims, tmp_path):
    from gpu_mpi_tests_amd import engine

    out = str(tmp_path / "fields.npz")
    combos = [(2, "rb", (2, 2), True), (0, "jacobi", (2, 1), False), (4, "jacobi", (2, 2), False)]
    ops = pair_ops(combos, coarsen="any")
    res = launch_cpu(dict(ny=ny, nx=nx, dims=dims, tsteps=2, ops=ops, out=out), np_)
    d = dims or (1, 1)
    seen = check_pairs(ops, res[1:], dict(np.load(out)), combos, ny, nx, d, 2, None, "any")
    table = engine.mg_levels(ny, nx, d, 0, "any")
    tab = [l for l, (my, mx) in enumerate(table[:-1]) if my % 2 == 0 or mx % 2 == 0]
    for levels in seen:
        assert levels and not set(levels) & set(tab), (levels, tab)  # table-driven levels stay unfused
    if ny == 64:
        assert tab and tab[0] == 0 and 1 in seen[0], (tab, seen)     # the nested ones below them fuse


def test_residual_series(tmp_path):
    """Three calls of one cycle each: the residual after every cycle is the unfused engine's, bit for bit."""
    kw = dict(max_cycles=1, fuse=2, smoother="rb", fuse_resid=True)
    ops = [dict(op="reset")] + [dict(op="mg", tag=f"p{i}", kw=dict(kw, fuse_prolong=False)) for i in range(3)] + \
          [dict(op="reset")] + [dict(op="mg", tag=f"f{i}", kw=dict(kw, fuse_prolong=True)) for i in range(3)]
    out = str(tmp_path / "fields.npz")
    res = launch_cpu(dict(ny=NY, nx=NX, dims=(2, 2), tsteps=2, ops=ops, out=out), 4)[1:]
    fields = dict(np.load(out))
    for i in range(3):
        p, f = res[1 + i], res[5 + i]
        for k in RESULT_KEYS:
            assert p["res"][k] == f["res"][k], (i, k, p["res"], f["res"])
        assert same_bits(fields[f"p{i}"], fields[f"f{i}"]), i


def test_refusals():
    """fuse_prolong takes False or True only (the engine's own 0-or-1 check: test_c_api_refuses_other_values)."""
    bad = [dict(max_cycles=2, fuse_prolong=2), dict(max_cycles=2, fuse_prolong=-1), dict(max_cycles=2, fuse_prolong="yes")]
    ok = [dict(max_cycles=2, fuse_prolong=True), dict(max_cycles=2, fuse_prolong=0)]
    res = launch_cpu(dict(ny=NY, nx=NX, dims=None, ops=[dict(op="bad", kws=bad), dict(op="bad", kws=ok)]), 1)
    assert res[1] == [True, True, True] and res[2] == [False, False], res[1:]


_C_API = """
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from gpu_mpi_tests_amd import engine
from gpu_mpi_tests_amd.parallel import dist as gd
env = gd.init(device="cpu")
e = engine.NativeJacobi(63, 127, env, periodic=False, init="random", seed=1)
codes = []
for v in (0, 1, 2, -1):
    e.prepare(1)
    o = engine.MgOpts(max_cycles=1, check_every=1, lag=1, nu1=2, nu2=2, omega=0.8, fuse_prolong=v)
    r = engine.MgResult()
    codes.append([int(e.lib.gmt_engine_jacobi_mg(e.h, ctypes.byref(o), ctypes.byref(r))), r.fuse_prolong, r.prolong_levels])
e.close()
print(json.dumps(codes))
gd.shutdown()
"""


def test_c_api_refuses_other_values():
    """gmt_engine_jacobi_mg through the C structs: fuse_prolong 0 and 1 run (and are reported), 2 and -1 are
    refused with code 1 by JacobiSolver::mg's own check, which Python's bool never reaches."""
    import json
    import os
    import subprocess
    import sys

    from native_util import ROOT, ensure_host_build

    ensure_host_build()
    p = subprocess.run([sys.executable, "-c", _C_API, ROOT], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", GMT_TEST_DEVICE="cpu"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    codes = json.loads(p.stdout.strip().splitlines()[-1])
    nlev = 5  # 63 x 127: 63, 31, 15, 7, 3, 1 rows
    assert codes[0] == [0, 0, 0] and codes[1][:2] == [0, 1] and codes[1][2] == nlev, codes
    assert [c[0] for c in codes[2:]] == [1, 1], codes
