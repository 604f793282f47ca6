"""Fused smoothing of the multigrid cycle (NativeJacobi.mg(fuse=...)) on the GPU:
the assertions of tests/test_mg_fuse_cpu.py — after the cycles interior() is
bitwise engine.serial_mg and bitwise the same engine's fuse = 0 field, r0 and
the residual are the fuse = 0 call's bit for bit — through the engine kinds
whose buffers and transport mg() borrows: a plain engine at one rank (every
level fused), a tsteps = 20 engine at 1 x 2 replaying hipGraphs (the fine level
fused; run() still replays before and after), an inline-halo engine at 2 x 1, a
plain tsteps = 1 engine at 2 x 2 (ghost depth 1: the fine level unfused, the
coarse levels fused), 1 x 2 with a source, and coarsen = "any" at 256 x 768.
Ranks share cuda:0 over IPC.  Every child runs under `timeout`; once a child
has failed nothing further runs on the GPU from this file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import free_port
from gpu_mpi_tests_amd import _native
from mg_worker import SEED, reference
from test_mg_cpu import same_bits
from test_mg_fuse_cpu import CYCLES, NX, NY, VARIANTS, check_pairs, pair_ops, sequence_ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mg_worker.py")
_failed = []


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _launch(cfg, np_):
    if _failed:
        pytest.fail(f"not run: an earlier child failed ({_failed[0]})")
    if np_ == 1:
        cmd = ["timeout", "-k", "10", "150", sys.executable, WORKER, json.dumps(cfg)]
    else:
        cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               "--nproc-per-node", str(np_), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
               WORKER, json.dumps(cfg)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd=ROOT,
                       env=dict(os.environ, OMP_NUM_THREADS="1", GMT_TRANSPORT="ipc", GMT_TEST_DEVICE="cuda"))
    if p.returncode != 0:
        _failed.append(f"rc={p.returncode}")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("[")][-1])


def graph_ops(tsteps, fuse):
    """run() replays before and after an mg() that starts from a swept field."""
    return [dict(op="reset"), dict(op="run", k=2 * tsteps, tag=f"pre_{fuse}"),
            dict(op="mg", tag=f"mid_{fuse}", kw=dict(max_cycles=3, lag=0, fuse=fuse)),
            dict(op="run", k=2 * tsteps, tag=f"post_{fuse}")]


@pytest.mark.parametrize("name,np_,cfg", [
    ("one rank plain", 1, dict(transport="local")),
    ("1x2 fused passes from graphs", 2, dict(dims=(1, 2), tsteps=20, graph=True)),
    ("2x1 inline halo", 2, dict(dims=(2, 1), tsteps=20, push=True)),
    ("2x2 plain", 4, dict(dims=(2, 2))),
    ("1x2 with a source", 2, dict(dims=(1, 2), source="random")),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_fused_cycle_is_the_unfused_cycle(name, np_, cfg, tmp_path):
    from gpu_mpi_tests_amd import engine

    tsteps = cfg.get("tsteps", 1)
    dims = cfg.get("dims") or (1, 1)
    variants = {k: VARIANTS[k] for k in ("v22", "v44", "v32", "d1")}
    ops = pair_ops(variants) + sequence_ops(tsteps, 0) + sequence_ops(tsteps, 2)
    if cfg.get("graph"):
        ops += graph_ops(tsteps, 0) + graph_ops(tsteps, 2)
    out = str(tmp_path / "fields.npz")
    res = _launch(dict(cfg, ny=NY, nx=NX, ops=ops, out=out), np_)
    fields = dict(np.load(out))
    info = res[0]
    check_pairs(res[1:], fields, variants, dims, tsteps)
    nlev = len(engine.mg_levels(NY, NX, dims))
    for tag, nu in (("v22", (2, 2)), ("v44", (4, 4)), ("v32", (3, 2))):
        ref_f, _ = reference(NY, NX, CYCLES, cfg.get("source"), nu, nlev)
        assert same_bits(fields[f"{tag}_{variants[tag][0]}"], ref_f[CYCLES]), tag
    for s in ("s1", "s2", "s3", "s4"):  # mg, run, mg(fuse = 0), mg: what they are without fusing
        assert same_bits(fields[f"{s}_0"], fields[f"{s}_2"]), s
    by_tag = {op["tag"]: r for op, r in zip(ops, res[1:]) if op["op"] == "mg"}
    r = by_tag["v44_4"]["res"]
    if np_ == 1:
        assert (r["fuse_fine"], r["fuse_levels"]) == (4, r["levels"] - 1), r
    else:
        assert r["fuse_fine"] == (1 if tsteps == 1 else 4), r
        assert r["fuse_levels"] == r["levels"] - 1 - (1 if tsteps == 1 else 0), r
    if cfg.get("push"):
        assert info["push"], info
    if cfg.get("graph"):
        assert info["graph_fused"], info
        assert np.array_equal(fields["pre_2"], engine.serial_jacobi(NY, NX, 2 * tsteps, init="random", seed=SEED))
        want, _ = engine.serial_mg(NY, NX, 3, init="random", seed=SEED, start=fields["pre_2"])
        assert same_bits(fields["mid_2"], want) and same_bits(fields["mid_0"], want)
        assert same_bits(fields["post_0"], fields["post_2"])


def test_fused_cycle_any_size(tmp_path):
    """coarsen = "any" at 256 x 768 on 1 x 2 with a fused fine level."""
    from gpu_mpi_tests_amd import engine

    ny, nx, dims, tsteps = 256, 768, (1, 2), 4
    variants = {"a22": (2, dict(max_cycles=CYCLES, nu=(2, 2), coarsen="any")),
                "a43": (4, dict(max_cycles=2, nu=(4, 3), coarsen="any"))}
    out = str(tmp_path / "fields.npz")
    res = _launch(dict(ny=ny, nx=nx, dims=dims, tsteps=tsteps, ops=pair_ops(variants), out=out), 2)
    fields = dict(np.load(out))
    check_pairs(res[1:], fields, variants, dims, tsteps, ny, nx, "any")
    nlev = len(engine.mg_levels(ny, nx, dims, 0, "any"))
    want, _ = engine.serial_mg(ny, nx, CYCLES, init="random", seed=SEED, nu=(2, 2), max_levels=nlev, coarsen="any")
    assert same_bits(fields["a22_2"], want)
