"""``mpi_stencil2d_gt --overlap`` and ``engine.deriv_step_bench`` on the host
backend: whole steps (halo exchange + derivative) in the serial and the
overlapped order (gmt/deriv.hpp), the overlapped one through
gmt_stencil5_2d_interior / gmt_stencil5_2d_edges.

With --check the field is raised by 1.0 before every exchange and every
overlapped step's derivative is compared with the analytic one: a ghost cell
the edges read too early, or one left from an earlier step, moves an edge
value by scale / 12 = n_global / 96, and ``step_err`` is held against half of
that.  The corruption case shows the check is not vacuous.
"""
import re

import pytest

from conftest import free_port
from native_util import ensure_host_build, have_mpi, run_app

mpi = pytest.mark.skipif(not have_mpi(), reason="mpirun not available")

N_LOCAL = 64
ARGS = ("mpi_stencil2d_gt", str(N_LOCAL), "20", "--no-managed", "--tests=deriv", "--n-other=512", "--check")
TEST_RE = r"^TEST dim:(\d), device , buf:(\d); [0-9.]+, err=([0-9.]+)"
STEP_RE = (r"^STEP dim:(\d), device , buf:(\d); serial=([0-9.]+), overlap=([0-9.]+), step_err=([0-9.]+) "
           r"\[([\w-]+)\]$")


def _lines(out):
    return re.findall(TEST_RE, out, re.M), re.findall(STEP_RE, out, re.M)


@mpi
@pytest.mark.parametrize("transport", ["mpi-host", "mpi-direct"])
@pytest.mark.parametrize("np_", [1, 2, 3])
def test_overlapped_steps_compute_the_derivative(np_, transport):
    plain = run_app(*ARGS, f"--transport={transport}", np=np_).stdout
    out = run_app(*ARGS, f"--transport={transport}", "--overlap", np=np_).stdout  # exit status 0
    tests0, steps0 = _lines(plain)
    tests, steps = _lines(out)
    # without the flag: the reference's lines alone
    assert len(tests0) == 4 and not steps0 and "STEP" not in plain, plain
    # one STEP line after each TEST line, for the same test
    assert len(tests) == 4 and len(steps) == 4, out
    assert [t[:2] for t in tests] == [s[:2] for s in steps], out
    kinds = [ln.split(" ", 1)[0] for ln in out.splitlines() if ln.startswith(("TEST", "STEP"))]
    assert kinds == ["TEST", "STEP"] * 4, out
    threshold = N_LOCAL * np_ / 192
    for (_, _, err), (_, _, serial, overlap, step_err, tag), (_, _, err0) in zip(tests, steps, tests0):
        print(f"np {np_} {transport}: err {err} (serial order {err0}), step_err {step_err}, threshold {threshold}")
        assert tag == transport
        assert float(serial) > 0 and float(overlap) > 0
        assert float(step_err) < threshold, out
        # the last overlapped step's err_norm against the serial run's, on
        # test_app_stencil2d_gt_err_norm's bar
        assert float(err) < 1e-5 and float(err0) < 1e-5 and abs(float(err) - float(err0)) < 1e-5, out
    assert len(re.findall(r"# halo check dim:\d buf:\d \([\w-]+\): 0 bad ghost cells, 50 exchanges", out)) == 4, out


@mpi
@pytest.mark.parametrize("np_", [2, 3])
def test_stale_ghost_cell_in_an_overlapped_step_is_caught(np_):
    """GMT_CORRUPT_GHOST=1:3: rank 1 puts one ghost cell back to the last
    step's value between finish() and the edges kernel of iteration 3: exit
    status 5, and step_err above the threshold in every test."""
    p = run_app(*ARGS, "--transport=mpi-host", "--overlap", np=np_, env={"GMT_CORRUPT_GHOST": "1:3"}, check=False)
    assert p.returncode == 5, p.stdout + p.stderr
    _, steps = _lines(p.stdout)
    assert len(steps) == 4, p.stdout
    threshold = N_LOCAL * np_ / 192
    for s in steps:
        print(f"np {np_}: step_err {s[4]}, threshold {threshold}")
        assert float(s[4]) > threshold, p.stdout
    assert len(re.findall(r"# halo check dim:\d buf:\d \(mpi-host\): 1 bad ghost cells", p.stdout)) == 4, p.stdout


@mpi
def test_overlap_json_record(tmp_path):
    import json

    j = tmp_path / "steps.jsonl"
    run_app(*ARGS, "--overlap", "--dim=0", "--buf=0", f"--json={j}", np=2)
    (rec,) = [json.loads(ln) for ln in j.read_text().splitlines()]
    assert rec["step_serial_us_median_max_rank"] > 0 and rec["step_overlap_us_median_max_rank"] > 0
    assert 0 <= rec["step_err_max"] < 2 * N_LOCAL / 192
    j0 = tmp_path / "plain.jsonl"
    run_app(*ARGS, "--dim=0", "--buf=0", f"--json={j0}", np=2)
    (rec0,) = [json.loads(ln) for ln in j0.read_text().splitlines()]
    assert not [k for k in rec0 if k.startswith("step_")]
    assert [k for k in rec if not k.startswith("step_")] == list(rec0)


def _step_bench(env):
    from gpu_mpi_tests_amd import engine

    return engine.deriv_step_bench(N_LOCAL, 512, n_iter=6, n_warmup=1, env=env, check=True)


@pytest.mark.parametrize("world", [1, 2])
def test_engine_deriv_step_bench(world):
    from mp_util import run_dist

    ensure_host_build()
    res = run_dist(_step_bench, world, free_port(), timeout=120)
    assert len(res) == world
    for r in res:
        for d in (0, 1):
            v = r[f"dim{d}"]
            print(f"world {world} dim {d}: {v}")
            assert v["serial_median_s"] > 0 and v["overlap_median_s"] > 0
            assert v["err_norm"] < 1e-5
            assert 0 <= v["step_err_max"] < N_LOCAL * world / 192
            assert v["bad_ghosts"] == 0
