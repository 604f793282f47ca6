"""The communication kernels that no kernel-level test called: gmt_slices_reduce
(csrc/kernels/reduce.hip — the solve-to-tolerance mode decides convergence on
its output), gmt_stage_copy / gmt_stage_scatter with rows == 0
(csrc/kernels/stage.hip: the aligned loop, its remainder, the byte tail, the
byte loop), gmt_signal_wait eager and from a captured graph, and gmt_fill_poly
modes 3, 4 and 5.  The checks are tests/comm_cases.py, which the CPU backend
runs too (tests/test_ipc_cpu.py); everything is bitwise except mode 3."""
import pytest
import torch

import comm_cases
import ipc_cases
from gpu_mpi_tests_amd import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = ipc_cases.Rt(_native.lib())
    assert r.hip
    yield r
    r.close()


@pytest.mark.parametrize("nslices", comm_cases.SLICE_COUNTS)
def test_slices_reduce_matches_numpy_loop(rt, nslices):
    """n in {1, 255, 256, 257, 4099}: sum and fmax in rank order, with inf and
    NaN in slice 0, a middle and the last slice; out of place and in place."""
    assert comm_cases.run_slices(rt, ns_list=(nslices,)) == 5 * 4 + 7


@pytest.mark.parametrize("shift", comm_cases.STAGE_SHIFTS)
def test_stage_contiguous_chunks(rt, shift):
    """Chunks of 0 .. 2^20 + 40 bytes in one table, 1 / 4 / 300 workgroups,
    then scattered back with 1 / 3 workgroups per chunk."""
    assert comm_cases.run_stage(rt, shifts=(shift,)) == 5


def test_signal_wait_eager_and_replayed(rt):
    assert comm_cases.run_signal_wait(rt) == "graph"


def test_fill_poly_lattice_modes(rt):
    assert comm_cases.run_fill(rt) == 3
