"""gmt_ipc_exchange (csrc/kernels/ipc.hip) called directly, in one process:
every case of tests/ipc_cases.py against its byte-exact NumPy model — the
vector and the byte path, strided sources and destinations, both parity
slots, the chunk table and its grid-stride walk, zero-byte channels, the flags,
the epoch and the role counters after every launch, eager and replayed from
a captured graph — and the plans gmt_ipc_plan_init must refuse."""
import pytest
import torch

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


@pytest.mark.parametrize("name", ipc_cases.CASE_NAMES)
def test_ipc_exchange_matches_model(rt, name):
    case = ipc_cases.CASES[ipc_cases.CASE_NAMES.index(name)]
    log = []
    assert ipc_cases.run_case(rt, case, log) == "ok"
    assert len(log) == (len(ipc_cases.GRAPH_TURNS) if case["graph"] else ipc_cases.EXCHANGES) >= 6


def test_the_parametrisation_is_the_whole_table():
    """No case left out silently: one test id per case of the table."""
    assert len(set(ipc_cases.CASE_NAMES)) == len(ipc_cases.CASES) == 21


def test_plan_refusals(rt):
    assert ipc_cases.run_refusals(rt) == ipc_cases.N_REFUSALS
