"""gmt_mg_restrict_tab and gmt_mg_prolong_add_tab on the GPU
(csrc/kernels/mg.hip) against the NumPy model of tests/mg_tab_cases.py.

Everything outside a kernel's read set is NaN, everything outside its output
region a sentinel that must be bitwise intact afterwards; inputs are compared
bitwise before and after; outputs are bitwise NumPy.  x regions are the whole
axis and every share of its 2- and 3-way splits (both tap halo sides, both
coarse ring ends, an odd coarse width with its single last column), 766 -> 382
wraps the lane numbering around a 256-lane workgroup.  Only the all-aligned
variant may take the fast path: the path of every case is asserted.  Every
table index a kernel uses was checked on the host by gmt_mg_xfer_plan_create;
descriptions that fail that check create no plan and nothing is launched."""
import types

import numpy as np
import pytest
import torch

import mg_tab_cases as tc
from gpu_mpi_tests_amd import _native, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.lib()


def _impl():
    return types.SimpleNamespace(lib=_native.lib(), has_paths=True, stream=torch.cuda.current_stream().cuda_stream,
                                 upload=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(),
                                 download=lambda t: t.cpu().numpy(), ptr=lambda t: t.data_ptr())


XPAIRS = tc.X_AXES + (tc.WIDE,)
_ids = [f"{n}to{m}" for n, m in XPAIRS]


def test_case_set():
    tc.assert_coverage()


@pytest.mark.parametrize("xpair", XPAIRS, ids=_ids)
def test_restrict_tab_shapes(xpair):
    assert tc.run_restrict_shapes(_impl(), xpair) == tc.n_cases(xpair) * len(tc.ALIGN_R)


@pytest.mark.parametrize("xpair", XPAIRS, ids=_ids)
def test_prolong_tab_shapes(xpair):
    assert tc.run_prolong_shapes(_impl(), xpair) == tc.n_cases(xpair) * len(tc.ALIGN_P)


def test_empty_regions_and_refusals():
    codes = tc.run_empty_and_refusals(_impl())
    assert codes == [1] * tc.N_REFUSALS, codes  # the CPU backend's codes (tests/test_mg_tab_kernels_cpu.py)


def _t(field):
    st = torch.from_numpy(field.store).cuda()
    return st[field.off:field.off + field.rows * field.ld].view(field.rows, field.ld)


def test_ops_wrappers():
    """ops.mg_*_tab and their path queries give the C ABI's results; a refused description raises before any launch."""
    for xa, ya in tc.case_list((94, 46))[::7] + tc.case_list(tc.WIDE)[::5]:
        d, s, origin, coarse, (mx_, my_) = tc.restrict_fields(xa, ya, "fast")
        want = tc.restrict_reference(d, origin, mx_, my_)
        td, ts = _t(d), _t(s)
        assert ops.mg_restrict_tab_path(td, ts, origin, coarse) == ops.PATH_PT
        assert ops.mg_restrict_tab_path(td, ts, origin, (coarse[0] + 1, coarse[1])) == ops.PATH_SCALAR
        assert ops.mg_restrict_tab(td, ts, xa, ya, origin, coarse) is ts
        (cx0, cy0), mx, my = coarse, xa[5], ya[5]
        assert tc.same_bits(ts.cpu().numpy()[cy0:cy0 + my, cx0:cx0 + mx], want), (xa, ya)
        e, u, origin, coarse, (mx_, my_) = tc.prolong_fields(xa, ya, "fast")
        want = tc.prolong_reference(e, u, origin, coarse, mx_, my_)
        te, tu = _t(e), _t(u)
        assert ops.mg_prolong_add_tab_path(te, tu, origin) == ops.PATH_PT
        assert ops.mg_prolong_add_tab_path(te, tu[:, 1:], origin) == ops.PATH_SCALAR
        assert ops.mg_prolong_add_tab(te, tu, xa, ya, origin, coarse) is tu
        (x0, y0), nx, ny = origin, xa[3], ya[3]
        assert tc.same_bits(tu.cpu().numpy()[y0:y0 + ny, x0:x0 + nx], want), (xa, ya)
    t = torch.zeros(40, 40, dtype=torch.float64, device="cuda")
    for xa, ya in tc.BAD_DESCS:
        with pytest.raises(ValueError, match="refused"):
            ops.mg_restrict_tab(t, torch.zeros_like(t), xa, ya, (2, 2), (1, 1))
    with pytest.raises(ValueError, match="share storage"):
        ops.mg_prolong_add_tab(t, t, tc.share(22, 10, 0, 22), tc.share(22, 10, 0, 22), (1, 1), (1, 1))
    assert bool((t == 0).all())
